"""The plan of the device vector draws (maus_pop_draw_plan, csrc/mtplan.cpp) and the vector_draws keyword, without a GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive_matrix_solver_amd", "csrc")
MIN_N = 1024
CHUNK = 16 * 312                 # elements per partial sum of the squared norm: sub-streams start on its multiples


@pytest.mark.parametrize("L", [MIN_N, MIN_N + 1, 4368, 4369, 65536, 1 << 20])
def test_every_generator_starts_at_its_word(L):
    """Generator (k, sb, part) starts at stream word pos + 2L (2 ord_k + part) + 2 sb E, reconstructed from the jump strides
    and the (extra, rpos) the plan reports.  4368 = 14 * 312: the draw ends on a block boundary."""
    from adaptive_matrix_solver_amd import _cabi
    assert _cabi.pop_draw_min_len() == MIN_N
    ords = np.array([0, 1, 3, 7, 64, 129, 200], dtype=np.int32)         # gaps; 2 * 129 + 1 > 256: a third hexadecimal digit
    for pos in (624, 1, 312, 623):
        for S in (0, 1, 2, 5, 64):
            pl = _cabi.pop_draw_plan(L, ords, pos, S)
            Sx, E = pl["S"], pl["E"]
            assert Sx == S or S == 0
            assert E % CHUNK == 0 and Sx * E >= L and pl["ngen"] == 2 * len(ords) * Sx
            assert pl["dj"] == (2 * L) // 624 and pl["dj2"] == ((2 * E) // 624 if Sx > 1 else 0)
            assert (pl["extra"] >= 0).all() and ((pl["rpos"] >= 0) & (pl["rpos"] < 624)).all()
            for k, o in enumerate(ords.tolist()):
                for sb in range(Sx):
                    for part in range(2):
                        gi = (k * Sx + sb) * 2 + part
                        word = 624 * ((2 * o + part) * pl["dj"] + sb * pl["dj2"] + int(pl["extra"][gi])) + int(pl["rpos"][gi])
                        assert word == pos + 2 * L * (2 * o + part) + 2 * sb * E, (pos, S, k, sb, part)
            if pos == 624:                                              # a freshly seeded state: its own block is never read
                assert (pl["extra"] >= 1).all()


def test_rule_and_refusals():
    from adaptive_matrix_solver_amd import _cabi
    one = _cabi.pop_draw_plan(MIN_N, [0], 624)
    assert one["S"] == 1 and one["E"] == CHUNK
    # a sub-stream of the rule is at least 256 blocks long, at most 16 per draw
    for L in (65536, 262144, 1 << 20):
        for count in (1, 15, 64):
            S = _cabi.pop_draw_plan(L, np.arange(count), 1)["S"]
            assert 1 <= S <= 16 and (S == 1 or L // S >= 256 * 312)
    assert _cabi.pop_draw_plan(1 << 20, [0], 1)["S"] > 1
    for bad in ((MIN_N - 1, [0], 624, 0), (MIN_N, [0], 625, 0), (MIN_N, [0], -1, 0), (MIN_N, [-1], 624, 0), (MIN_N, [0], 624, -1), (0, [0], 624, 0)):
        with pytest.raises(_cabi.MausHipError):
            _cabi.pop_draw_plan(*bad)


# ---- maus_mt_plan for L = n * n: the plan of the dense regulariser is what it was ------------------------------------------
def _parent_plan(n, pos, ords, wpc, lead, s_override):
    """The arithmetic of maus_mt_plan before it was generalised to draws of L elements, restated."""
    g = len(ords)
    two = 2 * n * n
    s_cap = 64 if n >= 2048 else 16
    S = 1
    while 2 * S <= s_cap and S * max(1, g) < 1024:
        S *= 2
    nn = n * n
    while S > 1 and nn // S < 64 * 312:
        S -= 1
    if s_override > 0:
        S = max(1, min(64, s_override))
    E = (nn + S - 1) // S
    ngen = 2 * g * S
    dj = two // 624
    dj2 = (2 * E) // 624 if S > 1 else 0
    m, bsel, extra, rpos = [0] * ngen, [0] * ngen, [0] * ngen, [0] * ngen
    for k, o in enumerate(ords):
        for sb in range(S):
            for part in range(2):
                gi = (k * S + sb) * 2 + part
                mm = (lead + o * wpc) // two + part
                t = pos + mm * two + 2 * sb * E
                m[gi] = mm if dj else 0
                bsel[gi] = sb if dj2 else 0
                extra[gi] = t // 624 - m[gi] * dj - bsel[gi] * dj2
                rpos[gi] = t % 624
    hs = extra + rpos
    levels = []
    maxm = max(m)
    dig = 0
    while dj and 4 * dig < 64 and (maxm >> (4 * dig)):
        sel, mult = [], []
        for i in range(ngen):
            v = (m[i] >> (4 * dig)) & 15
            if v and (not dj2 or (i // 2) % S == 0):
                sel.append(i)
                mult.append(v)
        if sel:
            levels.append((len(hs), len(sel), (624 * dj) << (4 * dig), 0, 1))
            hs = hs + sel + mult
        dig += 1
    bit = 0
    while dj2 and (1 << bit) < S:
        sel = [i for i in range(ngen) if (1 << bit) <= (i // 2) % S < (2 << bit)]
        if sel:
            levels.append((len(hs), len(sel), 624 * dj2 * (1 << bit), 2 << bit, 0))
            hs = hs + sel
        bit += 1
    return (S, E, ngen, dj, dj2), levels, hs


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mtplan") / "mt_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(CSRC, "mtplan.cpp"), os.path.join(ROOT, "tests", "native", "mt_plan_dump.cpp"),
                    "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("n", [8, 100, 312, 640, 1024, 4096])
def test_matrix_plan_is_unchanged(dump, n):
    for g, ords in ((1, [0]), (7, [0, 1, 2, 4, 9, 17, 300]), (181, list(range(181)))):
        for pos in (624, 1, 623):
            for wpc, lead in ((4 * n * n, 0), (8 * n * n, 4 * n * n)):
                for s_override in (0, 3):
                    out = subprocess.run([dump, str(n), str(pos), str(g), str(wpc), str(lead), str(s_override)] + [str(o) for o in ords],
                                         check=True, capture_output=True, text=True).stdout.split("\n")
                    head = tuple(int(x) for x in out[0].split())
                    nlev = head[5]
                    levels = [tuple(int(x) for x in out[1 + i].split()) for i in range(nlev)]
                    hs = [int(x) for x in out[1 + nlev].split()]
                    want_head, want_levels, want_hs = _parent_plan(n, pos, ords, wpc, lead, s_override)
                    assert head[:5] == want_head, (n, g, pos, wpc, s_override)
                    assert levels == want_levels, (n, g, pos, wpc, s_override)
                    assert hs[0] == len(want_hs) and hs[1:] == want_hs, (n, g, pos, wpc, s_override)


# ---- the keyword -----------------------------------------------------------------------------------------------------------
def test_vector_draws_keyword(monkeypatch):
    import inspect
    from adaptive_matrix_solver_amd import engine, solver
    monkeypatch.delenv("MAUS_VECTOR_DRAWS", raising=False)
    assert engine.vector_draws_mode(None) == "host"
    assert engine.vector_draws_mode("device") == "device" and engine.vector_draws_mode("host") == "host"
    assert engine.vector_draws_mode("auto") == "host"
    monkeypatch.setenv("MAUS_VECTOR_DRAWS", "device")
    assert engine.vector_draws_mode(None) == "device" and engine.vector_draws_mode("host") == "host"
    monkeypatch.setenv("MAUS_VECTOR_DRAWS", "gpu")
    with pytest.raises(ValueError):
        engine.vector_draws_mode(None)
    with pytest.raises(ValueError):
        engine.vector_draws_mode("Device")
    for f in (solver.MAUS_Solver.__init__, engine.DeviceEngine.__init__):
        assert inspect.signature(f).parameters["vector_draws"].default is None


def test_engine_default_is_host_and_defers_nothing(monkeypatch):
    """On the CPU double of the context the default engine draws on the host; 'device' on a context without maus_pop_draw
    (the double) registers nothing either: the bracket stays the transfer bracket it was."""
    from fake_ctx import FakeContext
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    monkeypatch.delenv("MAUS_VECTOR_DRAWS", raising=False)
    eng = DeviceEngine(ctx=FakeContext())
    assert eng.vector_draws == "host"
    eng.begin_deferred_push()
    assert eng._draws is None
    eng.end_deferred_push()
    eng = DeviceEngine(ctx=FakeContext(), vector_draws="device")
    assert eng.vector_draws == "device"
    eng.begin_deferred_push()
    assert eng._draws is None
    eng.end_deferred_push()
    with pytest.raises(ValueError):
        DeviceEngine(ctx=FakeContext(), vector_draws="sometimes")
