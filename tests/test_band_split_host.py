"""The split beside the band method (sparse_split="on", maus_band_set_split) without a device: the C rule against band.py over
every boundary, the partition's invariants, the keyword, and the NumPy model of tests/split_cases.py against LAPACK."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack

import split_cases as sc
from adaptive_matrix_solver_amd import _cabi, band

# kl + ku in {0, 1, 2, 30, 31, 32} and kl in {0, 1, 15, 16}
RULE_SHAPES = [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (15, 15), (1, 29), (15, 16), (0, 31), (1, 30), (16, 15), (16, 0), (16, 16),
               (15, 17), (0, 32), (1, 31)]


def _sizes(kl, ku, part_len):
    """n on both sides of two partitions of the forced or planned length, and up to 2^20."""
    w = kl + ku
    out = {1, 2, 2 * w + 2, 2 * w + 3, 2 * w + 4, 63, 64, 65, 127, 128, 129, 1000, 4096, 65536, 1 << 20}
    if part_len:
        out |= {part_len - 1, part_len, part_len + 1, 2 * part_len, 2 * part_len + 1}
    for n in list(out):                                                  # the rule's own boundary: n against split_len(n)
        if w >= 1 and n >= 1:
            m = band.split_len(n, kl, ku)
            out |= {m - 1, m, m + 1}
    return sorted(n for n in out if n >= 1)


@pytest.mark.parametrize("kl,ku", RULE_SHAPES)
def test_split_plan_matches_band_py(kl, ku):
    w = kl + ku
    in_range = 1 <= w <= 31 and kl <= 15
    for part_len in (0, 2 * w + 1, 2 * w + 2):
        if part_len and part_len < 2 * w + 2 and in_range:               # refused where the band is in range
            with pytest.raises(_cabi.MausHipError):
                _cabi.band_split_plan(0, 500, kl, ku, part_len)
            with pytest.raises(ValueError):
                band.runs_split(500, kl, ku, part_len)
            continue
        for n in _sizes(kl, ku, part_len):
            for method in (0, 1, 2, 4, 8):
                takes, m, p, n_red, klr, kur, per = _cabi.band_split_plan(method, n, kl, ku, part_len)
                assert takes == band.runs_split(n, kl, ku, part_len), (n, kl, ku, part_len)
                assert per == band.split_bytes_per_solve(n, kl, ku, part_len, method), (n, kl, ku, part_len, method)
                if not takes:
                    assert (m, p, n_red, klr, kur, per) == (0, 0, 0, 0, 0, 0)
                    assert not in_range or n <= (part_len or band.split_len(n, kl, ku))
                    continue
                assert in_range and p >= 2 and n > m
                assert m == (part_len or band.split_len(n, kl, ku)) and m >= 2 * w + 2
                assert (p, n_red, klr, kur) == band.split_shape(n, kl, ku, part_len)
                assert n_red == (p - 1) * w and klr < 2 * w and kur < 2 * w
                if method == 0:
                    assert per == 16 * n * (2 * w + 2) + 16 * ((2 * klr + kur + 1) * n_red + 2 * n_red) + 4 * n_red + 12


def test_split_len_rule():
    for n, kl, ku in [(1 << 20, 1, 1), (1 << 20, 15, 15), (65536, 2, 2), (262144, 1, 1), (700, 15, 15), (100, 1, 1), (3, 0, 1)]:
        w = kl + ku
        m = band.split_len(n, kl, ku)
        assert m >= 2 * w + 2
        if m > 2 * w + 2:
            assert m % 64 == 0 and m >= np.sqrt(n * w) > m - 64
    assert band.split_len(1 << 20, 1, 1) == 1472 and band.split_len(1 << 20, 15, 15) == 5632


def test_split_plan_refuses_bad_input():
    lib = _cabi.load_library()
    for args in [(0, -1, 1, 1, 0), (0, 100, -1, 1, 0), (0, 100, 1, -1, 0), (0, 100, 1, 1, -1), (3, 100, 1, 1, 0), (16, 100, 1, 1, 0)]:
        assert lib.maus_band_split_plan(*args, *([None] * 7)) == -1, args
    assert lib.maus_band_split_plan(8, 1000, 1, 1, 0, *([None] * 7)) == 0          # every out pointer may be NULL
    assert lib.maus_band_set_split(None, 1, 0) == -1 and lib.maus_band_get_split(None, None) == -1
    for name in ("maus_band_set_split", "maus_band_get_split", "maus_band_split_plan"):
        assert name in _cabi.SYMBOLS
    # the method table and the plan of every method are what they were
    assert band.DIRECT_METHOD == {"band": 0, "blocked": 1, "tiled": 2, "narrow": 8, "wide": 4}
    assert _cabi.band_plan(8, 1 << 20, 1, 1)[:3] == (8, 1, 0) and _cabi.band_plan(8, 1 << 20, 1, 1)[3] == band.band_bytes_per_solve(1 << 20, 1, 1)
    assert _cabi.KC_BAND_SPLIT == len(_cabi.KC_NAMES) == 18


@pytest.mark.parametrize("kl,ku", sc.SHAPES)
def test_partition_invariants(kl, ku):
    w = kl + ku
    m0 = 2 * w + 2
    for m in (m0, 64 if 64 > m0 else m0 + 7):
        for n in (m + 1, 2 * m - 1, 2 * m, 3 * m + w - 1, 5 * m + 1):
            parts = sc.partitions(n, kl, ku, m)
            p, n_red, _, _ = band.split_shape(n, kl, ku, m)
            assert len(parts) == p and band.runs_split(n, kl, ku, m)
            nxt, left = 0, 0
            for i, (a, b, r0, r1, s0, s1) in enumerate(parts):
                assert r0 == nxt and r1 > r0                             # the R_i tile [0, n)
                nxt = r1
                assert b >= a and s1 - s0 == (0 if i == p - 1 else w)
                assert (r0, r1) == (max(a - ku, 0), min(b + kl, n - 1) + 1)
                extra = (r1 - r0) - (b - a + 1)
                assert extra == (kl if i == 0 else ku if i == p - 1 else w)
                left += extra
                for r in range(r0, r1):                                  # every row of R_i touches I_i, and nothing outside S_{i-1}, I_i, S_i
                    assert max(r - kl, a) <= min(r + ku, b)
                    assert r - kl >= a - w and min(r + ku, n - 1) <= (n - 1 if i == p - 1 else s1 - 1)
            assert nxt == n and left == n_red
            Q = sc.column_order(n, kl, ku, m)
            assert np.array_equal(np.sort(Q), np.arange(n))


def test_keyword_and_env(monkeypatch):
    from adaptive_matrix_solver_amd import engine
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_SPLIT", raising=False)
    assert engine.sparse_split_mode(None) == "off" and engine.sparse_split_mode("on") == "on"
    monkeypatch.setenv("MAUS_SPARSE_SPLIT", "on")
    assert engine.sparse_split_mode(None) == "on" and engine.sparse_split_mode("off") == "off"
    assert InverseIterateSolver(8, 1e-3, 2).sparse_split == "on"
    monkeypatch.setenv("MAUS_SPARSE_SPLIT", "yes")
    with pytest.raises(ValueError, match="sparse_split"):
        engine.sparse_split_mode(None)
    with pytest.raises(ValueError, match="sparse_split"):
        InverseIterateSolver(8, 1e-3, 2, sparse_split="auto")
    monkeypatch.delenv("MAUS_SPARSE_SPLIT")
    assert InverseIterateSolver(8, 1e-3, 2).sparse_split == "off"
    assert engine.SPARSE_SPLIT_MODES == ("off", "on")


class _Ctx:
    """Records what prepare_band tells the context."""
    def __init__(self):
        self.calls = []

    def band_set_split(self, on, part_len=0):
        self.calls.append(("split", on, part_len))

    def band_set_method(self, m):
        self.calls.append(("method", m))

    def band_prepare(self, perm):
        self.calls.append(("prepare",))
        return 1, 1


@pytest.mark.parametrize("mode,expect", [("off", []), ("on", [("split", True, 0)])])
def test_prepare_band_touches_the_context_only_when_on(mode, expect):
    import scipy.sparse as sp
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    ctx = _Ctx()
    eng = DeviceEngine(ctx=ctx, sparse_mode="device", sparse_direct="band", sparse_split=mode)
    eng._bound = sp.identity(8, format="csr", dtype=np.complex128)
    eng.prepare_band()
    assert [c for c in ctx.calls if c[0] == "split"] == expect
    assert ("method", 0) not in ctx.calls and ctx.calls[-1] == ("prepare",)


CASES = [(kl, ku, n) for kl, ku in sc.SHAPES for n in (2 * (2 * (kl + ku) + 2) + 1, 257)]


@pytest.mark.parametrize("kl,ku,n", CASES)
def test_model_solves_to_the_bound(kl, ku, n):
    """omega of the model against omega of LAPACK on H[:, Q]: the bound the device is held to."""
    m = 2 * (kl + ku) + 2
    H, ab, b = sc.band_case(n, kl, ku, 100 + kl * 32 + ku)
    x, st, piv, sure = sc.split_reference(ab, b, kl, ku, m)
    assert st == 0
    om, om_ref = sc.omega(H, x, b), sc.model_omega(H, b, kl, ku, m)
    print(f"({kl},{ku}) n={n}: omega model {om:.3g}, LAPACK on H[:, Q] {om_ref:.3g}")
    assert om <= 8 * max(om_ref, sc.EPS)
    parts = sc.partitions(n, kl, ku, m)
    inter = [c for a, bb, *_ in parts for c in range(a, bb + 1)]
    assert len(set(piv[inter])) == len(inter)                            # a row is a pivot row once


@pytest.mark.parametrize("kl,ku,n,zero_cols", [
    (1, 1, 40, (7,)), (2, 2, 100, (9,)), (2, 2, 100, (0,)), (2, 2, 100, (99,)), (3, 2, 90, (30, 8, 70)), (0, 4, 61, (25,)),
    (4, 0, 61, (3, 9)), (7, 24, 400, (130, 200)), (15, 15, 200, (61,)),
])
def test_model_status_is_zgbtrf_info(kl, ku, n, zero_cols):
    """Planted zero columns in an interior, a separator (m = 2 w + 2: columns m - w .. m - 1), the first and the last column."""
    m = 2 * (kl + ku) + 2
    H, ab, b = sc.band_case(n, kl, ku, 7, zero_cols=zero_cols)
    _, _, info = lapack.zgbtrf(ab, kl, ku)
    assert info == min(zero_cols) + 1
    with np.errstate(all="ignore"):
        _, st, _, _ = sc.split_reference(ab, b, kl, ku, m)
    assert st == info
