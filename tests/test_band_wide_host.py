"""Host side of sparse_direct="wide" (the two-level band LU of csrc/band.hip), without a GPU: the keyword and its
environment variable, what the engine tells the context and when, the rule and the size rule."""
import pytest

from adaptive_matrix_solver_amd import band
from adaptive_matrix_solver_amd.band import band_bytes_per_solve, band_order, runs_blocked, runs_tiled
from test_band_host import FakeBandContext, _diag, _linear


class FakeWideContext(FakeBandContext):
    """FakeBandContext plus the method calls of _cabi.Context (there is no method 3); the band solve itself is LAPACK's in
    every method."""

    def __init__(self, hbm_total=288 << 30):
        super().__init__(hbm_total)
        self.method = 0
        self.log = []                                    # ("set_method", m) / ("solve", method at the time)

    def band_set_method(self, method):
        assert method in (0, 1, 2, 4)
        self.method = int(method)
        self.log.append(("set_method", int(method)))

    def band_method(self):
        return self.method

    def band_solve(self, slots, shift, psi, rhs_mode=0):
        self.log.append(("solve", self.method))
        return super().band_solve(slots, shift, psi, rhs_mode)


def _engine(ctx, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx, pert_mode="mt19937", sparse_mode="device", **kw)


def _solver(A, b, ctx, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    return MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=4, quiet=True,
                       engine=_engine(ctx, **kw), sparse_mode="device", diag_info=_diag(A))


def test_wide_is_accepted_by_keyword_and_environment(monkeypatch):
    from adaptive_matrix_solver_amd.engine import SPARSE_DIRECT_MODES
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_DIRECT", raising=False)
    assert "wide" in SPARSE_DIRECT_MODES
    assert SPARSE_DIRECT_MODES[:5] == ("auto", "dense", "band", "blocked", "tiled")       # the earlier modes keep their places
    assert SPARSE_DIRECT_MODES[-1] == "wide"
    assert _engine(FakeWideContext(), sparse_direct="wide").sparse_direct == "wide"
    assert InverseIterateSolver(4, 1e-20, 3, sparse_direct="wide").sparse_direct == "wide"
    assert _engine(FakeWideContext()).sparse_direct == "auto"           # the default does not move
    assert _engine(FakeWideContext(), sparse_direct="wide").uses_band(10)
    monkeypatch.setenv("MAUS_SPARSE_DIRECT", "wide")
    assert _engine(FakeWideContext()).sparse_direct == "wide"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_direct == "wide"
    assert _engine(FakeWideContext(), sparse_direct="band").sparse_direct == "band"       # an explicit keyword wins
    assert InverseIterateSolver(4, 1e-20, 3, sparse_direct="tiled").sparse_direct == "tiled"
    for bad in ("wid", "wider"):
        with pytest.raises(ValueError) as e:
            _engine(FakeWideContext(), sparse_direct=bad)
        assert all(m in str(e.value) for m in SPARSE_DIRECT_MODES)
        with pytest.raises(ValueError) as e:
            InverseIterateSolver(4, 1e-20, 3, sparse_direct=bad)
        assert all(m in str(e.value) for m in SPARSE_DIRECT_MODES)


@pytest.mark.parametrize("mode,calls", [("wide", [4]), ("tiled", [2]), ("blocked", [1]), ("band", []), ("auto", [])])
def test_prepare_band_sets_method_4_exactly_in_this_mode(mode, calls):
    A, b = _linear(m=142 if mode == "auto" else 64, seed=2)
    ctx = FakeWideContext()
    s = _solver(A, b, ctx, sparse_direct=mode, gmres_compat="scipy-legacy")
    s.loop_body(1)
    assert [m for what, m in ctx.log if what == "set_method"] == calls
    solves = [e for e in ctx.log if e[0] == "solve"]
    assert solves and all(e == ("solve", calls[0] if calls else 0) for e in solves)
    if calls:
        assert ctx.log.index(("set_method", calls[0])) < ctx.log.index(solves[0])


def test_runs_wide_matches_the_rule():
    assert (band.WIDE_MIN_KL, band.WIDE_MAX_KL, band.WIDE_NBO) == (64, 4096, 64)
    assert [band.runs_wide(kl, 40) for kl in (63, 64, 4096, 4097)] == [False, True, True, False]
    assert band.runs_wide(64, 0) and band.runs_wide(4096, 5000) and not band.runs_wide(63, 5000)     # ku plays no part
    # the other rules stay
    assert [runs_tiled(kl, 40) for kl in (15, 16, 1024, 1025, 4096, 4097)] == [False, True, True, True, True, False]
    assert [runs_blocked(kl, 40) for kl in (15, 16, 1024, 1025)] == [False, True, True, False]


def test_band_bytes_per_solve_wide():
    n = 5000
    for kl, ku in ((64, 3), (1024, 900), (1025, 600), (4096, 1000)):   # wide runs: tiled's panel and reach, plus LW
        base = 16 * ((2 * kl + ku + 1) * n + n) + 4 * n
        assert band_bytes_per_solve(n, kl, ku) == base
        assert band_bytes_per_solve(n, kl, ku, wide=True) == base + 16 * (kl + 16) * 16 + 4 + 16 * (kl + 64) * 64
        assert band_bytes_per_solve(n, kl, ku, wide=True) == band_bytes_per_solve(n, kl, ku, tiled=True) + 16 * (kl + 64) * 64
    for kl, ku in ((16, 3), (33, 17), (63, 500)):                      # below the outer block's width: what tiled runs
        assert band_bytes_per_solve(n, kl, ku, wide=True) == band_bytes_per_solve(n, kl, ku, tiled=True)
        assert band_bytes_per_solve(n, kl, ku, wide=True) > band_bytes_per_solve(n, kl, ku)
    for kl, ku in ((15, 40), (4097, 10), (0, 0)):                      # outside: the column kernel
        assert band_bytes_per_solve(n, kl, ku, wide=True) == band_bytes_per_solve(n, kl, ku)
    # the earlier keywords and the positional `blocked` keep their meaning
    assert band_bytes_per_solve(n, 300, 20, True) == band_bytes_per_solve(n, 300, 20, blocked=True)
    assert band_bytes_per_solve(n, 300, 20, True, False) == band_bytes_per_solve(n, 300, 20, blocked=True)
    assert band_bytes_per_solve(n, 300, 20, False, True) == band_bytes_per_solve(n, 300, 20, tiled=True)
    assert band_bytes_per_solve(n, 300, 20, tiled=True) == 16 * ((2 * 300 + 20 + 1) * n + n) + 4 * n + 16 * 316 * 16 + 4
    assert band_bytes_per_solve(n, 1025, 600, blocked=True) == band_bytes_per_solve(n, 1025, 600)


def test_too_wide_refusal_names_the_wide_bytes():
    A, b = _linear()
    n = A.shape[0]
    perm, kl, ku = band_order(A)
    assert band.runs_wide(kl, ku)
    per = band_bytes_per_solve(n, kl, ku)
    per_w = band_bytes_per_solve(n, kl, ku, wide=True)
    assert per_w == per + 16 * (kl + 16) * 16 + 4 + 16 * (kl + 64) * 64
    with pytest.raises(NotImplementedError) as e:
        _solver(A, b, FakeWideContext(hbm_total=16 * per_w - 1), sparse_direct="wide")
    assert f"n = {n}" in str(e.value) and str(per_w) in str(e.value)
    _solver(A, b, FakeWideContext(hbm_total=16 * per_w), sparse_direct="wide")
    _solver(A, b, FakeBandContext(hbm_total=16 * per_w - 1), sparse_direct="band")        # today's bytes for today's modes
