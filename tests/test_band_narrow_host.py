"""Host side of sparse_direct="narrow" (the streaming band LU for narrow bands of csrc/band.hip), without a GPU:
the keyword and its environment variable, what the engine tells the context and when, the rule and the size rule."""
import numpy as np
import pytest
import scipy.sparse as sp

from adaptive_matrix_solver_amd import band
from adaptive_matrix_solver_amd.band import band_bytes_per_solve, band_order
from test_band_host import FakeBandContext, _diag


class FakeNarrowContext(FakeBandContext):
    """FakeBandContext plus the method calls of _cabi.Context (methods 0, 1, 2, 4 and 8); the band solve itself is LAPACK's
    in every method."""

    def __init__(self, hbm_total=288 << 30):
        super().__init__(hbm_total)
        self.method = 0
        self.log = []                                    # ("set_method", m) / ("solve", method at the time)

    def band_set_method(self, method):
        assert method in (0, 1, 2, 4, 8)
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


def _tridiagonal(n=600, seed=4):
    """Non-Hermitian complex tridiagonal operator, strictly diagonally dominant, and a right-hand side."""
    rng = np.random.default_rng(seed)
    lo = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    up = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    A = sp.diags([0.3 * lo, 4.0 + 1j + 0.1 * rng.standard_normal(n), 0.3 * up], [-1, 0, 1], format="csr")
    return A, rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _solver(A, b, ctx, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    return MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=4, quiet=True,
                       engine=_engine(ctx, **kw), sparse_mode="device", diag_info=_diag(A))


def test_narrow_is_accepted_by_keyword_and_environment(monkeypatch):
    from adaptive_matrix_solver_amd.engine import SPARSE_DIRECT_MODES
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_DIRECT", raising=False)
    assert SPARSE_DIRECT_MODES == ("auto", "dense", "band", "blocked", "tiled", "narrow", "wide")
    assert _engine(FakeNarrowContext(), sparse_direct="narrow").sparse_direct == "narrow"
    assert InverseIterateSolver(4, 1e-20, 3, sparse_direct="narrow").sparse_direct == "narrow"
    assert _engine(FakeNarrowContext()).sparse_direct == "auto"         # the default does not move
    assert InverseIterateSolver(4, 1e-20, 3).sparse_direct == "auto"
    assert _engine(FakeNarrowContext(), sparse_direct="narrow").uses_band(10)          # at every n, as 'band'
    assert _engine(FakeNarrowContext(), sparse_direct="narrow").uses_band(1 << 20)
    monkeypatch.setenv("MAUS_SPARSE_DIRECT", "narrow")
    assert _engine(FakeNarrowContext()).sparse_direct == "narrow"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_direct == "narrow"
    assert _engine(FakeNarrowContext(), sparse_direct="band").sparse_direct == "band"  # an explicit keyword wins
    assert InverseIterateSolver(4, 1e-20, 3, sparse_direct="wide").sparse_direct == "wide"
    for bad in ("narow", "narrower", "window"):
        with pytest.raises(ValueError) as e:
            _engine(FakeNarrowContext(), sparse_direct=bad)
        assert all(m in str(e.value) for m in SPARSE_DIRECT_MODES)
        with pytest.raises(ValueError) as e:
            InverseIterateSolver(4, 1e-20, 3, sparse_direct=bad)
        assert all(m in str(e.value) for m in SPARSE_DIRECT_MODES)


def test_cabi_names_method_8():
    from adaptive_matrix_solver_amd import _cabi
    assert _cabi.BAND_NARROW == 8
    assert (_cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE) == (0, 1, 2, 4)
    assert _cabi.KC_NAMES.index("band") == 12 and "band_narrow" not in _cabi.KC_NAMES  # accounted under `band`: no new class


@pytest.mark.parametrize("mode,calls", [("narrow", [8]), ("band", []), ("auto", [])])
def test_prepare_band_sets_method_8_exactly_in_this_mode(mode, calls):
    A, b = _tridiagonal(20000 if mode == "auto" else 600)
    ctx = FakeNarrowContext()
    s = _solver(A, b, ctx, sparse_direct=mode, gmres_compat="scipy-legacy")
    s.loop_body(1)
    assert [m for what, m in ctx.log if what == "set_method"] == calls
    solves = [e for e in ctx.log if e[0] == "solve"]
    assert solves and all(e == ("solve", calls[0] if calls else 0) for e in solves)
    if calls:
        assert ctx.log.index(("set_method", 8)) < ctx.log.index(solves[0])


def test_runs_narrow_matches_the_rule():
    assert (band.NARROW_MAX_KL, band.NARROW_MAX_KV) == (15, 31)
    inside = [(0, 0), (1, 1), (15, 15), (15, 16), (1, 30), (0, 31)]
    outside = [(16, 1), (15, 17), (0, 32)]
    assert all(band.runs_narrow(kl, ku) for kl, ku in inside)
    assert not any(band.runs_narrow(kl, ku) for kl, ku in outside)
    # the other rules stay
    assert [band.runs_tiled(kl, 40) for kl in (15, 16, 4096, 4097)] == [False, True, True, False]
    assert [band.runs_blocked(kl, 40) for kl in (15, 16, 1024, 1025)] == [False, True, True, False]
    assert [band.runs_wide(kl, 40) for kl in (63, 64, 4096, 4097)] == [False, True, True, False]


def test_band_bytes_per_solve_narrow_adds_nothing():
    n = 5000
    for kl, ku in ((0, 0), (1, 1), (2, 2), (15, 16), (1, 30), (16, 1), (15, 17), (300, 20)):
        base = 16 * ((2 * kl + ku + 1) * n + n) + 4 * n
        assert band_bytes_per_solve(n, kl, ku) == base
        assert band_bytes_per_solve(n, kl, ku, narrow=True) == base
    # the earlier keywords keep their meaning beside it
    assert band_bytes_per_solve(n, 300, 20, tiled=True, narrow=True) == band_bytes_per_solve(n, 300, 20, tiled=True)
    assert band_bytes_per_solve(n, 300, 20, True, False, False, True) == band_bytes_per_solve(n, 300, 20, blocked=True)


def test_maus_solver_linear_tridiagonal_under_narrow():
    A, b = _tridiagonal()
    n = A.shape[0]
    perm, kl, ku = band_order(A)
    assert (kl, ku) == (1, 1) and band.runs_narrow(kl, ku)
    ctx = FakeNarrowContext()
    s = _solver(A, b, ctx, sparse_direct="narrow", gmres_compat="scipy-legacy")
    assert s.engine.sparse_direct == "narrow" and s.engine._band
    s.loop_body(1)
    assert ctx.method == 8 and ctx.calls["band"] > 0
    checked = 0
    for c in s.candidates:
        if np.isfinite(c.residual_k):
            r = np.linalg.norm(A @ c.x_k - b)
            assert abs(r - c.residual_k) <= 1e-8 * r + 1e-12 * np.linalg.norm(b)
            checked += 1
    assert checked > 0
    # the size rule takes the plain bytes: a device that just fits 'band' fits 'narrow'
    per = band_bytes_per_solve(n, kl, ku)
    _solver(A, b, FakeNarrowContext(hbm_total=16 * per), sparse_direct="narrow")
    with pytest.raises(NotImplementedError):
        _solver(A, b, FakeNarrowContext(hbm_total=16 * per - 1), sparse_direct="narrow")
