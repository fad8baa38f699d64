"""Host side of sparse_direct="blocked" (the blocked band LU of csrc/band.hip), without a GPU: the keyword and its
environment variable, what the engine tells the context and when, the size rule, and that the mode changes nothing on the
host side of a loop body."""
import random

import numpy as np
import pytest

from adaptive_matrix_solver_amd.band import band_bytes_per_solve, band_order, kernel_for, runs_blocked
from test_band_host import FakeBandContext, _diag, _linear, five_point


class FakeBlockedContext(FakeBandContext):
    """FakeBandContext plus the method calls of _cabi.Context; the band solve itself is LAPACK's either way."""

    def __init__(self, hbm_total=288 << 30):
        super().__init__(hbm_total)
        self.method = 0
        self.log = []                                    # ("set_method", m) / ("prepare",) / ("solve", method at the time)

    def band_set_method(self, method):
        assert method in (0, 1)
        self.method = int(method)
        self.log.append(("set_method", int(method)))

    def band_method(self):
        return self.method

    def band_kernel_for(self, n, kl, ku):
        return kernel_for(self.method, kl, ku)

    def band_prepare(self, perm):
        self.log.append(("prepare",))
        return super().band_prepare(perm)

    def band_solve(self, slots, shift, psi, rhs_mode=0):
        self.log.append(("solve", self.method))
        return super().band_solve(slots, shift, psi, rhs_mode)


def _engine(ctx, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx, pert_mode="mt19937", sparse_mode="device", **kw)


def _solver(A, b, ctx, ptype=None, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    ptype = ptype or ProblemType.SOLVE_LINEAR_SYSTEM
    eng = _engine(ctx, **kw)
    return MAUS_Solver(A, ptype, b_vector=b if ptype == ProblemType.SOLVE_LINEAR_SYSTEM else None, initial_num_candidates=4,
                       quiet=True, engine=eng, sparse_mode="device", diag_info=_diag(A))


def test_blocked_is_accepted_by_keyword_and_environment(monkeypatch):
    from adaptive_matrix_solver_amd.engine import SPARSE_DIRECT_MODES
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver, MAUS_Solver, ProblemType
    monkeypatch.delenv("MAUS_SPARSE_DIRECT", raising=False)
    assert "blocked" in SPARSE_DIRECT_MODES
    assert _engine(FakeBlockedContext(), sparse_direct="blocked").sparse_direct == "blocked"
    assert InverseIterateSolver(4, 1e-20, 3, sparse_direct="blocked").sparse_direct == "blocked"
    assert _engine(FakeBlockedContext()).sparse_direct == "auto"        # the default does not move
    A, b = _linear(m=16)
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=2, quiet=True, sparse_mode="device",
                    sparse_direct="blocked", diag_info=_diag(A), engine=_engine(FakeBlockedContext(), sparse_direct="blocked"))
    assert s.engine.sparse_direct == "blocked" and s.engine._band     # the band path at every n, as 'band'
    monkeypatch.setenv("MAUS_SPARSE_DIRECT", "blocked")
    assert _engine(FakeBlockedContext()).sparse_direct == "blocked"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_direct == "blocked"
    for bad in ("block", "banded"):
        with pytest.raises(ValueError, match="blocked") as e:
            _engine(FakeBlockedContext(), sparse_direct=bad)
        assert all(m in str(e.value) for m in SPARSE_DIRECT_MODES)
        with pytest.raises(ValueError, match="blocked"):
            InverseIterateSolver(4, 1e-20, 3, sparse_direct=bad)


def test_engine_hands_the_method_over_before_the_first_band_solve():
    A, b = _linear(m=64, seed=2)
    ctx = FakeBlockedContext()
    s = _solver(A, b, ctx, sparse_direct="blocked", gmres_compat="scipy-legacy")
    assert s.engine.uses_band(10) and s.engine.uses_band(1 << 20)
    for it in range(2):
        s.loop_body(it + 1)                              # FakeBandContext raises on lu_reserve / shifted_lu_solve
    solves = [e for e in ctx.log if e[0] == "solve"]
    assert solves and all(e == ("solve", 1) for e in solves)
    assert ctx.log.index(("set_method", 1)) < ctx.log.index(solves[0])
    assert ("set_method", 0) not in ctx.log
    perm, kl, ku = band_order(A)
    assert ctx.band_kernel_for(A.shape[0], kl, ku) == (1, 16)


@pytest.mark.parametrize("mode", ["band", "auto"])
def test_other_modes_never_see_the_new_calls(mode):
    """FakeBandContext has no band_set_method / band_method / band_kernel_for: any call would be an AttributeError."""
    A, b = _linear(m=142 if mode == "auto" else 64, seed=2)
    ctx = FakeBandContext()
    assert not hasattr(ctx, "band_set_method")
    s = _solver(A, b, ctx, sparse_direct=mode, gmres_compat="scipy-legacy")
    s.loop_body(1)
    assert ctx.calls["band"] > 0


def test_too_wide_refusal_uses_the_blocked_bytes_only_when_blocked_is_selected():
    A, b = _linear()
    n = A.shape[0]
    perm, kl, ku = band_order(A)
    assert runs_blocked(kl, ku)
    per = band_bytes_per_solve(n, kl, ku)
    assert per == 16 * ((2 * kl + ku + 1) * n + n) + 4 * n              # the three-argument form and its result stay
    per_b = band_bytes_per_solve(n, kl, ku, blocked=True)
    assert per_b == per + 16 * (kl + 16) * 16 + 4                       # the panel of L and the reach
    assert band_bytes_per_solve(n, 3, 2, blocked=True) == band_bytes_per_solve(n, 3, 2)     # a narrow band: the column kernel
    with pytest.raises(NotImplementedError) as e:
        _solver(A, b, FakeBlockedContext(hbm_total=16 * per_b - 1), sparse_direct="blocked")
    assert f"n = {n}" in str(e.value) and str(per_b) in str(e.value)
    _solver(A, b, FakeBlockedContext(hbm_total=16 * per_b), sparse_direct="blocked")
    assert 16 * per <= 16 * per_b - 1
    _solver(A, b, FakeBandContext(hbm_total=16 * per_b - 1), sparse_direct="band")       # today's bytes for today's modes
    _solver(A, b, FakeBandContext(hbm_total=16 * per), sparse_direct="auto")
    with pytest.raises(NotImplementedError, match=str(per)):
        _solver(A, b, FakeBandContext(hbm_total=16 * per - 1), sparse_direct="band")


@pytest.mark.parametrize("kind", ["linear", "eigen"])
def test_blocked_keeps_the_bookkeeping_and_both_streams_of_band(kind):
    from adaptive_matrix_solver_amd.solver import ProblemType, SolutionCandidate
    A, b = _linear(m=64, seed=2)
    assert A.shape[0] == 4096
    ptype = ProblemType.SOLVE_LINEAR_SYSTEM if kind == "linear" else ProblemType.EIGENVALUE
    out = []
    for mode, ctx in (("band", FakeBandContext()), ("blocked", FakeBlockedContext())):
        np.random.seed(9); random.seed(9); SolutionCandidate._candidate_id_counter = 0
        s = _solver(A, b, ctx, ptype=ptype, sparse_direct=mode, gmres_compat="scipy-legacy")
        for it in range(2):
            s.loop_body(it + 1)
        out.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                    np.random.get_state()[2], np.random.get_state()[1].copy(), random.getstate(), ctx.calls["band"]))
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3]
    assert out[0][4] == out[1][4] > 0
