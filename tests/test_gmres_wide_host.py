"""Host side of sparse_gmres="wide" (the device-wide GMRES post step of csrc/gmres.hip), without a GPU: the keyword
and its environment variable, what the engine and the solvers tell the context and when, the binding's names, and the new
case table (every decision of every case at least gc.GUARD from its threshold, so the device's counts can be demanded equal)."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as gc
import gmres_wide_cases as gw
from test_band_host import _diag, _linear, five_point
from test_sparse_host import FakeSparseContext


class RecordingContext(FakeSparseContext):
    """FakeSparseContext plus the method calls of _cabi.Context; GMRES itself is the double's in either method."""

    def __init__(self):
        super().__init__()
        self.method = 0
        self.log = []                                    # ("bind", "csr" | "dense") / ("set_method", m) / ("gmres", method at the time)

    def set_matrix(self, A):
        self.log.append(("bind", "dense"))
        super().set_matrix(A)

    def set_matrix_csr(self, A):
        self.log.append(("bind", "csr"))
        super().set_matrix_csr(A)

    def gmres_set_method(self, method):
        assert method in (0, 1)
        self.method = int(method)
        self.log.append(("set_method", int(method)))

    def gmres_method(self):
        return self.method

    def gmres(self, *a, **kw):
        self.log.append(("gmres", self.method))
        return super().gmres(*a, **kw)


def _engine(ctx, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx, pert_mode="mt19937", sparse_mode="device", **kw)


def test_mode_validator_keyword_environment_and_bad_values(monkeypatch):
    from adaptive_matrix_solver_amd.engine import SPARSE_GMRES_MODES, sparse_gmres_mode
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_GMRES", raising=False)
    assert SPARSE_GMRES_MODES == ("auto", "wide")
    assert sparse_gmres_mode(None) == "auto" and sparse_gmres_mode("auto") == "auto" and sparse_gmres_mode("wide") == "wide"
    assert _engine(RecordingContext()).sparse_gmres == "auto"           # the default does not move
    assert _engine(RecordingContext(), sparse_gmres="wide").sparse_gmres == "wide"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_gmres == "auto"
    assert InverseIterateSolver(4, 1e-20, 3, sparse_gmres="wide").sparse_gmres == "wide"
    monkeypatch.setenv("MAUS_SPARSE_GMRES", "wide")
    assert sparse_gmres_mode(None) == "wide"
    assert _engine(RecordingContext()).sparse_gmres == "wide"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_gmres == "wide"
    assert sparse_gmres_mode("auto") == "auto"                          # an explicit keyword wins
    assert _engine(RecordingContext(), sparse_gmres="auto").sparse_gmres == "auto"
    for bad in ("wid", "stream", "", "Wide"):
        with pytest.raises(ValueError) as e:
            sparse_gmres_mode(bad)
        assert all(m in str(e.value) for m in SPARSE_GMRES_MODES)
        with pytest.raises(ValueError):
            _engine(RecordingContext(), sparse_gmres=bad)
        with pytest.raises(ValueError):
            InverseIterateSolver(4, 1e-20, 3, sparse_gmres=bad)
    monkeypatch.setenv("MAUS_SPARSE_GMRES", "broad")
    with pytest.raises(ValueError):
        sparse_gmres_mode(None)
    with pytest.raises(ValueError):
        _engine(RecordingContext())


@pytest.mark.parametrize("mode,calls", [("wide", [1]), ("auto", [])])
def test_engine_sets_method_1_only_under_wide_and_only_for_a_sparse_matrix(mode, calls):
    ctx = RecordingContext()
    eng = _engine(ctx, sparse_gmres=mode)
    assert ctx.log == []                                                # nothing before a matrix is bound
    eng.bind_matrix(gc.spread(12, 3))
    assert ctx.log == [("bind", "dense")]                               # a dense matrix: the method is never touched
    eng.bind_matrix(five_point(4).astype(np.complex128))
    assert ctx.log[1:] == [("bind", "csr")] + [("set_method", m) for m in calls]
    eng.bind_matrix(gc.spread(12, 4))
    assert [e for e in ctx.log if e[0] == "set_method"] == [("set_method", m) for m in calls]


def test_auto_works_on_a_context_without_the_entry():
    """tests/fake_ctx.py and its descendants have no gmres_set_method: 'auto' never asks for it, 'wide' does."""
    A = five_point(4).astype(np.complex128)
    assert not hasattr(FakeSparseContext(), "gmres_set_method")
    _engine(FakeSparseContext(), sparse_gmres="auto").bind_matrix(A)
    with pytest.raises(AttributeError):
        _engine(FakeSparseContext(), sparse_gmres="wide").bind_matrix(A)


@pytest.mark.parametrize("mode,method", [("wide", 1), ("auto", 0)])
def test_solver_loop_body_runs_gmres_under_the_method(mode, method):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    A, b = _linear(m=12, seed=2)
    ctx = RecordingContext()
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=4, quiet=True,
                    engine=_engine(ctx, sparse_gmres=mode), sparse_mode="device",
                    diag_info=dict(_diag(A), condition_number=np.inf))      # what the diagnostics report of a sparse matrix
    s.loop_body(1)
    solves = [e for e in ctx.log if e[0] == "gmres"]
    assert solves and all(e == ("gmres", method) for e in solves)        # sparse problems start with GMRES preferred
    if method:
        assert ctx.log.index(("set_method", 1)) < ctx.log.index(solves[0])


def test_maus_solver_forwards_the_keyword(monkeypatch):
    from adaptive_matrix_solver_amd import solver
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    seen = []

    def fake_engine(**kw):
        seen.append(kw)
        return _engine(RecordingContext(), sparse_gmres=kw["sparse_gmres"])

    monkeypatch.setattr(solver, "DeviceEngine", fake_engine)
    monkeypatch.delenv("MAUS_SPARSE_GMRES", raising=False)
    A, b = _linear(m=6, seed=3)
    for given, want in ((None, "auto"), ("auto", "auto"), ("wide", "wide")):
        kw = {} if given is None else {"sparse_gmres": given}
        s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=4, quiet=True, sparse_mode="device",
                        diag_info=_diag(A), cond_exact_max=None, **kw)
        assert seen[-1]["sparse_gmres"] == want and s.engine.sparse_gmres == want
    with pytest.raises(ValueError):
        MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, quiet=True, sparse_mode="device", diag_info=_diag(A),
                    sparse_gmres="wider")


def test_inverse_iterate_solver_states_the_method_at_every_solve(monkeypatch):
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    ctx = RecordingContext()
    monkeypatch.setattr(InverseIterateSolver, "_engine", ctx)
    n = 30
    A = sp.csr_matrix(gc.banded(n, 1))
    b = np.arange(1, n + 1, dtype=np.complex128)
    kw = dict(is_sparse=True, sparse_mode="device")
    x, _ = InverseIterateSolver(n, np.complex128(1e-20), 25, "iterative_gmres", **kw).solve(A, b, 0)
    assert [e for e in ctx.log if e[0] != "bind"] == [("gmres", 0)]      # auto on a context at its default: nothing set
    x1, _ = InverseIterateSolver(n, np.complex128(1e-20), 25, "iterative_gmres", sparse_gmres="wide", **kw).solve(A, b, 0)
    assert [e for e in ctx.log if e[0] != "bind"][1:] == [("set_method", 1), ("gmres", 1)]
    InverseIterateSolver(n, np.complex128(1e-20), 25, "iterative_gmres", **kw).solve(A, b, 0)
    assert [e for e in ctx.log if e[0] != "bind"][3:] == [("set_method", 0), ("gmres", 0)]   # the shared context goes back
    assert np.linalg.norm(A @ x - b) <= 1e-8 * np.linalg.norm(b) and np.linalg.norm(A @ x1 - b) <= 1e-8 * np.linalg.norm(b)


def test_binding_names_the_entries_the_constants_and_the_class():
    from adaptive_matrix_solver_amd import _cabi
    assert (_cabi.GMRES_DEFAULT, _cabi.GMRES_WIDE) == (0, 1)
    for name in ("maus_gmres_set_method", "maus_gmres_get_method", "maus_gmres_kernel_for"):
        assert name in _cabi.SYMBOLS
    assert _cabi.KC_NAMES[-1] == "gmres_wide" and _cabi.KC_NAMES.index("band_wide") == 16     # appended: earlier classes keep their numbers
    lib = _cabi.load_library()
    assert lib.maus_gmres_set_method(None, 1) == -1 and lib.maus_gmres_get_method(None) == -1   # no context: an error, no fault
    for m in ("gmres_set_method", "gmres_method", "gmres_kernel_for"):
        assert callable(getattr(_cabi.Context, m))


# ---- the case table ----------------------------------------------------------------------------------------------------
def test_sizes_sit_on_the_piece_and_on_the_join():
    assert gw.WIDE_SIZES == (511, 512, 513, 131071, 131072, 131073)
    names = [c["name"] for c in gw.CASES]
    assert len(names) == 24 and not set(names) & set(gc.BY_NAME)


@pytest.mark.parametrize("name", [c["name"] for c in gw.CASES])
def test_every_wide_case_keeps_its_decisions_off_the_thresholds(name):
    """As test_gmres_cases_host.py demands of the old table.  All 24 converge (info 0) in 1 to 3 cycles of 17 to 46 inner
    iterations, and the double passes the checker the device is held to."""
    case = gw.BY_NAME[name]
    (x, info, inner, cycles, closest), = gw.reference(name)
    assert closest >= gc.GUARD, (name, closest)
    assert info == 0 and 17 <= inner <= 46 and 1 <= cycles <= 3, (name, info, inner, cycles)
    assert ((cycles == 1) if "_w0_" in name else (cycles >= 2)), (name, cycles)
    if case["build"]()["B"].shape[1] <= 513:                              # the double's GMRES is SciPy-in-Python: the small sizes
        gw.check_case(case, gc.run_case(FakeSparseContext(), case))
