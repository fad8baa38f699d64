"""Host side of few_rows="splitk" (split-K population products of at most 32 rows, csrc/zgemm.hip, DESIGN §3 "Few rows"),
without a GPU: the keyword and its environment variable, what the engine and the solvers tell the context and when, the
binding's names, and the slicing rule as the library states it (maus_few_rows_plan is host arithmetic: the tests ask it and
carry no copy of its constants)."""
import numpy as np
import pytest

from fake_ctx import FakeContext


class RecordingContext(FakeContext):
    """FakeContext plus the method calls of _cabi.Context."""

    def __init__(self):
        super().__init__()
        self.few, self.log = 0, []

    def few_rows_set_method(self, method, slices=0):
        assert method in (0, 1) and 0 <= slices <= 32
        self.few = int(method)
        self.log.append(("few_rows", int(method), int(slices)))

    def few_rows_method(self):
        return self.few


def _engine(ctx, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx, pert_mode="uniform", **kw)


def test_mode_validator_keyword_environment_and_bad_values(monkeypatch):
    from adaptive_matrix_solver_amd.engine import FEW_ROWS_MODES, few_rows_mode
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_FEW_ROWS", raising=False)
    assert FEW_ROWS_MODES == ("auto", "splitk")
    assert few_rows_mode(None) == "auto" and few_rows_mode("auto") == "auto" and few_rows_mode("splitk") == "splitk"
    assert _engine(RecordingContext()).few_rows == "auto"               # the default does not move
    assert _engine(RecordingContext(), few_rows="splitk").few_rows == "splitk"
    assert InverseIterateSolver(4, 1e-20, 3).few_rows == "auto"
    assert InverseIterateSolver(4, 1e-20, 3, few_rows="splitk").few_rows == "splitk"
    monkeypatch.setenv("MAUS_FEW_ROWS", "splitk")
    assert few_rows_mode(None) == "splitk"
    assert _engine(RecordingContext()).few_rows == "splitk"
    assert InverseIterateSolver(4, 1e-20, 3).few_rows == "splitk"
    assert few_rows_mode("auto") == "auto"                              # an explicit keyword wins
    assert _engine(RecordingContext(), few_rows="auto").few_rows == "auto"
    for bad in ("split", "splitK", "", 1):
        with pytest.raises(ValueError) as e:
            few_rows_mode(bad)
        assert all(m in str(e.value) for m in FEW_ROWS_MODES)
        with pytest.raises(ValueError):
            _engine(RecordingContext(), few_rows=bad)
        with pytest.raises(ValueError):
            InverseIterateSolver(4, 1e-20, 3, few_rows=bad)
    monkeypatch.setenv("MAUS_FEW_ROWS", "wide")
    with pytest.raises(ValueError):
        few_rows_mode(None)


def test_engine_sets_the_method_once_and_auto_never_asks():
    """tests/fake_ctx.py has no few_rows_set_method: 'auto' never asks for it, 'splitk' does, when the engine is created."""
    assert not hasattr(FakeContext(), "few_rows_set_method")
    A = np.eye(6, dtype=np.complex128)
    _engine(FakeContext(), few_rows="auto").bind_matrix(A)
    with pytest.raises(AttributeError):
        _engine(FakeContext(), few_rows="splitk")
    ctx = RecordingContext()
    eng = _engine(ctx, few_rows="splitk")
    assert ctx.log == [("few_rows", 1, 0)]
    eng.bind_matrix(A)
    eng.bind_matrix(2 * A)
    assert ctx.log == [("few_rows", 1, 0)] and ctx.few_rows_method() == 1       # kept across matrices, said once
    ctx = RecordingContext()
    _engine(ctx, few_rows="auto").bind_matrix(A)
    assert ctx.log == []


def test_maus_solver_forwards_the_keyword(monkeypatch):
    from adaptive_matrix_solver_amd import solver
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    seen = []

    def fake_engine(**kw):
        seen.append(kw)
        return _engine(RecordingContext(), few_rows=kw["few_rows"])

    monkeypatch.setattr(solver, "DeviceEngine", fake_engine)
    monkeypatch.delenv("MAUS_FEW_ROWS", raising=False)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((6, 6)) + 1j * rng.standard_normal((6, 6))
    for given, want in ((None, "auto"), ("auto", "auto"), ("splitk", "splitk")):
        kw = {} if given is None else {"few_rows": given}
        s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=4, quiet=True, cond_exact_max=None, **kw)
        assert seen[-1]["few_rows"] == want and s.engine.few_rows == want
        assert s.engine.ctx.log == ([("few_rows", 1, 0)] if want == "splitk" else [])
    with pytest.raises(ValueError):
        MAUS_Solver(A, ProblemType.EIGENVALUE, quiet=True, few_rows="split-k")


def test_inverse_iterate_solver_states_the_method_at_every_solve(monkeypatch):
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    ctx = RecordingContext()
    monkeypatch.setattr(InverseIterateSolver, "_engine", ctx)
    monkeypatch.delenv("MAUS_FEW_ROWS", raising=False)
    n = 12
    rng = np.random.default_rng(5)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) + 4 * np.eye(n)
    b = np.arange(1, n + 1, dtype=np.complex128)
    InverseIterateSolver(n, np.complex128(1e-20), 25).solve(A, b, 0)
    assert ctx.log == []                                                # auto on a context at its default: nothing set
    InverseIterateSolver(n, np.complex128(1e-20), 25, few_rows="splitk").solve(A, b, 0)
    assert ctx.log == [("few_rows", 1, 0)]
    InverseIterateSolver(n, np.complex128(1e-20), 25).solve(A, b, 0)
    assert ctx.log == [("few_rows", 1, 0), ("few_rows", 0, 0)]          # the shared context goes back


def test_binding_names_the_entries_the_constants_and_the_class():
    from adaptive_matrix_solver_amd import _cabi
    assert (_cabi.FEW_ROWS_DEFAULT, _cabi.FEW_ROWS_SPLITK) == (0, 1)
    header = open(_cabi.LIB_PATH.replace("adaptive_matrix_solver_amd/libmaus_hip.so", "include/maus_hip.h")).read()
    lib = _cabi.load_library()
    for name in ("maus_few_rows_set_method", "maus_few_rows_get_method", "maus_few_rows_kernel_for", "maus_few_rows_plan",
                 "maus_few_rows_workspace_allocs"):
        assert name in _cabi.SYMBOLS and f"int {name}(" in header       # declared, listed
        assert getattr(lib, name).argtypes is not None                  # exported and bound
    for ref in ("AMS:264-268", "295-301", "165-175", "227-255", "432-451"):
        assert ref in header
    # no context: an error, no fault
    assert lib.maus_few_rows_set_method(None, 1, 0) == -1 and lib.maus_few_rows_get_method(None) == -1
    assert lib.maus_few_rows_kernel_for(None, 15, 64, 1024, 1, 0, 0, None) == -1
    assert lib.maus_few_rows_workspace_allocs(None) == -1
    for m in ("few_rows_set_method", "few_rows_method", "few_rows_kernel_for", "few_rows_workspace_allocs"):
        assert callable(getattr(_cabi.Context, m))


# ---- the rule, as the library states it ----------------------------------------------------------------------------------
FORMS = [(1, False, False), (1, True, False), (1, False, True), (1, True, True), (0, True, False), (0, False, True), (0, True, True)]
SIZES = [(64, 1024), (1, 1024), (33, 4101), (65, 1029), (768, 768), (2048, 2048), (8192, 8192), (16384, 16384), (15, 8192),
         (32, 16384), (100, 37), (64, 1023), (8192, 16), (8192, 15)]


def _plan(*a, **kw):
    from adaptive_matrix_solver_amd._cabi import few_rows_plan
    return few_rows_plan(*a, **kw)


def test_default_method_never_splits():
    for N, K in SIZES:
        for M in (1, 15, 16, 17, 32, 33):
            for bl, ca, cb in FORMS + [(0, False, False)]:
                assert _plan(0, 0, M, N, K, bl, ca, cb) == (0, 1)
                assert _plan(0, 7, M, N, K, bl, ca, cb) == (0, 1)       # forced slices mean nothing under method 0


def test_split_k_covers_its_forms_and_nothing_else():
    for N, K in SIZES:
        for bl, ca, cb in FORMS:
            assert _plan(1, 0, 33, N, K, bl, ca, cb) == (0, 1)          # 33 rows: the DMA-staged kernels, as ever
            assert _plan(1, 0, 1000, N, K, bl, ca, cb) == (0, 1)
        for M in (1, 16, 32):
            assert _plan(1, 0, M, N, K, 0, False, False) == (0, 1)      # plain layout without conjugation: the LU family's kernels
            assert _plan(1, 8, M, N, K, 0, False, False) == (0, 1)


def test_slices_do_not_depend_on_the_rows():
    for N, K in SIZES:
        for bl, ca, cb in FORMS:
            plans = {_plan(1, 0, M, N, K, bl, ca, cb) for M in range(1, 33)}
            assert len(plans) == 1, (N, K, bl, ca, cb, plans)
            kern, S = plans.pop()
            assert (kern, S) == (0, 1) or (kern == 1 and 2 <= S <= 32 and K // S >= 16)
            forced = {_plan(1, 5, M, N, K, bl, ca, cb) for M in range(1, 33)}
            assert len(forced) == 1


def test_small_shapes_reach_the_path():
    """The one fixed condition of the rule: N <= 64 and K >= 1024 split (so that small tests reach the kernels)."""
    for N in (1, 15, 32, 33, 64):
        for K in (1024, 1029, 4101, 8192, 16384):
            for bl, ca, cb in FORMS:
                kern, S = _plan(1, 0, 15, N, K, bl, ca, cb)
                assert kern == 1 and S >= 2, (N, K, bl, ca, cb)


def test_forced_slices_are_honoured_and_clamped():
    for S in (2, 3, 7, 32):
        for K in (16 * S, 16 * S + 5):
            assert _plan(1, S, 15, 65, K, 1, False, False) == (1, S)
            assert _plan(1, S, 15, 65, K, 0, True, False) == (1, S)
    assert _plan(1, 32, 15, 65, 16 * 7 + 15, 1) == (1, 7)              # no slice shorter than 16
    assert _plan(1, 32, 15, 65, 32, 1) == (1, 2)
    assert _plan(1, 32, 15, 65, 31, 1) == (0, 1)                        # one slice: the default kernels
    assert _plan(1, 1, 15, 64, 4096, 1) == (0, 1)                       # slices = 1 is the default
    assert _plan(1, 3, 3, 33, 53, 1) == (1, 3)
    from adaptive_matrix_solver_amd._cabi import MausHipError
    for bad in ((2, 0, 15, 64, 1024), (-1, 0, 15, 64, 1024), (1, 33, 15, 64, 1024), (1, -1, 15, 64, 1024), (1, 0, 0, 64, 1024),
                (1, 0, 15, 0, 1024), (1, 0, 15, 64, 0)):
        with pytest.raises(MausHipError):
            _plan(*bad)
