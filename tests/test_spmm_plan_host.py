"""Host side of sparse_spmm="sell" (the lane-per-row SpMM on a sliced-ELL copy, csrc/spmm.hip), without a GPU: the
rule as the library states it (maus_spmm_plan is host arithmetic), the keyword and its environment variable, what the engine
and the solvers tell the context and when, the binding's names, and a NumPy restatement of the layout."""
import numpy as np
import pytest
import scipy.sparse as sp

import sell_cases as sc
from fake_ctx import FakeContext
from test_sparse_host import FakeSparseContext

ROWS, WAVE, SELL = 1, 2, 3


class RecordingSparseContext(FakeSparseContext):
    """FakeSparseContext plus the SpMM method calls of _cabi.Context."""

    def __init__(self):
        super().__init__()
        self.spmm, self.log = 0, []

    def spmm_set_method(self, method, fill_cap_percent=0):
        assert method in (0, 1) and (fill_cap_percent == 0 or 100 <= fill_cap_percent <= 1000000)
        self.spmm = int(method)
        self.log.append(("spmm", int(method), int(fill_cap_percent)))

    def spmm_method(self):
        return self.spmm


def _engine(ctx, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx, pert_mode="uniform", sparse_mode="device", **kw)


def _plan(*a):
    from adaptive_matrix_solver_amd._cabi import spmm_plan
    return spmm_plan(*a)


# (method, cap, rows, nnz, padded) -> kind
PLAN_TABLE = [
    ((0, 0, 100, 500, 640), ROWS),                      # method 0 never takes the copy
    ((0, 0, 100, 3201, 6400), WAVE),
    ((1, 0, 100, 500, 640), SELL),
    ((1, 0, 100, 500, 1000), SELL),                     # padded == 2 nnz: inside the default cap
    ((1, 0, 100, 500, 1001), ROWS),                     # one slot more
    ((1, 200, 100, 500, 1000), SELL),                   # 200 said out loud is the default
    ((1, 200, 100, 500, 1001), ROWS),
    ((1, 100, 128, 640, 640), SELL),                    # cap 100: only a copy without padding
    ((1, 100, 128, 640, 704), ROWS),
    ((1, 0, 100, 3200, 3200), SELL),                    # nnz == 32 rows: still a lane per row
    ((1, 0, 100, 3201, 3264), WAVE),                    # nnz == 32 rows + 1: a wave per row, never the copy
    ((1, 1000000, 100, 3201, 3264), WAVE),
    ((1, 0, 100, 0, 0), ROWS),                          # nothing stored: nothing to copy
    ((1, 1000000, 100, 0, 0), ROWS),
    ((1, 1000000, 1, 1, 64), SELL),                     # 1 x 1 under the largest cap (fill 64)
    ((1, 0, 1, 1, 64), ROWS),
    ((1, 258, 200, 1191, 3072), SELL),                  # the cap is compared as 100 padded <= cap nnz
    ((1, 257, 200, 1191, 3072), ROWS),
    ((1, 0, 1 << 26, (1 << 31) - 1, (1 << 31) + 64), SELL),   # padded beyond 2^31
    ((1, 0, 1 << 26, (1 << 31) - 1, (1 << 32) - 64), SELL),   # 2 nnz = 2^32 - 2
    ((1, 0, 1 << 26, (1 << 31) - 1, 1 << 32), ROWS),
    ((1, 1000000, 1 << 26, (1 << 31) - 1, 1 << 40), SELL),
]


@pytest.mark.parametrize("args,kind", PLAN_TABLE)
def test_plan_table(args, kind):
    assert _plan(*args) == kind


def test_plan_rejects_bad_arguments():
    from adaptive_matrix_solver_amd import _cabi
    lib = _cabi.load_library()
    for bad in ((2, 0, 10, 10, 64), (-1, 0, 10, 10, 64), (1, 99, 10, 10, 64), (1, 1000001, 10, 10, 64), (1, -200, 10, 10, 64),
                (1, 0, 0, 0, 0), (1, 0, -5, 10, 64), (1, 0, 10, -1, 64), (1, 0, 10, 10, -64)):
        with pytest.raises(_cabi.MausHipError):
            _plan(*bad)
        assert lib.maus_spmm_plan(*bad, None) == -1
    assert lib.maus_spmm_plan(1, 0, 10, 10, 64, None) == 0            # no place for the answer: still no fault


def test_plan_agrees_with_the_restated_rule_on_the_test_matrices():
    """The fills the issue quotes, from the NumPy layout, and the library's verdict on them under the default cap."""
    A5, A27 = sc.random_pattern(200, 5), sc.random_pattern(4096, 27)
    assert round(sc.fill(A5), 2) == 1.29 and round(sc.fill(sc.adjoint(A5)), 2) == 2.58
    assert round(sc.fill(A27), 2) == 1.00 and round(sc.fill(sc.adjoint(A27)), 2) == 1.47
    mats = [A5, sc.adjoint(A5), A27, sc.adjoint(A27), sc.random_pattern(2048, 100), sc.empty_slice_200(), sc.ragged_256(),
            sc.rect(200, 70, 3), sc.rect(70, 200, 4)] + [sc.tridiagonal(n) for n in (1, 63, 64, 65, 129)]
    for A in mats:
        for method, cap in ((0, 0), (1, 0), (1, 100), (1, sc.FORCE)):
            got = _plan(method, cap, A.shape[0], A.nnz, sc.sell_layout(A)[2])
            assert got == sc.expected_kind(A, method, cap), (A.shape, A.nnz, method, cap)
    # rectangular: the schedule is the matrix's (nnz against the rows of A) for both operands, never the operand's own
    for A, kinds in ((sc.wide_10x1000(), (WAVE, WAVE)), (sc.tall_1000x10(), (SELL, SELL))):
        AH = sc.adjoint(A)
        assert (A.nnz > 32 * A.shape[0]) != (AH.nnz > 32 * AH.shape[0])      # the two operands alone would disagree
        for M, kind in zip((A, AH), kinds):
            assert _plan(1, sc.FORCE, A.shape[0], M.nnz, sc.sell_layout(M)[2]) == kind == sc.expected_kind(M, 1, sc.FORCE, A.shape[0])
            assert _plan(0, 0, A.shape[0], M.nnz, sc.sell_layout(M)[2]) == (WAVE if kind == WAVE else ROWS)
    assert _plan(1, 0, 200, A5.nnz, sc.sell_layout(A5)[2]) == SELL
    assert _plan(1, 0, 200, A5.nnz, sc.sell_layout(sc.adjoint(A5))[2]) == ROWS


def test_layout_restatement():
    """off, len and the positions: every entry lands once, in its row's CSR order, at off[s] + 64 p + (r & 63); what is left is
    padding; a lane-per-row walk over the layout gives the CSR product."""
    for A in (sc.tridiagonal(1), sc.tridiagonal(64), sc.tridiagonal(65), sc.tridiagonal(129), sc.empty_slice_200(),
              sc.ragged_256(), sc.rect(70, 200, 4)):
        off, ln, padded = sc.sell_layout(A)
        ns = -(-A.shape[0] // 64)
        assert off.shape == (ns + 1,) and off[0] == 0 and padded == off[-1] and padded % 64 == 0
        assert np.array_equal(ln, np.diff(A.indptr)) and ln.sum() == A.nnz
        for s in range(ns):
            assert (off[s + 1] - off[s]) // 64 == ln[64 * s: 64 * s + 64].max(initial=0)
        val, idx = sc.sell_arrays(A)
        assert np.count_nonzero(val) == np.count_nonzero(A.data) and padded >= A.nnz
        x = np.random.default_rng(0).standard_normal(A.shape[1]) + 0j
        y = np.zeros(A.shape[0], dtype=np.complex128)
        for r in range(A.shape[0]):
            for p in range(ln[r]):
                q = off[r >> 6] + 64 * p + (r & 63)
                assert idx[q] == A.indices[A.indptr[r] + p]
                y[r] += val[q] * x[idx[q]]
        assert np.allclose(y, A @ x, rtol=1e-13, atol=1e-13)
    off, ln, padded = sc.sell_layout(sc.tridiagonal(129))
    assert off.tolist() == [0, 192, 384, 512] and padded == 512         # the last slice holds one row of two entries
    off, _, padded = sc.sell_layout(sc.empty_slice_200())
    assert off[2] == off[1]                                             # rows 64..127 emptied: a slice of width 0


def test_mode_validator_keyword_environment_and_bad_values(monkeypatch):
    from adaptive_matrix_solver_amd.engine import SPARSE_SPMM_MODES, sparse_spmm_mode
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_SPMM", raising=False)
    assert SPARSE_SPMM_MODES == ("auto", "csr", "sell")
    assert [sparse_spmm_mode(m) for m in (None, "auto", "csr", "sell")] == ["auto", "auto", "csr", "sell"]
    assert _engine(RecordingSparseContext()).sparse_spmm == "auto"      # the default does not move
    assert _engine(RecordingSparseContext(), sparse_spmm="sell").sparse_spmm == "sell"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_spmm == "auto"
    assert InverseIterateSolver(4, 1e-20, 3, sparse_spmm="sell").sparse_spmm == "sell"
    monkeypatch.setenv("MAUS_SPARSE_SPMM", "sell")
    assert sparse_spmm_mode(None) == "sell"
    assert _engine(RecordingSparseContext()).sparse_spmm == "sell"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_spmm == "sell"
    assert sparse_spmm_mode("auto") == "auto"                           # an explicit keyword wins
    assert _engine(RecordingSparseContext(), sparse_spmm="csr").sparse_spmm == "csr"
    for bad in ("ell", "SELL", "", 1):
        with pytest.raises(ValueError) as e:
            sparse_spmm_mode(bad)
        assert all(m in str(e.value) for m in SPARSE_SPMM_MODES)
        with pytest.raises(ValueError):
            _engine(RecordingSparseContext(), sparse_spmm=bad)
        with pytest.raises(ValueError):
            InverseIterateSolver(4, 1e-20, 3, sparse_spmm=bad)
    monkeypatch.setenv("MAUS_SPARSE_SPMM", "wide")
    with pytest.raises(ValueError):
        sparse_spmm_mode(None)


def test_engine_sets_the_method_once_and_auto_and_csr_never_ask(monkeypatch):
    """FakeContext and FakeSparseContext have no spmm_set_method: 'auto' and 'csr' never ask for it, 'sell' does, when the
    engine is created."""
    monkeypatch.delenv("MAUS_SPARSE_SPMM", raising=False)
    assert not hasattr(FakeContext(), "spmm_set_method") and not hasattr(FakeSparseContext(), "spmm_set_method")
    A = sc.tridiagonal(12)
    for mode in ("auto", "csr"):
        eng = _engine(FakeSparseContext(), sparse_spmm=mode)
        eng.bind_matrix(A)
        assert eng.sparse_spmm == mode and eng.ctx.matrix_is_sparse() == "rows"
        _engine(FakeContext(), sparse_spmm=mode).bind_matrix(A.toarray())
    with pytest.raises(AttributeError):
        _engine(FakeSparseContext(), sparse_spmm="sell")
    ctx = RecordingSparseContext()
    eng = _engine(ctx, sparse_spmm="sell")
    assert ctx.log == [("spmm", 1, 0)]
    eng.bind_matrix(A)
    eng.bind_matrix(sp.csr_matrix(2 * A))
    assert ctx.log == [("spmm", 1, 0)] and ctx.spmm_method() == 1       # kept across matrices, said once
    for mode in ("auto", "csr"):
        ctx = RecordingSparseContext()
        _engine(ctx, sparse_spmm=mode).bind_matrix(A)
        assert ctx.log == []


def test_maus_solver_forwards_the_keyword(monkeypatch):
    from adaptive_matrix_solver_amd import solver
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    seen = []

    def fake_engine(**kw):
        seen.append(kw)
        return _engine(RecordingSparseContext(), sparse_spmm=kw["sparse_spmm"])

    monkeypatch.setattr(solver, "DeviceEngine", fake_engine)
    monkeypatch.delenv("MAUS_SPARSE_SPMM", raising=False)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((6, 6)) + 1j * rng.standard_normal((6, 6))
    for given, want in ((None, "auto"), ("auto", "auto"), ("csr", "csr"), ("sell", "sell")):
        kw = {} if given is None else {"sparse_spmm": given}
        s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=4, quiet=True, cond_exact_max=None, **kw)
        assert seen[-1]["sparse_spmm"] == want and s.engine.sparse_spmm == want
        assert s.engine.ctx.log == ([("spmm", 1, 0)] if want == "sell" else [])
    with pytest.raises(ValueError):
        MAUS_Solver(A, ProblemType.EIGENVALUE, quiet=True, sparse_spmm="ell")


def test_inverse_iterate_solver_states_the_method_at_every_sparse_solve(monkeypatch):
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    ctx = RecordingSparseContext()
    monkeypatch.setattr(InverseIterateSolver, "_engine", ctx)
    monkeypatch.delenv("MAUS_SPARSE_SPMM", raising=False)
    n = 12
    A = sc.tridiagonal(n)
    b = np.arange(1, n + 1, dtype=np.complex128)
    kw = dict(is_sparse=True, sparse_mode="device")
    InverseIterateSolver(n, np.complex128(1e-20), 25, **kw).solve(A, b, 0)
    assert ctx.log == []                                                # auto on a context at its default: nothing set
    InverseIterateSolver(n, np.complex128(1e-20), 25, sparse_spmm="sell", **kw).solve(A, b, 0)
    assert ctx.log == [("spmm", 1, 0)]
    InverseIterateSolver(n, np.complex128(1e-20), 25, sparse_spmm="csr", **kw).solve(A, b, 0)
    assert ctx.log == [("spmm", 1, 0), ("spmm", 0, 0)]                  # the shared context goes back
    # a context without the entry points (FakeSparseContext) keeps working under 'auto' and 'csr'
    plain = FakeSparseContext()
    monkeypatch.setattr(InverseIterateSolver, "_engine", plain)
    for mode in ("auto", "csr"):
        x, _ = InverseIterateSolver(n, np.complex128(1e-20), 25, sparse_spmm=mode, **kw).solve(A, b, 0)[:2]
        assert np.linalg.norm(A @ x - b) <= 1e-8 * np.linalg.norm(b)


def test_binding_names_the_entries_and_the_constants():
    from adaptive_matrix_solver_amd import _cabi
    assert (_cabi.SPMM_CSR, _cabi.SPMM_SELL) == (0, 1)
    assert (_cabi.SPMM_KERNEL_NONE, _cabi.SPMM_KERNEL_ROWS, _cabi.SPMM_KERNEL_WAVE, _cabi.SPMM_KERNEL_SELL) == (0, 1, 2, 3)
    header = open(_cabi.LIB_PATH.replace("adaptive_matrix_solver_amd/libmaus_hip.so", "include/maus_hip.h")).read()
    lib = _cabi.load_library()
    for name in ("maus_spmm_set_method", "maus_spmm_get_method", "maus_spmm_kernel_for", "maus_spmm_plan", "maus_spmm_sell_info"):
        assert name in _cabi.SYMBOLS and f"int {name}(" in header       # declared, listed
        assert getattr(lib, name).argtypes is not None                  # exported and bound
    # no context: an error, no fault
    assert lib.maus_spmm_set_method(None, 1, 0) == -1 and lib.maus_spmm_get_method(None) == -1
    assert lib.maus_spmm_kernel_for(None, 0) == -1 and lib.maus_spmm_sell_info(None, 0, None, None, None) == -1
    for m in ("spmm_set_method", "spmm_method", "spmm_kernel_for", "spmm_sell_info"):
        assert callable(getattr(_cabi.Context, m))
