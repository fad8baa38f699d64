"""Host side of the band solves of sparse problems (band.py, engine / solver dispatch), without a GPU.

FakeBandContext adds the band entry points of _cabi.Context to FakeSparseContext: its band solve is SciPy's zgbtrf / zgbtrs
on the permuted band, the same LAPACK semantics csrc/band.hip implements."""
import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp

from adaptive_matrix_solver_amd.band import band_bytes_per_solve, band_order, band_widths
from test_sparse_host import FakeSparseContext


class FakeBandContext(FakeSparseContext):
    """FakeSparseContext plus maus_band_* (zgbtrf / zgbtrs) and a device of `hbm_total` bytes."""

    def __init__(self, hbm_total=288 << 30):
        super().__init__()
        self.hbm_total = hbm_total
        self.band = None
        self.calls["band"] = 0

    def set_matrix_csr(self, A):
        self.band = None
        super().set_matrix_csr(A)

    def device_info(self):
        return {"name": "fake (NumPy test double)", "cus": 0, "hbm_total": self.hbm_total, "hbm_free": self.hbm_total}

    def sparse_max_n(self):
        return 1 << 20

    def band_prepare(self, perm):
        perm = np.asarray(perm, dtype=np.int64)
        n = self.rows
        if perm.shape != (n,) or not np.array_equal(np.sort(perm), np.arange(n)):
            raise ValueError("perm is not a permutation of 0..n-1")
        kl, ku = band_widths(self.A, perm)
        self.band = (perm, kl, ku)
        return kl, ku

    def band_reserve(self, count):
        assert self.band is not None
        return int(count)

    def lu_reserve(self, n, count):
        if self.band is not None:
            raise AssertionError("the band path never reserves the dense LU workspace")
        return super().lu_reserve(n, count)

    def shifted_lu_solve(self, *a, **kw):
        if self.band is not None:
            raise AssertionError("the band path never calls shifted_lu_solve")
        return super().shifted_lu_solve(*a, **kw)

    def band_solve(self, slots, shift, psi, rhs_mode=0):
        perm, kl, ku = self.band
        n = self.rows
        status = np.zeros(len(slots), dtype=np.int32)
        B = sp.csr_matrix(self.A)[perm][:, perm]
        for k, s in enumerate(slots):
            self.calls["band"] += 1
            H = (B - shift[k] * sp.identity(n, dtype=np.complex128) + psi[k] * sp.identity(n, dtype=np.complex128)).tocoo()
            ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
            ab[kl + ku + H.row - H.col, H.col] = H.data
            rhs = (self.pop[0][s, :n] if rhs_mode == 0 else self.b)[perm]
            if not (np.all(np.isfinite(ab)) and np.all(np.isfinite(rhs))):
                status[k] = -1
                continue
            lu, piv, info = lapack.zgbtrf(ab, kl, ku)
            if info > 0:
                status[k] = info
                continue
            y, _ = lapack.zgbtrs(lu, kl, ku, rhs, piv)
            if not np.all(np.isfinite(y)):
                status[k] = -2
                continue
            x = np.empty(n, dtype=np.complex128)
            x[perm] = y
            self.pop[2][s, :n] = x
        return status


def five_point(m):
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    return (sp.kron(sp.identity(m), T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(m))).tocsr()


def _kl_ku_from_coo(A, perm):
    """Half-bandwidths by a separate route: the permuted COO's offsets."""
    P = sp.coo_matrix(sp.csr_matrix(A)[perm][:, perm])
    return max(0, int((P.row - P.col).max())), max(0, int((P.col - P.row).max()))


# ---- band_order ---------------------------------------------------------------------------------------------------
def test_band_order_five_point():
    A = five_point(32)
    rng = np.random.default_rng(0)
    p = rng.permutation(A.shape[0])
    S = A[p][:, p].tocsr()
    perm, kl, ku = band_order(S)
    assert (kl, ku) == _kl_ku_from_coo(S, perm)
    assert kl <= 33 and ku <= 33                       # about m after RCM, against ~n for the shuffled order
    assert np.array_equal(np.sort(perm), np.arange(S.shape[0]))
    again = band_order(S.copy())
    assert np.array_equal(again[0], perm) and again[1:] == (kl, ku)


def test_band_order_tridiagonal_keeps_identity():
    A = sp.diags([1.0, 2.0, 3.0], [-1, 0, 1], shape=(50, 50)).tocsr()
    perm, kl, ku = band_order(A)
    assert np.array_equal(perm, np.arange(50)) and (kl, ku) == (1, 1)


def test_band_order_identity_wins_for_a_lower_band():
    n = 40                                              # upper band kl = 0, ku = 3: ldab 4; RCM of the symmetrised pattern cannot beat it
    A = sp.diags([2 * np.ones(n), np.ones(n - 1), np.ones(n - 3)], [0, 1, 3], shape=(n, n)).tocsr()
    perm, kl, ku = band_order(A)
    assert np.array_equal(perm, np.arange(n)) and (kl, ku) == (0, 3)
    _, klr, kur = band_order(A[::-1][:, ::-1].tocsr())   # the same matrix reversed: RCM finds a better ordering than the identity
    assert 2 * klr + kur + 1 < 2 * 3 + 0 + 1


def test_band_order_random_pattern():
    A = sp.random(300, 300, density=0.01, random_state=3, format="csr") + sp.identity(300)
    perm, kl, ku = band_order(A)
    assert (kl, ku) == _kl_ku_from_coo(A, perm)
    ident_w = 2 * band_widths(A, np.arange(300))[0] + band_widths(A, np.arange(300))[1] + 1
    assert 2 * kl + ku + 1 <= ident_w


# ---- keyword, environment, validation -------------------------------------------------------------------------------
def _engine(ctx=None, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx or FakeBandContext(), pert_mode="mt19937", sparse_mode="device", **kw)


def test_sparse_direct_keyword_default_env_and_bad_values(monkeypatch):
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.delenv("MAUS_SPARSE_DIRECT", raising=False)
    assert _engine().sparse_direct == "auto"
    assert _engine(sparse_direct="band").sparse_direct == "band"
    monkeypatch.setenv("MAUS_SPARSE_DIRECT", "dense")
    assert _engine().sparse_direct == "dense"
    assert InverseIterateSolver(4, 1e-20, 3).sparse_direct == "dense"
    with pytest.raises(ValueError):
        _engine(sparse_direct="banded")
    monkeypatch.setenv("MAUS_SPARSE_DIRECT", "lu")
    with pytest.raises(ValueError):
        _engine()
    with pytest.raises(ValueError):
        InverseIterateSolver(4, 1e-20, 3)


def test_choice_is_made_at_bind_time():
    eng = _engine()
    small = five_point(8).astype(np.complex128)
    eng.bind_matrix(small)
    assert not eng._band                              # auto, n <= 16384: today's densified LU
    big = five_point(142).astype(np.complex128)        # n = 20164
    eng.bind_matrix(big)
    assert eng._band and eng.ctx.band is None         # chosen at bind time, the ordering prepared at the first band solve
    eng.prepare_band()
    assert eng.ctx.band is not None and eng.ctx.band[1:] == band_order(big)[1:]
    eng.bind_matrix(small)
    assert not eng._band
    eng2 = _engine(sparse_direct="band")
    eng2.bind_matrix(small)
    assert eng2._band


# ---- MAUS_Solver above n = 16384 -----------------------------------------------------------------------------------
def _linear(m=142, seed=1):
    A = (five_point(m) * (1.0 + 0.25j)).tocsr()
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(A.shape[0]) + 1j * rng.standard_normal(A.shape[0])
    return A, b


def _solver(A, b, ctx=None, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    eng = _engine(ctx, **{k: kw.pop(k) for k in ("sparse_direct", "gmres_compat") if k in kw})
    ptype = kw.pop("ptype", ProblemType.SOLVE_LINEAR_SYSTEM)
    return MAUS_Solver(A, ptype, b_vector=b if ptype == ProblemType.SOLVE_LINEAR_SYSTEM else None, initial_num_candidates=4,
                       quiet=True, engine=eng, sparse_mode="device", diag_info=_diag(A), **kw)


def _diag(A):
    return {"is_sparse_init": True, "condition_number": 10.0, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}


def test_auto_accepts_sparse_linear_above_16384():
    A, b = _linear()
    s = _solver(A, b)
    assert s.engine._band


def test_dense_above_16384_still_raises():
    A, b = _linear()
    with pytest.raises(NotImplementedError, match="16384"):
        _solver(A, b, sparse_direct="dense")


def test_band_too_wide_is_refused_with_n_kl_ku_and_bytes():
    A, b = _linear()
    n = A.shape[0]
    perm, kl, ku = band_order(A)
    per = band_bytes_per_solve(n, kl, ku)
    with pytest.raises(NotImplementedError) as e:
        _solver(A, b, ctx=FakeBandContext(hbm_total=16 * per - 1))
    msg = str(e.value)
    assert f"n = {n}" in msg and f"kl = {kl}" in msg and f"ku = {ku}" in msg and str(per) in msg
    _solver(A, b, ctx=FakeBandContext(hbm_total=16 * per))          # exactly 1/16 is accepted


def test_above_sparse_max_n_is_refused():
    class Tiny(FakeBandContext):
        def sparse_max_n(self):
            return 20000
    A, b = _linear()
    with pytest.raises(NotImplementedError, match="20000"):
        _solver(A, b, ctx=Tiny())


@pytest.mark.parametrize("compat", ["scipy-legacy", "rtol"])
def test_loop_bodies_above_16384(compat):
    A, b = _linear()
    np.random.seed(5)
    s = _solver(A, b, gmres_compat=compat)
    eng = s.engine
    solve, solves = eng._solve, [0]

    def no_draws(*a, **kw):                             # the solve phase of a sparse problem draws nothing from NumPy
        before = np.random.get_state()
        solve(*a, **kw)
        after = np.random.get_state()
        assert before[2] == after[2] and np.array_equal(before[1], after[1])
        solves[0] += 1

    eng._solve = no_draws
    for it in range(2):
        s.loop_body(it + 1)
    assert solves[0] > 0
    if compat == "scipy-legacy":
        assert eng.ctx.calls["band"] > 0
    checked = 0
    for c in s.candidates:
        if np.isfinite(c.residual_k):
            r = np.linalg.norm(A @ c.x_k - b)
            assert abs(r - c.residual_k) <= 1e-9 * max(r, 1e-300) + 1e-12 * np.linalg.norm(b)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("compat", ["scipy-legacy", "rtol"])
def test_band_and_dense_paths_keep_the_same_bookkeeping_and_stream(compat):
    """sparse_direct='band' against today's densified path at n = 4096: the solves draw nothing from NumPy either way, and
    the candidates' bookkeeping and the stream position agree exactly."""
    import random
    from adaptive_matrix_solver_amd.solver import SolutionCandidate
    A, b = _linear(m=64, seed=2)
    out = []
    for mode in ("dense", "band"):
        np.random.seed(9); random.seed(9); SolutionCandidate._candidate_id_counter = 0
        s = _solver(A, b, gmres_compat=compat, sparse_direct=mode)
        for it in range(3):
            s.loop_body(it + 1)
        out.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                    np.random.get_state()[2], np.random.get_state()[1].copy(), s.engine.ctx.calls["band"]))
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == 0 and (out[1][3] > 0 or compat == "rtol")


def test_prologue_linear_above_16384_uses_the_band_solve(monkeypatch):
    A, b = _linear()
    s = _solver(A, b)
    monkeypatch.setattr(type(A), "todense", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("todense")))
    x = s._reference_solution()
    assert x is not None
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b)


def test_prologue_eigen_above_16384_is_skipped(capsys):
    from adaptive_matrix_solver_amd.solver import ProblemType
    A, _ = _linear()
    s = _solver(A, None, ptype=ProblemType.EIGENVALUE)
    assert s._reference_solution() is None
    assert "not computed" in capsys.readouterr().out


def test_prologue_at_or_below_16384_is_unchanged():
    A, b = _linear(m=20)
    s = _solver(A, b)
    x = s._reference_solution()
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b)
    assert not s.engine._band
