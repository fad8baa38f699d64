"""Band LU of sparse problem matrices (csrc/band.hip) and GMRES on a CSR matrix above n = 16384, on the device."""
import os

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order

pytestmark = pytest.mark.gpu


def _ctx():
    try:
        return _cabi.Context(0)
    except _cabi.MausHipError as e:
        pytest.skip(f"no device: {e}")


def _band_case(n, kl, ku, seed, zero_cols=()):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    for d in range(-ku, kl + 1):
        m = n - abs(d)
        if m <= 0:
            continue
        v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        A += np.diag(v, -d)
    for j in zero_cols:
        A[:, j] = 0
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    for j in range(n):
        for i in range(max(0, j - ku), min(n, j + kl + 1)):
            ab[kl + ku + i - j, j] = A[i, j]
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, ab, b


@pytest.mark.parametrize("n,kl,ku,zero_cols", [
    (60, 3, 2, ()), (40, 0, 4, ()), (40, 4, 0, ()), (300, 70, 5, ()), (5, 3, 4, ()), (777, 129, 33, ()),
    (200, 1, 1, ()), (90, 5, 7, (17,)), (120, 8, 3, (0, 50)), (1, 0, 0, ()),
])
def test_band_lu_matches_zgbtrf(n, kl, ku, zero_cols):
    ctx = _ctx()
    A, ab, b = _band_case(n, kl, ku, 7 + n + kl, zero_cols)
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)
    x, ipiv, st = ctx.band_lu(ab[None], b[None], kl, ku)
    assert np.array_equal(ipiv[0], piv), (ipiv[0][:20], piv[:20])
    assert st[0] == info
    if info == 0:
        xr, _ = lapack.zgbtrs(lu, kl, ku, b, piv)
        cond = np.linalg.cond(A)
        assert np.linalg.norm(x[0] - xr) <= 1e-12 * cond * np.linalg.norm(xr)


def test_band_lu_batch_and_non_finite_input():
    ctx = _ctx()
    cases = [_band_case(64, 6, 9, s) for s in range(5)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[2, 6 + 9, 10] = np.nan
    x, ipiv, st = ctx.band_lu(ab, b, 6, 9)
    assert st[2] == -1
    for k in (0, 1, 3, 4):
        assert st[k] == 0
        assert np.linalg.norm(cases[k][0] @ x[k] - b[k]) <= 1e-11 * np.linalg.norm(b[k]) * np.linalg.cond(cases[k][0])


def _five_point(m, seed=0):
    """2-D 5-point operator on an m x m grid with complex values, shuffled so that the ordering has work to do."""
    rng = np.random.default_rng(seed)
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    L = (sp.kron(I, T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), I)).tocsr().astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    p = rng.permutation(m * m)
    return L[p][:, p].tocsr()


def _bind(ctx, A, P):
    ctx.set_matrix_csr(A)
    perm, kl, ku = band_order(A)
    assert ctx.band_prepare(perm) == (kl, ku)
    ctx.pop_reserve(P)
    return perm, kl, ku


def test_band_prepare_rejects_bad_orderings():
    ctx = _ctx()
    A = _five_point(8)
    ctx.set_matrix_csr(A)
    with pytest.raises(_cabi.MausHipError, match="permutation"):
        ctx.band_prepare(np.zeros(64, dtype=np.int32))
    with pytest.raises(_cabi.MausHipError):
        ctx.band_prepare(np.arange(63, dtype=np.int32))
    assert ctx.sparse_max_n() == 1 << 20


def test_band_rows_do_not_depend_on_the_batch():
    ctx = _ctx()
    n, P = 4096, 256
    A = _five_point(64, 1)
    _bind(ctx, A, P)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    psi = np.full(P, 1e-3)
    probe = [0, 17, 200]

    def run(c, slots):
        st = c.band_solve(slots, shift[slots], psi[slots], 0)
        assert (st == 0).all()
        return c.pop_get(_cabi.POP_W, probe, n)

    alone = np.stack([run(ctx, np.array([s]))[i] for i, s in enumerate(probe)])
    mid = run(ctx, np.r_[np.arange(0, 32), 200])                        # 33 solves
    full = run(ctx, np.arange(P))
    assert np.array_equal(alone.view(np.float64), mid.view(np.float64))
    assert np.array_equal(alone.view(np.float64), full.view(np.float64))
    os.environ["MAUS_BAND_BATCH"] = "40"
    try:
        c2 = _ctx()
        _bind(c2, A, P)
        c2.pop_put(_cabi.POP_X, np.arange(P), X)
        assert c2.band_reserve(P) == 40
        chunked = run(c2, np.arange(P))
        assert c2.band_workspace_allocations() == 1
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert np.array_equal(alone.view(np.float64), chunked.view(np.float64))
    # a non-finite shift reaches the diagonal: status -1
    st = ctx.band_solve([5], np.array([np.nan + 0j]), np.zeros(1), 0)
    assert st[0] == -1


def test_band_against_spsolve_65536():
    ctx = _ctx()
    m = 256
    n = m * m
    A = _five_point(m, 2)
    perm, kl, ku = _bind(ctx, A, 4)
    assert kl <= 300 and ku <= 300
    rng = np.random.default_rng(4)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.set_rhs(b)
    shift = np.array([0.0, 0.5 + 0.1j, 2.0 - 0.3j, 7.5j])
    psi = np.array([0.0, 1e-3, 0.0, 1e-6])
    st = ctx.band_solve(np.arange(4), shift, psi, 1)
    assert (st == 0).all()
    W = ctx.pop_get(_cabi.POP_W, np.arange(4), n)
    I = sp.identity(n, format="csc", dtype=np.complex128)
    for k in range(4):
        H = (A - shift[k] * I + psi[k] * I).tocsc()
        x = spla.spsolve(H, b)
        assert np.linalg.norm(H @ W[k] - b) <= 1e-10 * np.linalg.norm(b)
        assert np.linalg.norm(W[k] - x) <= 1e-8 * np.linalg.norm(x)


def test_band_against_dense_path_4096():
    ctx = _ctx()
    n, P = 4096, 64
    A = _five_point(64, 5)
    _bind(ctx, A, P)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    psi = np.full(P, 1e-20)
    slots = np.arange(P)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    Wb = ctx.pop_get(_cabi.POP_W, slots, n)
    assert (ctx.shifted_lu_solve(slots, shift, psi, 0) == 0).all()
    Wd = ctx.pop_get(_cabi.POP_W, slots, n)
    for k in range(P):
        assert np.linalg.norm(Wb[k] - Wd[k]) <= 1e-10 * np.linalg.norm(Wd[k])


def _scipy_gmres(H, rhs, jac):
    M = sp.diags(1.0 / H.diagonal(), format="csc") if jac else None
    count = [0]
    x, info = spla.gmres(H, rhs, x0=rhs, rtol=1e-8, restart=20, maxiter=50, M=M,
                         callback=lambda r: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
    return info, count[0], x


@pytest.mark.parametrize("jac", [0, 1])
def test_gmres_65536_matches_scipy(jac):
    ctx = _ctx()
    m = 256
    n = m * m
    A = _five_point(m, 8)
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(4)
    rng = np.random.default_rng(9)
    X = rng.standard_normal((4, n)) + 1j * rng.standard_normal((4, n))
    ctx.pop_put(_cabi.POP_X, np.arange(4), X)
    shift = np.array([0.3, 1.0 + 0.5j, -0.2j, 9.0])
    psi = np.full(4, 1e-20)
    ctx.profile_enable(True)
    info, inner, status = ctx.gmres(np.arange(4), shift, psi, 0, np.full(4, jac, dtype=np.int32))
    prof = ctx.profile_read()
    assert prof["spmm"]["launches"] > 0 and prof["zgemm"]["launches"] == 0
    W = ctx.pop_get(_cabi.POP_W, np.arange(4), n)
    I = sp.identity(n, format="csr", dtype=np.complex128)
    for k in range(4):
        H = (A - shift[k] * I + psi[k] * I).tocsr()
        inf_r, inner_r, xr = _scipy_gmres(H, X[k], jac)
        assert (int(info[k]), int(inner[k])) == (inf_r, inner_r)
        assert np.linalg.norm(W[k] - xr) <= 1e-6 * np.linalg.norm(xr)


def test_tridiagonal_2_pow_20_round_trip():
    ctx = _ctx()
    n = 1 << 20
    rng = np.random.default_rng(11)
    A = sp.diags([rng.standard_normal(n - 1) + 0j, 4.0 + rng.standard_normal(n) * 0.1 + 1j, rng.standard_normal(n - 1) + 0j],
                 [-1, 0, 1], format="csr")
    perm, kl, ku = _bind(ctx, A, 2)
    assert (kl, ku) == (1, 1)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.set_rhs(b)
    st = ctx.band_solve([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 1)
    assert st[0] == 0
    x = ctx.pop_get(_cabi.POP_W, [0], n)[0]
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)
    info, inner, status = ctx.gmres([1], np.zeros(1, dtype=np.complex128), np.zeros(1), 1, np.zeros(1, dtype=np.int32))
    assert info[0] == 0 and status[0] == 0
    xg = ctx.pop_get(_cabi.POP_W, [1], n)[0]
    assert np.linalg.norm(A @ xg - b) <= 1e-7 * np.linalg.norm(b)


def test_gmres_2_pow_20_runs_large_batches_in_chunks():
    """At n = 2^20 a candidate's GMRES scratch is 386 MB: 60 candidates run in chunks (1/16 of HBM each); every W row is
    bit-identical to the same candidate's lone run."""
    ctx = _ctx()
    n, P = 1 << 20, 60
    rng = np.random.default_rng(14)
    A = sp.diags([rng.standard_normal(n - 1) + 0j, 4.0 + 1j + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1) + 0j],
                 [-1, 0, 1], format="csr")
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(P)
    ctx.pop_put(_cabi.POP_X, np.arange(P), rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n)))
    shift = 0.5 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-20)
    jac = np.zeros(P, dtype=np.int32)
    info, inner, status = ctx.gmres(np.arange(P), shift, psi, 0, jac)
    assert (status == 0).all() and (info == 0).sum() >= P // 2
    probe = [0, 47, 59]
    Wb = ctx.pop_get(_cabi.POP_W, probe, n)
    for i, s in enumerate(probe):
        info1, inner1, _ = ctx.gmres([s], shift[[s]], psi[[s]], 0, jac[[s]])
        assert (info1[0], inner1[0]) == (info[s], inner[s])
        assert np.array_equal(ctx.pop_get(_cabi.POP_W, [s], n)[0].view(np.float64), Wb[i].view(np.float64))


def _strip(m, seed):
    """5-point operator on an m x 4096 strip plus 2 I (well conditioned), complex values, shuffled: n = 4096 m."""
    rng = np.random.default_rng(seed)
    L = (sp.kron(sp.identity(m), sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(4096, 4096)))
         + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(4096))).tocsr().astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    L = (L + 2.0 * sp.identity(L.shape[0])).tocsr()
    p = rng.permutation(L.shape[0])
    return L[p][:, p].tocsr()


def _loop_bodies(A, b, engine, compat, iters=2):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}                 # Fragile: GMRES preferred (scipy-legacy: every solve direct)
    kw = {"engine": engine} if engine is not None else {"gmres_compat": compat}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=6, quiet=True,
                    sparse_mode="device", diag_info=diag, **kw)
    rows = []
    for it in range(iters):
        s.loop_body(it + 1)
        rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                     np.random.get_state()[2], np.random.get_state()[1].copy()))
    return s, rows


@pytest.mark.parametrize("compat", ["scipy-legacy", "rtol"])
def test_solver_loop_bodies_65536_against_host(compat):
    """MAUS_Solver on a sparse linear system at n = 65536 through a real DeviceEngine (band solves or GMRES with its band
    fallback, CSR products), against the same loop bodies on FakeBandContext (SciPy's zgbtrf / zgbtrs and gmres)."""
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from test_band_host import FakeBandContext
    A = _strip(16, 12)
    n = A.shape[0]
    assert n == 65536
    rng = np.random.default_rng(13)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    host_ctx = FakeBandContext()
    ref_s, ref = _loop_bodies(A, b, DeviceEngine(ctx=host_ctx, gmres_compat=compat, sparse_mode="device"), compat)
    s, got = _loop_bodies(A, b, None, compat)
    assert s.engine._band
    if compat == "scipy-legacy":
        assert host_ctx.calls["band"] > 0
    for (r_rows, r_pos, r_key), (g_rows, g_pos, g_key) in zip(ref, got):
        assert r_rows == g_rows
        assert r_pos == g_pos and np.array_equal(r_key, g_key)
    checked = 0
    for c, cr in zip(s.candidates, ref_s.candidates):
        if np.isfinite(c.residual_k):
            r = np.linalg.norm(A @ c.x_k - b)
            assert abs(r - c.residual_k) <= 1e-8 * r + 1e-12 * np.linalg.norm(b)
            assert abs(c.residual_k - cr.residual_k) <= 1e-6 * max(cr.residual_k, 1e-10 * np.linalg.norm(b))
            checked += 1
    assert checked > 0


def test_band_solve_rejects_bad_rhs_mode_and_scans_only_the_matrix():
    ctx = _ctx()
    A = _five_point(8)
    _bind(ctx, A, 1)
    with pytest.raises(_cabi.MausHipError, match="rhs_mode"):
        ctx.band_solve([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 2)
    M, ab, b = _band_case(30, 3, 4, 5)
    ab[3, 0] = np.nan                                   # row kl of column 0 lies above the matrix: zgbtrf never reads it
    x, ipiv, st = ctx.band_lu(ab[None], b[None], 3, 4)
    assert st[0] == 0
    assert np.linalg.norm(M @ x[0] - b) <= 1e-12 * np.linalg.cond(M) * np.linalg.norm(b)
