"""Sparse problem matrices on the device (sparse_mode='device', csrc/spmm.hip).

The CSR SpMM against SciPy and its batch independence, the CSR H build + LU against spsolve, GMRES through the CSR product
against SciPy's GMRES (info and inner-iteration counts), the SVD products, the sparse Hermitian shortcut, malformed CSR input,
rebinding, and whole loop bodies of the HIP path against the same loop bodies on FakeSparseContext (the reference's sparse
SciPy calls on the host)."""
import random

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from test_gpu_step_parity import compare
import sparse_scenarios
from test_sparse_host import FakeSparseContext, _herm, _tridiag

pytestmark = pytest.mark.gpu

POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3


@pytest.fixture(autouse=True, scope="module")
def _blas_threads():
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        yield
        return
    with threadpool_limits(limits=16):
        yield


def _ctx():
    from adaptive_matrix_solver_amd import Context
    return Context(0)


def _laplace2d(m, seed=0):
    """complex 5-point operator on an m x m grid (n = m^2)"""
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    I = sp.identity(m)
    L = sp.kron(I, T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), I)
    rng = np.random.default_rng(seed)
    L = sp.csr_matrix(L, dtype=np.complex128)
    L.data = L.data * (1.0 + 0.1j * rng.standard_normal(L.nnz))
    return L


def _random_pattern(n, per_row, seed=1):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, n * per_row)
    vals = rng.standard_normal(n * per_row) + 1j * rng.standard_normal(n * per_row)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    return A + sp.identity(n, format="csr") * 30.0


def _rows(n, P, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))


def _products(ctx, X, slots, adjoint):
    """A x (POP_Y, via maus_matvec_rayleigh) or A^H x (POP_W, via the SVD residual) for the listed slots."""
    n = X.shape[1]
    ctx.pop_put(POP_U if adjoint else POP_X, slots, X[: len(slots)])
    if adjoint:
        ctx.residual(3, slots, np.zeros(len(slots), dtype=np.complex128))
        return ctx.pop_get(POP_W, slots, n)
    ctx.matvec_rayleigh(slots)
    return ctx.pop_get(POP_Y, slots, n)


@pytest.mark.parametrize("which,sched", [("laplace", "rows"), ("pattern27", "rows"), ("pattern100", "wave")])
def test_spmm_matches_scipy_and_is_batch_independent(which, sched):
    n = 16384
    A = _laplace2d(128) if which == "laplace" else _random_pattern(n, int(which[7:]))
    X = _rows(n, 256, 3)
    ctx = _ctx()
    try:
        ctx.set_matrix_csr(A)
        assert ctx.matrix_is_sparse() == sched
        ctx.pop_reserve(256)
        for adjoint in (False, True):
            M = A.conj().T.tocsr() if adjoint else A
            full = _products(ctx, X, list(range(256)), adjoint)
            want = (M @ X.T).T
            rel = np.linalg.norm(full - want, axis=1) / np.linalg.norm(want, axis=1)
            assert rel.max() <= 1e-14, (adjoint, rel.max())
            one = _products(ctx, X[[5]], [5], adjoint)
            assert np.array_equal(one[0], full[5])
            some = _products(ctx, X[:33], list(range(33)), adjoint)
            assert np.array_equal(some, full[:33])
            perm = np.random.default_rng(9).permutation(256)
            got = _products(ctx, X[perm], perm.tolist(), adjoint)
            assert np.array_equal(got, full[perm])
    finally:
        ctx.close()


def _scipy_gmres_counts(H, b, jac):
    count = [0]
    M = sp.diags(1.0 / H.diagonal(), format="csc") if jac else None
    x, info = spla.gmres(H, b, x0=b, rtol=1e-8, restart=20, maxiter=50, M=M,
                         callback=lambda r: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
    return x, info, count[0]


@pytest.mark.parametrize("jac", [0, 1])
def test_sparse_gmres_16384_matches_scipy(jac):
    n, P = 16384, 64
    A = _laplace2d(128, seed=2)
    b = np.random.default_rng(4).standard_normal(n) + 0j
    psi = 1e-19 * 10.0 ** (np.arange(P) % 4)
    ctx = _ctx()
    try:
        ctx.set_matrix_csr(A)
        ctx.set_rhs(b)
        ctx.pop_reserve(P)
        slots = list(range(P))
        ctx.pop_put(POP_X, slots, np.tile(b, (P, 1)))
        ctx.profile_enable(True)
        info, inner, status = ctx.gmres(slots, np.zeros(P, dtype=np.complex128), psi, 1, np.full(P, jac, dtype=np.int32))
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        X = ctx.pop_get(POP_W, slots, n)
    finally:
        ctx.close()
    assert prof["spmm"]["launches"] > 0 and prof["zgemm"]["launches"] == 0, prof
    assert (status == 0).all()
    for k in (0, 1, 2, 63):
        H = sp.csr_matrix(A + sp.identity(n, dtype=np.complex128, format="csc") * np.complex128(psi[k]))
        xr, info_r, inner_r = _scipy_gmres_counts(H, b, jac)
        assert (info[k], inner[k]) == (info_r, inner_r), (k, info[k], info_r, inner[k], inner_r)
        assert np.linalg.norm(X[k] - xr) <= 1e-8 * np.linalg.norm(xr)


def test_sparse_direct_solve_9000():
    n = 9000
    rng = np.random.default_rng(5)
    A = sp.csr_matrix(sp.diags([rng.standard_normal(n - 1), 4.0 + rng.standard_normal(n) + 1j * rng.standard_normal(n),
                                rng.standard_normal(n - 1)], [-1, 0, 1]) + _random_pattern(n, 3, seed=6) * 0.1)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx = _ctx()
    try:
        ctx.set_matrix_csr(A)
        ctx.set_rhs(b)
        ctx.pop_reserve(2)
        ctx.pop_put(POP_X, [0, 1], np.tile(b, (2, 1)))
        st = ctx.shifted_lu_solve([0, 1], np.zeros(2, dtype=np.complex128), np.array([1e-18, 1e-17]), rhs_mode=1, pert_mode=0)
        X = ctx.pop_get(POP_W, [0, 1], n)
        assert (st == 0).all()
        for k, ps in enumerate((1e-18, 1e-17)):
            H = sp.csc_matrix(A + sp.identity(n, dtype=np.complex128) * ps)
            xr = spla.spsolve(H, b)
            assert np.linalg.norm(H @ X[k] - b) <= 1e-12 * np.linalg.norm(b)
            assert np.linalg.norm(X[k] - xr) <= 1e-10 * np.linalg.norm(xr)
        # a singular H (an empty row and column) has the status of the dense path: info > 0
        S = sp.lil_matrix(A)
        S[17, :] = 0
        S[:, 17] = 0
        ctx.set_matrix_csr(S)
        st = ctx.shifted_lu_solve([0], np.zeros(1, dtype=np.complex128), np.zeros(1), rhs_mode=1, pert_mode=0)
        assert st[0] > 0
    finally:
        ctx.close()


def test_sparse_svd_products_2048x1536():
    m, n, P = 2048, 1536, 64
    A = sp.random(m, n, density=0.01, random_state=np.random.RandomState(7), format="csr", dtype=np.float64)
    A = sp.csr_matrix(A * (1 + 0.5j))
    V = _rows(n, P, 8)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    ctx = _ctx()
    try:
        ctx.set_matrix_csr(A)
        ctx.pop_reserve(P)
        slots = list(range(P))
        ctx.pop_put(POP_X, slots, V)
        norms = ctx.svd_power_propose(slots)
        ctx.svd_commit(slots)
        u = ctx.pop_get(POP_U, slots, m)
        v = ctx.pop_get(POP_X, slots, n)
        sig = np.maximum(norms[:, 1], norms[:, 3])
        res, fin = ctx.residual(3, slots, sig.astype(np.complex128))
    finally:
        ctx.close()
    for k in np.random.default_rng(1).choice(P, 32, replace=False):
        t = A @ V[k]
        s1 = np.linalg.norm(t)
        uu = t / s1
        w = A.conj().T @ uu
        s2 = np.linalg.norm(w)
        assert abs(norms[k, 1] - s1) <= 1e-13 * s1 and abs(norms[k, 3] - s2) <= 1e-13 * s2
        assert np.linalg.norm(u[k] - uu) <= 1e-13 and np.linalg.norm(v[k] - w / s2) <= 1e-13
        s = max(s1, s2)
        r = np.linalg.norm(A @ v[k] - s * u[k]) + np.linalg.norm(A.conj().T @ u[k] - s * v[k])
        assert abs(res[k] - r) <= 1e-12 * max(1.0, r)


def test_malformed_csr_is_rejected():
    from adaptive_matrix_solver_amd._cabi import MausHipError
    ctx = _ctx()
    try:
        ptr, idx, val = np.array([0, 2, 3]), np.array([0, 1, 1]), np.ones(3, dtype=np.complex128)
        ctx.set_matrix_csr_arrays(2, 2, ptr, idx, val)
        assert ctx.matrix_is_sparse() == "rows"
        for p, i, why in [(ptr, np.array([0, 2, 1]), "out of range"), (np.array([0, 4, 3]), idx, "monotone"),
                          (np.array([0, 2, 4]), idx, "nnz"), (ptr, np.array([1, 0, 1]), "increasing")]:
            with pytest.raises(MausHipError, match=why):
                ctx.set_matrix_csr_arrays(2, 2, p, i, val)
        with pytest.raises(MausHipError):
            ctx.set_matrix_csr_arrays(2, 2, ptr, idx, val[:2])
    finally:
        ctx.close()


def test_sparse_dense_sparse_rebinding():
    n, P = 512, 40
    A = sp.csr_matrix(_tridiag(n, seed=11))
    D = np.random.default_rng(12).standard_normal((n, n)) + 0j
    X = _rows(n, P, 13)
    ctx = _ctx()
    try:
        for M in (A, D, A * 2.0, D[:300, :300]):
            ctx.set_matrix_csr(M) if sp.issparse(M) else ctx.set_matrix(M)
            m = M.shape[0]
            ctx.pop_reserve(P)
            got = _products(ctx, X[:, :m], list(range(P)), False)
            want = (M @ X[:, :m].T).T
            assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want)
            assert ctx.matrix_is_sparse() == ("rows" if sp.issparse(M) else None)
    finally:
        ctx.close()


def test_sparse_hermitian_1024():
    import scipy.linalg as sla
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    A = _herm(1024, seed=14)
    np.random.seed(1)
    random.seed(1)
    SolutionCandidate._candidate_id_counter = 0
    s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=32, quiet=True, sparse_mode="device")
    assert s.problem_knowledge["is_hermitian"] and s.engine.ctx.matrix_is_sparse()
    s._update_global_diagnostics(1)
    s._adjust_global_strategy(1)
    s.step_population()
    ev = sla.eigvalsh(A.toarray())
    top = ev[np.argsort(np.abs(ev))[-6:]]
    scale = np.abs(ev).max()
    for c in s.candidates:
        assert c.state.name == "CONVERGED"
        assert np.min(np.abs(top - c.lambda_k)) <= 1e-12 * scale
        r = np.linalg.norm(A @ c.v_k - c.lambda_k * c.v_k)
        assert r <= 1e-10 * scale and abs(c.residual_k - r) <= 1e-12 * scale


# ---- whole loop bodies: HIP path against the reference's sparse SciPy calls on the host ---------------------------------
def _scenario(name):
    """the scenarios of the reference fixtures (tests/golden/sparse_scenarios.py)"""
    from adaptive_matrix_solver_amd.solver import ProblemType as PT
    spec = sparse_scenarios.SPARSE_TRAJECTORIES[name]
    A, b = sparse_scenarios.build(name)
    kind = {"eig": PT.EIGENVALUE, "lin": PT.SOLVE_LINEAR_SYSTEM, "svd": PT.SVD}[spec["kind"]]
    return A, kind, b, spec["P"], spec["tol"]


def _run(name, iters, engine, compat):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    import snapshot
    A, kind, b, P, tol = _scenario(name)
    seed = sparse_scenarios.SPARSE_TRAJECTORIES[name]["seed"]
    np.random.seed(seed)
    random.seed(seed)
    SolutionCandidate._candidate_id_counter = 0
    kw = {"engine": engine} if engine is not None else {"gmres_compat": compat}
    s = MAUS_Solver(A, kind, b_vector=b, initial_num_candidates=P, global_convergence_tol=tol, quiet=True, sparse_mode="device", **kw)
    out = []
    for it in range(iters):
        s._update_global_diagnostics(it + 1)
        s._adjust_global_strategy(it + 1)
        s.step_population()
        rows = []
        for c in s.candidates:
            if kind == ProblemType.EIGENVALUE:
                lam, vecs = c.lambda_k, [c.v_k]
            elif kind == ProblemType.SOLVE_LINEAR_SYSTEM:
                lam, vecs = 0j, [c.x_k]
            else:
                lam, vecs = c.sigma_k, [c.u_k, c.right_v_k]
            rows.append(dict(id=c.id, state=c.state.value, stuck=c.stuck_counter, retries=c.local_psi_retries_needed,
                             resets=c.num_resets, w=float(c.w_k), resid=float(c.residual_k), alpha=complex(c.alpha_local_step),
                             lam=complex(lam if lam is not None else 0j), vecs=[np.array(v) for v in vecs]))
        s._manage_candidates(it + 1)
        out.append(dict(rows=rows, rng=snapshot.rng_digest(), after=[c.id for c in s.candidates], energy=s.landscape_energy,
                        n_distinct=s.num_distinct_converged_solutions, thr=s.strat_params["current_convergence_threshold"],
                        pref=s.problem_knowledge["local_solver_preference"]))
    return out, float(abs(sp.csr_matrix(A)).sum(axis=0).max())


@pytest.mark.parametrize("name,compat", [(n, m) for n, sc in sparse_scenarios.SPARSE_TRAJECTORIES.items() for m in sc["modes"]])
def test_sparse_loop_bodies_match_host(name, compat):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    iters = min(4, sparse_scenarios.SPARSE_TRAJECTORIES[name]["iters"])
    ref, anorm = _run(name, iters, DeviceEngine(ctx=FakeSparseContext(), gmres_compat=compat, sparse_mode="device"), compat)
    got, _ = _run(name, iters, None, compat)
    herm = name.startswith("sp_herm") or name.startswith("sp_real")
    compare(ref, got, anorm, name, tie_tol=1e-12 if herm else None)
