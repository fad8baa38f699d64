"""The direct LU path and both GMRES modes above n = 8192 (up to maus_lu_max_n() = 16384).

Above 8192 rows the base panel is the tall 32-rows-per-thread variant, the back substitution always runs in blocks of 256
rows (a short top block when npad is not a multiple of 256) and GMRES takes the 512-thread post-kernel.  Host-side checks
are O(n^2) per check, except one LAPACK factorisation at n = 9000.
"""
import random

import numpy as np
import pytest

import scenarios
from oracle import maus_oracle as orc

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


@pytest.fixture(autouse=True, scope="module")
def _blas_threads():
    """A GPU box hands one GPU's share of cores (16) to the job."""
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        yield
        return
    with threadpool_limits(limits=16):
        yield


def _ginibre_batch(n, count, seed):
    rng = np.random.default_rng(seed)
    A = np.empty((count, n, n), dtype=np.complex128)
    for g in range(count):
        A[g].real = rng.standard_normal((n, n))
        A[g].imag = rng.standard_normal((n, n))
        A[g] *= 1.0 / np.sqrt(n)
    b = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    return A, b


def _zgetf2_pivots(panel):
    """Unblocked LAPACK zgetf2 on an n x k panel: pivot = max |re| + |im|, first index wins."""
    P = panel.copy()
    piv = []
    for c in range(P.shape[1]):
        p = c + int(np.argmax(np.abs(P[c:, c].real) + np.abs(P[c:, c].imag)))
        piv.append(p)
        P[[c, p]] = P[[p, c]]
        P[c + 1:, c] /= P[c, c]
        P[c + 1:, c + 1:] -= np.outer(P[c + 1:, c], P[c, c + 1:])
    return np.array(piv)


def test_lu_9000_same_pivots_as_lapack():
    """npad = 9024: panels above 8192 rows (the tall panel), and a back substitution whose top block is 64 rows."""
    import scipy.linalg as sla
    from adaptive_matrix_solver_amd import Context
    n = 9000
    A, b = _ginibre_batch(n, 1, 9000)
    ctx = Context(0)
    try:
        x, status, ipiv = ctx.lu_solve(A, b, want_ipiv=True)
    finally:
        ctx.close()
    assert status[0] == 0
    lu, piv = sla.lu_factor(A[0])
    assert np.array_equal(ipiv[0], piv)
    ref = sla.lu_solve((lu, piv), b[0])
    del lu
    r_dev = np.linalg.norm(A[0] @ x[0] - b[0])
    r_ref = np.linalg.norm(A[0] @ ref - b[0])
    floor = EPS * np.linalg.norm(A[0], 1) * np.linalg.norm(ref)
    assert r_dev <= 10.0 * max(r_ref, floor), (r_dev, r_ref, floor)


def test_lu_9000_status_codes():
    """One call, three matrices: an exact zero column (LAPACK info = its 1-based index), a NaN entry (-1), a regular one."""
    from adaptive_matrix_solver_amd import Context
    n = 9000
    A, b = _ginibre_batch(n, 3, 77)
    A[0][:, 7] = 0.0
    A[1][1234, 4321] = np.nan
    ctx = Context(0)
    try:
        x, status = ctx.lu_solve(A, b)
    finally:
        ctx.close()
    assert status[0] == 8, status
    assert status[1] == -1, status
    assert status[2] == 0, status
    r = np.linalg.norm(A[2] @ x[2] - b[2])
    assert r <= EPS * np.abs(A[2]).sum(axis=0).max() * np.linalg.norm(x[2]) * n, r


def test_lu_9000_bits_do_not_depend_on_the_batch(monkeypatch):
    """A candidate's solution is the same bits alone, inside a batch of 40 and with MAUS_LU_STREAMS=2 (above 8192 no kernel
    choice depends on the batch); a reservation at n = 16384 asks for what it needs, not for 32 solves."""
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import PERT_NONE
    n, G, k = 9000, 40, 17
    A = scenarios.ginibre(n, 9001)
    rng = np.random.default_rng(5)
    V = (rng.standard_normal((G, n)) + 1j * rng.standard_normal((G, n))) / np.sqrt(n)
    lam = (rng.standard_normal(G) + 1j * rng.standard_normal(G)) * 0.5
    psi = np.full(G, 1e-20)
    monkeypatch.delenv("MAUS_LU_STREAMS", raising=False)
    ctx = Context(0)
    try:
        ctx.set_matrix(A)
        ctx.pop_reserve(G)
        sl = list(range(G))
        ctx.pop_put(0, sl, V)
        st = ctx.shifted_lu_solve(sl, lam, psi, 0, PERT_NONE, None)
        assert (st == 0).all(), st
        W_batch = ctx.pop_get(2, sl, n)
        st = ctx.shifted_lu_solve([k], lam[k:k + 1], psi[k:k + 1], 0, PERT_NONE, None)
        assert st[0] == 0
        w_alone = ctx.pop_get(2, [k], n)[0]
        monkeypatch.setenv("MAUS_LU_STREAMS", "2")
        st = ctx.shifted_lu_solve(sl, lam, psi, 0, PERT_NONE, None)
        assert (st == 0).all(), st
        W_streams = ctx.pop_get(2, sl, n)
        monkeypatch.delenv("MAUS_LU_STREAMS")
        assert np.array_equal(W_batch[k], w_alone)
        assert np.array_equal(W_batch, W_streams)
        # the solve itself: (A - lam I + psi I) w = v, by its backward error
        w = W_batch[k]
        r = np.linalg.norm(A @ w + (psi[k] - lam[k]) * w - V[k])
        assert r <= EPS * n * (np.abs(A).sum(axis=0).max() + abs(lam[k])) * np.linalg.norm(w), r
        assert ctx.lu_reserve(16384, 1) <= 4
    finally:
        ctx.close()


def test_lu_16384_round_trip():
    from adaptive_matrix_solver_amd import Context
    n = 16384
    A, b = _ginibre_batch(n, 1, 16384)
    ctx = Context(0)
    try:
        assert ctx.lu_max_n() == 16384
        x, status, ipiv = ctx.lu_solve(A, b, want_ipiv=True)
    finally:
        ctx.close()
    assert status[0] == 0
    piv = ipiv[0]
    assert piv.shape == (n,) and np.all(piv >= np.arange(n)) and np.all(piv < n)
    assert np.array_equal(piv[:32], _zgetf2_pivots(A[0][:, :32]))
    assert np.isfinite(x[0]).all()
    r = np.linalg.norm(A[0] @ x[0] - b[0])
    bound = EPS * np.abs(A[0]).sum(axis=0).max() * np.linalg.norm(x[0]) * n
    assert r <= bound, (r, bound)


def test_lu_above_the_limit_fails_loudly():
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import MausHipError
    ctx = Context(0)
    try:
        with pytest.raises(MausHipError, match="16384"):
            ctx.lu_reserve(16385, 1)
    finally:
        ctx.close()


def test_gmres_12288_shared_matrix_jacobi():
    from adaptive_matrix_solver_amd import Context
    n, P = 12288, 32
    A, b = scenarios.wide_diag_system(n, 12, decades=3.0, offdiag=0.02)
    psi = np.full(P, 1e-19) * (10.0 ** (np.arange(P) % 3))
    ctx = Context(0)
    try:
        ctx.set_matrix(A)
        ctx.set_rhs(b)
        ctx.pop_reserve(P)
        slots = list(range(P))
        ctx.pop_put(0, slots, np.tile(b, (P, 1)))
        assert ctx.jacobi_check(np.zeros(P, dtype=np.complex128), psi).all()
        info, inner, status = ctx.gmres(slots, np.zeros(P, dtype=np.complex128), psi, 1, np.ones(P, dtype=np.int32))
        X = ctx.pop_get(2, slots, n)
    finally:
        ctx.close()
    assert (status == 0).all() and (info == 0).all()
    H0 = A.copy()
    H0[np.diag_indices(n)] += psi[0]
    xr, info_r, inner_r, _ = orc.gmres_restated(H0, b, b, 1.0 / np.diag(H0))
    del H0
    assert info[0] == info_r and inner[0] == inner_r, (info[0], info_r, inner[0], inner_r)
    assert np.linalg.norm(X[0] - xr) <= 1e-9 * np.linalg.norm(xr)
    R = b[None, :] - (X @ A.T + psi[:, None] * X)
    rel = np.linalg.norm(R, axis=1) / np.linalg.norm(b)
    assert (rel <= 1e-8 * (1 + 1e-6)).all(), rel.max()


def test_gmres_12288_dense_mode_device_draws():
    """maus_gmres_pert at n = 12288: H_k materialised in the LU workspace with device-regenerated MT19937 draws; candidate 0's
    H_k rebuilt on the host from the same draws, and its iterate checked by SciPy's stopping rule on the true residual."""
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import PERT_MT19937
    n, P = 12288, 2
    A, b = scenarios.wide_diag_system(n, 13, decades=3.0, offdiag=0.02)
    shift = np.zeros(P, dtype=np.complex128)
    psi = np.array([3e-3, 1e-2])                    # escalated: the random term is far above the rounding of a matvec
    np.random.seed(41)
    st = np.random.get_state()
    ctx = Context(0)
    try:
        ctx.set_matrix(A)
        ctx.set_rhs(b)
        ctx.pop_reserve(P)
        slots = list(range(P))
        ctx.pop_put(0, slots, np.tile(b, (P, 1)))
        info, inner, status, jac = ctx.gmres_pert(slots, shift, psi, 1, np.ones(P, dtype=np.int32), PERT_MT19937,
                                                  (st, 4 * n * n, 0, np.arange(P, dtype=np.int32)))
        X = ctx.pop_get(2, slots, n)
    finally:
        ctx.close()
    assert (status == 0).all() and (info == 0).all() and jac.all(), (status, info, jac)
    assert (inner > 0).all()
    np.random.set_state(st)                         # candidate 0 = the first 4 n^2 words: U1, U2 (AMS:49-50)
    H = A.copy()
    H.real += ((np.random.rand(n, n) - 0.5) * psi[0]) * 0.15
    H.imag += ((np.random.rand(n, n) - 0.5) * psi[0]) * 0.15
    H[np.diag_indices(n)] += psi[0]
    x0 = X[0]
    r = np.linalg.norm(b - H @ x0) / np.linalg.norm(b)
    assert r <= 1e-8 * (1 + 1e-6), r
    del H
    # the random term matters here: against the matrix without it the same iterate fails the test
    r0 = np.linalg.norm(b - (A @ x0 + psi[0] * x0)) / np.linalg.norm(b)
    assert r0 > 1e-8, r0


def test_eig12288_solver_construction_and_loop_body():
    """MAUS_Solver at n = 12288: construction runs the device condition estimate (LU on A and on A^H), then one loop body
    with the bookkeeping and NumPy-stream checks of the n = 4096 test (the stream jump by maus_mt19937_jump)."""
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    from adaptive_matrix_solver_amd._cabi import mt19937_jump
    n, P = 12288, 8
    A = scenarios.ginibre(n, 12288, None)
    np.random.seed(6)
    random.seed(6)
    SolutionCandidate._candidate_id_counter = 0
    solver = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=P, global_convergence_tol=1e-8, quiet=True)
    st0 = np.random.get_state()
    py0 = random.getstate()
    solver._update_global_diagnostics(1)
    solver._adjust_global_strategy(1)
    solver.step_population()
    st1 = np.random.get_state()
    assert random.getstate() == py0
    cands = list(solver.candidates)
    assert [c.id for c in cands] == list(range(P))
    assert all(c.local_psi_retries_needed == 0 and c.num_resets == 0 for c in cands)
    key, pos = mt19937_jump(st0[1], st0[2], 4 * n * n * P)
    assert st1[2] == pos and np.array_equal(st1[1], key)
    for c in cands[:4]:
        v = np.asarray(c.v_k)
        r = np.linalg.norm(A @ v - c.lambda_k * v)
        assert abs(r - c.residual_k) <= 1e-9 * max(r, 1e-12)
        assert abs(np.linalg.norm(v) - 1.0) <= 1e-12
