"""The blocked band LU (sparse_direct="blocked", maus_band_set_method(ctx, 1), csrc/band.hip) on the device: against LAPACK,
against the column kernel of the same context, and through the engine and the solvers."""
import os

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order
from test_gpu_band import _band_case, _bind, _ctx, _five_point, _loop_bodies, _strip

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED


def _blocked_ctx():
    ctx = _ctx()
    ctx.band_set_method(BLOCKED)
    return ctx


def _expected_kernel(kl):
    """The rule of csrc/band.hip: blocked from kl = 16 to kl = 1024, nb = 16 while kl + 16 rows fit the panel at
    two rows per thread (kl <= 1008) and 8 above; the column kernel otherwise."""
    if kl < 16 or kl > 1024:
        return COLUMN, 1
    return BLOCKED, 16 if kl + 16 <= 1024 else 8


# the ten cases of test_band_lu_matches_zgbtrf, then kl above, at and below nb, n not a multiple of nb, n < nb,
# kl + ku + 1 > n, the tallest panel, singular columns at block edges
LU_CASES = [
    (60, 3, 2, ()), (40, 0, 4, ()), (40, 4, 0, ()), (300, 70, 5, ()), (5, 3, 4, ()), (777, 129, 33, ()),
    (200, 1, 1, ()), (90, 5, 7, (17,)), (120, 8, 3, (0, 50)), (1, 0, 0, ()),
    (500, 32, 32, ()), (500, 16, 40, ()), (500, 31, 9, ()), (515, 33, 17, ()), (50, 20, 30, ()), (20, 40, 3, ()),
    (2000, 300, 280, ()), (2000, 513, 64, ()), (3000, 64, 513, ()), (2500, 1024, 900, ()), (1500, 1024, 1024, ()),
    (400, 48, 20, (31, 32, 63, 64)),
]


@pytest.mark.parametrize("n,kl,ku,zero_cols", LU_CASES)
def test_blocked_band_lu_matches_zgbtrf(n, kl, ku, zero_cols):
    ctx = _ctx()
    A, ab, b = _band_case(n, kl, ku, 7 + n + kl, zero_cols)
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)               # the default method
    ctx.band_set_method(BLOCKED)
    assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    ctx.band_set_method(COLUMN)
    x, ipiv, st = ctx.band_lu(ab[None], b[None], kl, ku, method=BLOCKED)
    assert ctx.band_method() == COLUMN                                  # method= holds for the one call
    assert np.array_equal(ipiv[0], piv), (ipiv[0][:20], piv[:20])
    assert st[0] == info
    if info == 0:
        xr, _ = lapack.zgbtrs(lu, kl, ku, b, piv)
        cond = np.linalg.cond(A)
        err = np.linalg.norm(x[0] - xr) / np.linalg.norm(xr)
        print(f"n={n} kl={kl} ku={ku}: cond {cond:.3g}, |x - xr| / |xr| = {err:.3g}")
        assert err <= 1e-12 * cond


def test_blocked_band_lu_batch_and_non_finite_input():
    ctx = _blocked_ctx()
    kl, ku = 24, 19
    assert ctx.band_kernel_for(200, kl, ku) == (BLOCKED, 16)
    cases = [_band_case(200, kl, ku, s) for s in range(5)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[2, kl + ku, 100] = np.nan
    x, ipiv, st = ctx.band_lu(ab, b, kl, ku)
    assert st[2] == -1
    for k in (0, 1, 3, 4):
        assert st[k] == 0
        assert np.linalg.norm(cases[k][0] @ x[k] - b[k]) <= 1e-11 * np.linalg.norm(b[k]) * np.linalg.cond(cases[k][0])


def test_blocked_band_rows_do_not_depend_on_the_batch():
    ctx = _blocked_ctx()
    n, P = 4096, 256
    A = _five_point(64, 1)
    perm, kl, ku = _bind(ctx, A, P)
    assert ctx.band_kernel_for(n, kl, ku)[0] == BLOCKED
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
        c2 = _blocked_ctx()
        _bind(c2, A, P)
        c2.pop_put(_cabi.POP_X, np.arange(P), X)
        assert c2.band_reserve(P) == 40
        chunked = run(c2, np.arange(P))
        assert c2.band_workspace_allocations() == 1
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert np.array_equal(alone.view(np.float64), chunked.view(np.float64))
    st = ctx.band_solve([5], np.array([np.nan + 0j]), np.zeros(1), 0)
    assert st[0] == -1


def test_blocked_against_the_column_kernel_4096_and_profile_class():
    ctx = _ctx()
    n, P = 4096, 64
    A = _five_point(64, 5)
    perm, kl, ku = _bind(ctx, A, P)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    psi = np.full(P, 1e-20)
    slots = np.arange(P)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    Wc = ctx.pop_get(_cabi.POP_W, slots, n)
    ctx.band_set_method(BLOCKED)                                        # the bound ordering stays; the workspace follows
    assert ctx.band_kernel_for(n, kl, ku)[0] == BLOCKED
    ctx.profile_enable(True)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert prof["band_blocked"]["launches"] > 0 and prof["band"]["launches"] == 0
    assert prof["band_blocked"]["flops"] > 0 and prof["band_blocked"]["bytes"] > 0
    Wb = ctx.pop_get(_cabi.POP_W, slots, n)
    for k in range(P):
        assert np.linalg.norm(Wb[k] - Wc[k]) <= 1e-10 * np.linalg.norm(Wc[k])


def test_blocked_against_spsolve_65536():
    ctx = _blocked_ctx()
    m = 256
    n = m * m
    A = _five_point(m, 2)
    perm, kl, ku = _bind(ctx, A, 4)
    assert kl <= 300 and ku <= 300
    assert ctx.band_kernel_for(n, kl, ku) == (BLOCKED, 16)
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


def test_blocked_mode_tridiagonal_2_pow_20_runs_the_column_kernel():
    ctx = _blocked_ctx()
    n = 1 << 20
    rng = np.random.default_rng(11)
    A = sp.diags([rng.standard_normal(n - 1) + 0j, 4.0 + rng.standard_normal(n) * 0.1 + 1j, rng.standard_normal(n - 1) + 0j],
                 [-1, 0, 1], format="csr")
    perm, kl, ku = _bind(ctx, A, 2)
    assert (kl, ku) == (1, 1)
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)                # the narrow-band rule
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.set_rhs(b)
    ctx.profile_enable(True)
    st = ctx.band_solve([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 1)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert st[0] == 0
    assert prof["band"]["launches"] > 0 and prof["band_blocked"]["launches"] == 0
    x = ctx.pop_get(_cabi.POP_W, [0], n)[0]
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(b)


def test_blocked_five_point_262144():
    """One lone solve at the size where the column kernel needs 25 s (profiles/band_rates.txt)."""
    ctx = _blocked_ctx()
    m = 512
    n = m * m
    A = _five_point(m, 15)
    perm, kl, ku = _bind(ctx, A, 1)
    assert 400 <= kl <= 600
    assert ctx.band_kernel_for(n, kl, ku) == (BLOCKED, 16)
    rng = np.random.default_rng(16)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.set_rhs(b)
    shift = np.array([0.5 + 0.1j])
    st = ctx.band_solve([0], shift, np.zeros(1), 1)
    assert st[0] == 0
    x = ctx.pop_get(_cabi.POP_W, [0], n)[0]
    H = A - shift[0] * sp.identity(n, format="csr", dtype=np.complex128)
    assert np.linalg.norm(H @ x - b) <= 1e-10 * np.linalg.norm(b)


def test_blocked_solver_loop_bodies_65536_against_host():
    """test_solver_loop_bodies_65536_against_host with sparse_direct='blocked' and every solve a band solve."""
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from test_band_host import FakeBandContext
    compat = "scipy-legacy"
    A = _strip(16, 12)
    n = A.shape[0]
    assert n == 65536
    rng = np.random.default_rng(13)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    host_ctx = FakeBandContext()
    ref_s, ref = _loop_bodies(A, b, DeviceEngine(ctx=host_ctx, gmres_compat=compat, sparse_mode="device"), compat)
    eng = DeviceEngine(gmres_compat=compat, sparse_mode="device", sparse_direct="blocked")
    s, got = _loop_bodies(A, b, eng, compat)
    assert s.engine is eng and eng._band and eng.ctx.band_method() == BLOCKED
    perm, kl, ku = eng.band_shape(A)
    assert eng.ctx.band_kernel_for(n, kl, ku)[0] == BLOCKED
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


def test_inverse_iterate_solver_blocked_against_spsolve():
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    _ctx()
    A = (_five_point(64, 17) + 2.0 * sp.identity(4096)).tocsr()
    n = A.shape[0]
    rng = np.random.default_rng(18)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    solver = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="blocked")
    x, tries = solver.solve(A, b, 0)
    assert tries == 0
    ctx = InverseIterateSolver._ctx()
    assert ctx.band_method() == BLOCKED
    perm, kl, ku = band_order(A)
    assert ctx.band_kernel_for(n, kl, ku)[0] == BLOCKED
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
    # the next solver on the shared context asks for the column kernel again
    InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="band").solve(A, b, 0)
    assert ctx.band_method() == COLUMN
