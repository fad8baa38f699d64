"""The row-tiled blocked band LU (sparse_direct="tiled", maus_band_set_method(ctx, 2), csrc/band.hip) on the device: against
LAPACK above the blocked method's kl = 1024, bit for bit against the blocked method below it, against the column kernel of the
same context, and through the engine and the solvers."""
import os

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order
from test_gpu_band import _bind, _ctx, _loop_bodies

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED
TILED = getattr(_cabi, "BAND_TILED", None)               # None without the feature: every test below then fails in its first call


def _expected_kernel(kl):
    """The rule of csrc/band.hip: tiled from kl = 16 to kl = 4096; nb as the blocked method's up to kl = 1024 (16
    up to 1008, then 8); above it 16 while kl + 16 rows fit the panel at three rows per thread (kl <= 1520), 8 while kl + 8 fit
    at six (kl <= 3064) and 4 above."""
    if kl < 16 or kl > 4096:
        return COLUMN, 1
    if kl <= 1024:
        return TILED, 16 if kl <= 1008 else 8
    return TILED, 16 if kl <= 1520 else (8 if kl <= 3064 else 4)


def _wide_case(n, kl, ku, seed, zero_cols=()):
    """A dense complex normal matrix cut to the band, the listed columns zero; `ab` in zgbtrf's layout, diagonal by diagonal."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = np.tril(np.triu(A, -kl), ku)
    for j in zero_cols:
        A[:, j] = 0
    kv = kl + ku
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    for k in range(-min(kl, n - 1), min(ku, n - 1) + 1):  # diagonal k holds A[i, i + k]: row kv - k of ab, columns i + k
        d = np.diagonal(A, k)
        if k >= 0:
            ab[kv - k, k:] = d
        else:
            ab[kv - k, :n + k] = d
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, ab, b


def _same_bits(x, y):
    """Equal as float64 values, element for element; the NaNs of a solve past a zero pivot count as equal to each other."""
    return np.array_equal(np.ascontiguousarray(x).view(np.float64), np.ascontiguousarray(y).view(np.float64), equal_nan=True)


# the first band above the blocked method's limit, n < kl, ku > kl, a tall band, above the nb = 8 panel, the cap (full-height
# slices for the first block steps), n no multiple of any nb, singular columns at block edges
WIDE_CASES = [
    (1400, 1025, 600, ()), (1200, 1500, 200, ()), (2600, 1025, 1030, ()), (2600, 2048, 300, ()), (3300, 3072, 800, ()),
    (4160, 4096, 1000, ()), (2307, 1100, 500, ()), (2300, 1100, 500, (7, 8, 1023, 1024)),
]


@pytest.mark.parametrize("n,kl,ku,zero_cols", WIDE_CASES)
def test_tiled_band_lu_matches_zgbtrf_above_1024(n, kl, ku, zero_cols):
    ctx = _ctx()
    A, ab, b = _wide_case(n, kl, ku, 7 + n + kl, zero_cols)
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)
    if zero_cols:
        assert info == 8
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)               # the default method
    ctx.band_set_method(BLOCKED)
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)               # too tall for the blocked method
    ctx.band_set_method(TILED)
    assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == TILED
    ctx.band_set_method(COLUMN)
    x, ipiv, st = ctx.band_lu(ab[None], b[None], kl, ku, method=TILED)
    assert ctx.band_method() == COLUMN                                  # method= holds for the one call
    assert np.array_equal(ipiv[0], piv), (np.flatnonzero(ipiv[0] != piv)[:10], n)
    assert st[0] == info
    if info == 0:
        xr, _ = lapack.zgbtrs(lu, kl, ku, b, piv)
        cond = np.linalg.cond(A, 1)
        err = np.linalg.norm(x[0] - xr) / np.linalg.norm(xr)
        print(f"n={n} kl={kl} ku={ku}: cond_1 {cond:.3g}, |x - xr| / |xr| = {err:.3g}")
        assert err <= 1e-12 * cond


# every shape class of the blocked method's own cases: kl at and next to nb, n no multiple of nb, n < nb + kl, kl > n, the
# nb = 8 panel, the tallest band both methods take, singular columns at block edges
BITS_CASES = [
    (500, 32, 32, ()), (500, 16, 40, ()), (515, 33, 17, ()), (50, 20, 30, ()), (20, 40, 3, ()), (2000, 513, 64, ()),
    (2500, 1024, 900, ()), (1500, 1024, 1024, ()), (400, 48, 20, (31, 32, 63, 64)),
]


@pytest.mark.parametrize("n,kl,ku,zero_cols", BITS_CASES)
def test_tiled_gives_the_bits_of_blocked_up_to_1024(n, kl, ku, zero_cols):
    ctx = _ctx()
    A, ab, b = _wide_case(n, kl, ku, 7 + n + kl, zero_cols)
    ctx.band_set_method(BLOCKED)
    assert ctx.band_kernel_for(n, kl, ku)[0] == BLOCKED
    ctx.band_set_method(TILED)
    assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == TILED
    xb, pb, sb = ctx.band_lu(ab[None], b[None], kl, ku, method=BLOCKED)
    xt, pt, st_ = ctx.band_lu(ab[None], b[None], kl, ku, method=TILED)
    assert np.array_equal(pt, pb), np.flatnonzero(pt[0] != pb[0])[:10]
    assert np.array_equal(st_, sb)
    if zero_cols:
        assert sb[0] > 0
    else:
        assert sb[0] == 0 and np.isfinite(xb).all()
    assert _same_bits(xt, xb), np.flatnonzero(xt[0] != xb[0])[:10]


def test_tiled_gives_the_status_of_blocked_on_non_finite_input():
    ctx = _ctx()
    kl, ku = 24, 19
    cases = [_wide_case(200, kl, ku, s) for s in range(5)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[2, kl + ku, 100] = np.nan
    xb, pb, sb = ctx.band_lu(ab, b, kl, ku, method=BLOCKED)
    xt, pt, st_ = ctx.band_lu(ab, b, kl, ku, method=TILED)
    assert st_[2] == -1 and np.array_equal(st_, sb)
    assert np.array_equal(pt, pb)
    keep = [0, 1, 3, 4]
    assert (st_[keep] == 0).all()
    assert np.isfinite(xt[keep]).all() and _same_bits(xt, xb)


def test_tiled_rule():
    ctx = _ctx()
    ctx.band_set_method(TILED)
    assert ctx.band_method() == TILED
    assert ctx.band_kernel_for(4096, 15, 40) == (COLUMN, 1)
    assert ctx.band_kernel_for(6000, 4097, 10) == (COLUMN, 1)
    assert ctx.band_kernel_for(4096, 16, 5) == (TILED, 16)
    assert ctx.band_kernel_for(3000, 1016, 5) == (TILED, 8)
    assert ctx.band_kernel_for(3000, 1008, 5) == (TILED, 16)
    assert ctx.band_kernel_for(3000, 1025, 5) == (TILED, 16)
    assert ctx.band_kernel_for(3000, 1520, 5) == (TILED, 16)
    assert ctx.band_kernel_for(3000, 1521, 5) == (TILED, 8)
    assert ctx.band_kernel_for(5000, 3064, 5) == (TILED, 8)
    assert ctx.band_kernel_for(5000, 3065, 5) == (TILED, 4)
    assert ctx.band_kernel_for(6000, 4096, 10) == (TILED, 4)
    with pytest.raises(_cabi.MausHipError):
        ctx.band_set_method(3)
    assert ctx.band_method() == TILED


_WIDE = {}


def _wide_operator():
    """n = 2400, four random entries per row in [-0.5, 0.5) with complex scaling, plus 0.5 I: small enough a diagonal that the
    factorisation pivots.  The ordering leaves kl ~ 1490: a band only the tiled method takes.  Built once, never changed."""
    if not _WIDE:
        n = 2400
        A = sp.random(n, n, density=4 / n, random_state=np.random.default_rng(1), format="csr").astype(np.complex128)
        rng = np.random.default_rng(101)
        A.data = (A.data - 0.5) * (1.0 + 0.3j * rng.standard_normal(A.nnz))
        A = (A + 0.5 * sp.identity(n)).tocsr()
        perm, kl, ku = band_order(A)
        _WIDE.update(A=A, kl=kl, ku=ku, cond=np.linalg.cond(A.toarray()),
                     b=rng.standard_normal(n) + 1j * rng.standard_normal(n))
    assert _WIDE["kl"] > 1024 and _WIDE["cond"] < 1e6
    return _WIDE["A"], _WIDE["b"]


def _tiled_ctx():
    ctx = _ctx()
    ctx.band_set_method(TILED)
    return ctx


def test_tiled_rows_do_not_depend_on_the_batch_on_a_wide_band():
    ctx = _tiled_ctx()
    A, _ = _wide_operator()
    n, P = A.shape[0], 33
    perm, kl, ku = _bind(ctx, A, P)
    assert kl > 1024 and ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == TILED
    rng = np.random.default_rng(3)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = 0.1 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3)
    probe = [0, 17, 32]

    def run(c, slots):
        st = c.band_solve(slots, shift[slots], psi[slots], 0)
        assert (st == 0).all()
        return c.pop_get(_cabi.POP_W, probe, n)

    alone = np.stack([run(ctx, np.array([s]))[i] for i, s in enumerate(probe)])
    full = run(ctx, np.arange(P))
    assert _same_bits(alone, full)
    k = 17                                                              # the solve is a solve: one row against its system
    H = A - (shift[k] - psi[k]) * sp.identity(n, format="csr", dtype=np.complex128)
    assert np.linalg.norm(H @ alone[1] - X[k]) <= 1e-10 * np.linalg.norm(X[k])
    os.environ["MAUS_BAND_BATCH"] = "8"
    try:
        c2 = _tiled_ctx()
        _bind(c2, A, P)
        c2.pop_put(_cabi.POP_X, np.arange(P), X)
        assert c2.band_reserve(P) == 8
        chunked = run(c2, np.arange(P))
        assert c2.band_workspace_allocations() == 1
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert _same_bits(alone, chunked)
    st = ctx.band_solve([5], np.array([np.nan + 0j]), np.zeros(1), 0)
    assert st[0] == -1


def test_tiled_against_the_column_kernel_and_profile_class():
    ctx = _ctx()
    A, _ = _wide_operator()
    n, P = A.shape[0], 8
    perm, kl, ku = _bind(ctx, A, P)
    rng = np.random.default_rng(6)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = 0.1 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-20)
    slots = np.arange(P)
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    Wc = ctx.pop_get(_cabi.POP_W, slots, n)
    ctx.band_set_method(TILED)                                          # the bound ordering stays; the workspace follows
    assert ctx.band_kernel_for(n, kl, ku)[0] == TILED
    ctx.profile_enable(True)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert prof["band_tiled"]["launches"] > 0 and prof["band"]["launches"] == 0 and prof["band_blocked"]["launches"] == 0
    assert prof["band_tiled"]["flops"] > 0 and prof["band_tiled"]["bytes"] > 0
    Wt = ctx.pop_get(_cabi.POP_W, slots, n)
    for k in range(P):
        assert np.linalg.norm(Wt[k] - Wc[k]) <= 1e-10 * np.linalg.norm(Wc[k])


def _seven_point(m, seed):
    """3-D 7-point operator on an m x m x m grid with complex values, shuffled so that the ordering has work to do."""
    rng = np.random.default_rng(seed)
    I = sp.identity(m)
    T = sp.diags([-1.0, 6.0, -1.0], [-1, 0, 1], shape=(m, m))
    O = sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m))
    L = (sp.kron(I, sp.kron(I, T)) + sp.kron(I, sp.kron(O, I)) + sp.kron(O, sp.kron(I, I))).tocsr().astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    p = rng.permutation(m ** 3)
    return L[p][:, p].tocsr()


def test_tiled_seven_point_40_cubed():
    """One lone solve at the size the mode exists for: a 3-D grid whose band is too tall for the blocked method."""
    ctx = _tiled_ctx()
    A = _seven_point(40, 15)
    n = A.shape[0]
    assert n == 64000
    perm, kl, ku = _bind(ctx, A, 1)
    assert 1025 <= kl <= 1500
    assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == TILED
    rng = np.random.default_rng(16)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.set_rhs(b)
    shift = np.array([0.5 + 0.1j])
    st = ctx.band_solve([0], shift, np.zeros(1), 1)
    assert st[0] == 0
    x = ctx.pop_get(_cabi.POP_W, [0], n)[0]
    H = A - shift[0] * sp.identity(n, format="csr", dtype=np.complex128)
    assert np.linalg.norm(H @ x - b) <= 1e-10 * np.linalg.norm(b)


def test_tiled_solver_loop_bodies_against_host():
    """test_blocked_solver_loop_bodies_65536_against_host on the n = 2400 wide-band operator with sparse_direct='tiled'."""
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from test_band_host import FakeBandContext
    compat = "scipy-legacy"
    A, b = _wide_operator()
    n = A.shape[0]
    host_ctx = FakeBandContext()
    ref_s, ref = _loop_bodies(A, b, DeviceEngine(ctx=host_ctx, gmres_compat=compat, sparse_mode="device", sparse_direct="band"),
                              compat)
    eng = DeviceEngine(gmres_compat=compat, sparse_mode="device", sparse_direct="tiled")
    s, got = _loop_bodies(A, b, eng, compat)
    assert s.engine is eng and eng._band and eng.ctx.band_method() == TILED
    perm, kl, ku = eng.band_shape(A)
    assert kl > 1024 and eng.ctx.band_kernel_for(n, kl, ku)[0] == TILED
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


def test_inverse_iterate_solver_tiled_against_spsolve():
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    _ctx()
    A, b = _wide_operator()
    n = A.shape[0]
    solver = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="tiled")
    x, tries = solver.solve(A, b, 0)
    assert tries == 0
    ctx = InverseIterateSolver._ctx()
    assert ctx.band_method() == TILED
    perm, kl, ku = band_order(A)
    assert kl > 1024 and ctx.band_kernel_for(n, kl, ku)[0] == TILED
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
    # the next solver on the shared context asks for the column kernel again
    InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="band").solve(A, b, 0)
    assert ctx.band_method() == COLUMN
