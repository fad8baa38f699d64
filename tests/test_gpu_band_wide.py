"""The two-level band LU with the MFMA trailing update (sparse_direct="wide", maus_band_set_method(ctx, 4), csrc/band.hip) on
the device: against LAPACK, exactly on a case whose every intermediate is representable, against the tiled method, and through
the engine and the solvers."""
import os

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order, runs_wide
from test_gpu_band import _bind, _ctx, _five_point, _loop_bodies
from test_gpu_band_tiled import _same_bits, _wide_case, _wide_operator

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED, TILED = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED
WIDE = getattr(_cabi, "BAND_WIDE", None)                 # None without the feature: every test below then fails in its first call


def _expected_kernel(kl):
    """The rule of csrc/band.hip under method 4: wide from kl = 64 to kl = 4096 with the tiled method's inner
    nb, exactly the tiled method from kl = 16 to 63, the column kernel elsewhere."""
    if kl < 16 or kl > 4096:
        return COLUMN, 1
    if kl <= 1024:
        nb = 16 if kl <= 1008 else 8
    else:
        nb = 16 if kl <= 1520 else (8 if kl <= 3064 else 4)
    return (WIDE if kl >= 64 else TILED), nb


# the smallest band that runs wide; ku > kl and n no multiple of 64 or 16; one full outer block with kl + ku + 1 close to n;
# n < NBO (inner steps only); singular columns at inner and outer block edges; inner nb = 16, 8 and 4
LAPACK_CASES = [
    (300, 64, 20, ()), (333, 65, 130, ()), (100, 70, 10, ()), (60, 64, 5, ()), (400, 100, 40, (15, 16, 63, 64, 127, 128)),
    (1400, 1025, 600, ()), (2600, 2048, 300, ()), (3300, 3072, 800, ()), (4160, 4096, 1000, ()),
]
_CASES = {}


def _case(n, kl, ku, zero_cols):
    """System, LAPACK's factorisation and solution, cond_1 -- built once per shape, never changed."""
    key = (n, kl, ku, zero_cols)
    if key not in _CASES:
        A, ab, b = _wide_case(n, kl, ku, 7 + n + kl, zero_cols)
        lu, piv, info = lapack.zgbtrf(ab, kl, ku)
        xr = lapack.zgbtrs(lu, kl, ku, b, piv)[0] if info == 0 else None
        cond = np.linalg.cond(A, 1) if info == 0 else np.inf
        _CASES[key] = dict(ab=ab, b=b, piv=piv, info=info, xr=xr, cond=cond, got={})
    return _CASES[key]


def _solved(ctx, case, kl, ku, method):
    """(x, ipiv, status) of `case` under `method`, one device solve per method and case."""
    if method not in case["got"]:
        case["got"][method] = ctx.band_lu(case["ab"][None], case["b"][None], kl, ku, method=method)
    return case["got"][method]


@pytest.mark.parametrize("n,kl,ku,zero_cols", LAPACK_CASES)
def test_wide_band_lu_matches_zgbtrf(n, kl, ku, zero_cols):
    ctx = _ctx()
    case = _case(n, kl, ku, zero_cols)
    if zero_cols:
        assert case["info"] == 16
    ctx.band_set_method(WIDE)
    assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == WIDE and ctx.band_outer_nb(n, kl, ku) == 64
    ctx.band_set_method(COLUMN)
    x, ipiv, st = _solved(ctx, case, kl, ku, WIDE)
    assert ctx.band_method() == COLUMN                                  # method= holds for the one call
    assert np.array_equal(ipiv[0], case["piv"]), (np.flatnonzero(ipiv[0] != case["piv"])[:10], n)
    assert st[0] == case["info"]
    if case["info"] == 0:
        xr = case["xr"]
        err = np.linalg.norm(x[0] - xr) / np.linalg.norm(xr)
        print(f"n={n} kl={kl} ku={ku}: cond_1 {case['cond']:.3g}, |x - xr| / |xr| = {err:.3g}")
        assert err <= 1e-12 * case["cond"]


@pytest.mark.parametrize("n,kl,ku,zero_cols", LAPACK_CASES)
def test_wide_against_tiled(n, kl, ku, zero_cols):
    """Same pivots and status as the tiled method; x within the zgbtrs contract of tiled's x where the factorisation went
    through (past an exact zero pivot neither solution means anything)."""
    ctx = _ctx()
    case = _case(n, kl, ku, zero_cols)
    xw, pw, sw = _solved(ctx, case, kl, ku, WIDE)
    xt, pt, st_ = _solved(ctx, case, kl, ku, TILED)
    assert np.array_equal(pw, pt), np.flatnonzero(pw[0] != pt[0])[:10]
    assert np.array_equal(sw, st_)
    if st_[0] == 0:
        err = np.linalg.norm(xw[0] - xt[0]) / np.linalg.norm(xt[0])
        print(f"n={n} kl={kl} ku={ku}: |x_wide - x_tiled| / |x_tiled| = {err:.3g}")
        assert err <= 1e-12 * case["cond"]
    else:
        assert zero_cols and st_[0] == 16


@pytest.mark.parametrize("n,kl,ku", [(500, 32, 32), (515, 33, 17)])
def test_wide_gives_the_bits_of_tiled_below_64(n, kl, ku):
    ctx = _ctx()
    ctx.band_set_method(WIDE)
    assert ctx.band_kernel_for(n, kl, ku) == (TILED, 16) and ctx.band_outer_nb(n, kl, ku) == 0
    ctx.band_set_method(COLUMN)
    A, ab, b = _wide_case(n, kl, ku, 7 + n + kl)
    xt, pt, st_ = ctx.band_lu(ab[None], b[None], kl, ku, method=TILED)
    xw, pw, sw = ctx.band_lu(ab[None], b[None], kl, ku, method=WIDE)
    assert st_[0] == 0 and np.isfinite(xt).all()
    assert np.array_equal(pw, pt) and np.array_equal(sw, st_)
    assert _same_bits(xw, xt), np.flatnonzero(xw[0] != xt[0])[:10]


def _exact_case(n, kl, ku, seed):
    """A = L U with L unit lower (entries 0, +-1/2, +-i/2, 1/4, -i/4 inside kl) and U upper (diagonal 4 {+-1, +-i}, the rest
    0, +-1, +-i, +-1 + i inside ku); x small Gaussian integers, b = A x.  Every product and partial sum of the elimination
    and of both substitutions is a small multiple of 1/4: exact in any summation order.  Below the diagonal the candidates
    of column j are L[i, j] U[j, j], at most 2 against 4 in |re| + |im|: the diagonal wins every pivot search."""
    rng = np.random.default_rng(seed)
    lv = np.array([0, 0.5, -0.5, 0.5j, -0.5j, 0.25, -0.25j])
    uv = np.array([0, 1, -1, 1j, -1j, 1 + 1j, -1 + 1j])
    dv = 4 * np.array([1, -1, 1j, -1j])
    L = np.tril(np.triu(lv[rng.integers(0, len(lv), (n, n))], -kl), -1) + np.eye(n)
    U = np.triu(np.tril(uv[rng.integers(0, len(uv), (n, n))], ku), 1) + np.diag(dv[rng.integers(0, 4, n)])
    A = L @ U
    x = (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)
    b = A @ x
    kv = kl + ku
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    for k in range(-min(kl, n - 1), min(ku, n - 1) + 1):
        d = np.diagonal(A, k)
        if k >= 0:
            ab[kv - k, k:] = d
        else:
            ab[kv - k, :n + k] = d
    return ab, b, x


@pytest.mark.parametrize("n,kl,ku", [(200, 70, 40), (333, 100, 130), (150, 64, 64)])
def test_wide_exact_case(n, kl, ku):
    ctx = _ctx()
    ab, b, x = _exact_case(n, kl, ku, n)
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)                           # the construction holds what it promises
    assert info == 0 and np.array_equal(piv, np.arange(n)) and np.array_equal(lapack.zgbtrs(lu, kl, ku, b, piv)[0], x)
    ctx.band_set_method(WIDE)
    assert ctx.band_kernel_for(n, kl, ku) == (WIDE, 16)
    ctx.band_set_method(COLUMN)
    got = {m: ctx.band_lu(ab[None], b[None], kl, ku, method=m) for m in (WIDE, TILED, BLOCKED)}
    for m, (xm, pm, sm) in got.items():
        assert sm[0] == 0, m
        assert np.array_equal(pm[0], np.arange(n)), (m, np.flatnonzero(pm[0] != np.arange(n))[:10])
        assert _same_bits(xm[0], x), (m, np.flatnonzero(xm[0] != x)[:10])


def test_wide_gives_the_status_of_tiled_on_non_finite_input():
    ctx = _ctx()
    kl, ku = 70, 19
    cases = [_wide_case(200, kl, ku, s) for s in range(5)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[2, kl + ku, 100] = np.nan
    xt, pt, st_ = ctx.band_lu(ab, b, kl, ku, method=TILED)
    xw, pw, sw = ctx.band_lu(ab, b, kl, ku, method=WIDE)
    assert sw[2] == -1 and np.array_equal(sw, st_)
    assert np.array_equal(pw, pt)
    keep = [0, 1, 3, 4]
    assert (sw[keep] == 0).all()
    assert np.isfinite(xw[keep]).all()


def test_wide_rule():
    ctx = _ctx()
    ctx.band_set_method(WIDE)
    assert ctx.band_method() == WIDE == 4
    for kl in (15, 16, 63, 64, 1008, 1016, 1520, 1521, 3064, 3065, 4096, 4097):
        n = kl + 2000
        for ku in (5, 700):                                             # ku plays no part
            assert ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl), kl
            assert ctx.band_outer_nb(n, kl, ku) == (64 if 64 <= kl <= 4096 else 0), kl
    assert ctx.band_kernel_for(3000, 63, 5) == (TILED, 16) and ctx.band_kernel_for(3000, 64, 5) == (WIDE, 16)
    assert ctx.band_kernel_for(3000, 1016, 5) == (WIDE, 8) and ctx.band_kernel_for(6000, 4096, 5) == (WIDE, 4)
    assert ctx.band_kernel_for(6000, 4097, 5) == (COLUMN, 1) and ctx.band_kernel_for(6000, 15, 5) == (COLUMN, 1)
    with pytest.raises(_cabi.MausHipError):
        ctx.band_set_method(3)
    assert ctx.band_method() == WIDE
    for m in (COLUMN, BLOCKED, TILED):                                  # outside method 4 nothing runs wide
        ctx.band_set_method(m)
        assert ctx.band_outer_nb(3000, 100, 5) == 0
    ctx.band_set_method(TILED)
    assert ctx.band_kernel_for(3000, 100, 5) == (TILED, 16)


def _wide_ctx():
    ctx = _ctx()
    ctx.band_set_method(WIDE)
    return ctx


_NARROW = {}


def _narrow_operator():
    """2-D 5-point operator on a 72 x 72 grid: the ordering leaves kl = 72, between the outer block's width and twice that."""
    if not _NARROW:
        _NARROW["A"] = _five_point(72, 1)
    return _NARROW["A"]


@pytest.mark.parametrize("which", ["five_point_72", "wide_operator_2400"])
def test_wide_rows_do_not_depend_on_the_batch(which):
    ctx = _wide_ctx()
    A = _narrow_operator() if which == "five_point_72" else _wide_operator()[0]
    n, P = A.shape[0], 33
    perm, kl, ku = _bind(ctx, A, P)
    if which == "five_point_72":
        assert 64 <= kl < 128
    else:
        assert kl > 1024
    assert runs_wide(kl, ku) and ctx.band_kernel_for(n, kl, ku) == _expected_kernel(kl)
    assert ctx.band_kernel_for(n, kl, ku)[0] == WIDE and ctx.band_outer_nb(n, kl, ku) == 64
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
        c2 = _wide_ctx()
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


def test_wide_profile_class_and_workspace():
    ctx = _ctx()
    A = _narrow_operator()
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
    allocs = ctx.band_workspace_allocations()
    ctx.band_set_method(WIDE)                                           # the bound ordering stays; the workspace follows
    assert ctx.band_kernel_for(n, kl, ku)[0] == WIDE
    ctx.profile_enable(True)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert prof["band_wide"]["launches"] > 0 and prof["band_wide"]["flops"] > 0 and prof["band_wide"]["bytes"] > 0
    assert prof["band"]["launches"] == 0 and prof["band_blocked"]["launches"] == 0 and prof["band_tiled"]["launches"] == 0
    assert ctx.band_workspace_allocations() == allocs + 1               # re-reserved for the method, once
    Ww = ctx.pop_get(_cabi.POP_W, slots, n)
    for k in range(P):
        assert np.linalg.norm(Ww[k] - Wc[k]) <= 1e-10 * np.linalg.norm(Wc[k])
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    assert ctx.band_workspace_allocations() == allocs + 1
    ctx.band_set_method(TILED)                                          # tiled's workspace has no LW: another one
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    assert ctx.band_workspace_allocations() == allocs + 2


def test_wide_solver_loop_bodies_against_host():
    """test_tiled_solver_loop_bodies_against_host with sparse_direct='wide'."""
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from test_band_host import FakeBandContext
    compat = "scipy-legacy"
    A, b = _wide_operator()
    n = A.shape[0]
    host_ctx = FakeBandContext()
    ref_s, ref = _loop_bodies(A, b, DeviceEngine(ctx=host_ctx, gmres_compat=compat, sparse_mode="device", sparse_direct="band"),
                              compat)
    eng = DeviceEngine(gmres_compat=compat, sparse_mode="device", sparse_direct="wide")
    s, got = _loop_bodies(A, b, eng, compat)
    assert s.engine is eng and eng._band and eng.ctx.band_method() == WIDE
    perm, kl, ku = eng.band_shape(A)
    assert kl > 1024 and eng.ctx.band_kernel_for(n, kl, ku)[0] == WIDE
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


def test_inverse_iterate_solver_wide_against_spsolve():
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    _ctx()
    A, b = _wide_operator()
    n = A.shape[0]
    solver = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="wide")
    x, tries = solver.solve(A, b, 0)
    assert tries == 0
    ctx = InverseIterateSolver._ctx()
    assert ctx.band_method() == WIDE
    perm, kl, ku = band_order(A)
    assert kl > 1024 and ctx.band_kernel_for(n, kl, ku)[0] == WIDE
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
    # the next solver on the shared context asks for the column kernel again
    InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="band").solve(A, b, 0)
    assert ctx.band_method() == COLUMN


def test_maus_solver_wide_linear_system():
    """MAUS_Solver(sparse_direct='wide') end to end on the n = 2400 operator: the engine it builds selects method 4 and its
    candidates carry residuals that are the residuals of their x."""
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    _ctx()
    A, b = _wide_operator()
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}                 # as _loop_bodies; scipy-legacy: every solve direct
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=4, quiet=True, sparse_mode="device",
                    sparse_direct="wide", gmres_compat="scipy-legacy", diag_info=diag)
    assert s.engine.sparse_direct == "wide"
    s.loop_body(1)
    assert s.engine._band and s.engine.ctx.band_method() == WIDE
    checked = 0
    for c in s.candidates:
        if np.isfinite(c.residual_k):
            r = np.linalg.norm(A @ c.x_k - b)
            assert abs(r - c.residual_k) <= 1e-8 * r + 1e-12 * np.linalg.norm(b)
            checked += 1
    assert checked > 0
