"""real_arith="on" (maus_real_set_method, csrc/gmres.hip and csrc/spmm.hip; DESIGN §11 "GMRES in real arithmetic") on the
device (GPU box only): the real SpMM against the complex kernels' real part, real solves against the complex path of the same
context under np.array_equal on (x, info, inner, status), the rule and what runs under it, non-finite data, and whole loop
bodies of MAUS_Solver under real_arith="on" against "off".

No test claims equality before it has seen the real path run: maus_real_plan says so for the call at hand, and afterwards the
profile classes gmres_real / spmm_real have counted launches while vector, gmres_wide and spmm have counted none (and the
other way round for the complex run).  W is filled with NaN before every solve, so a solve that wrote nothing cannot pass."""
import random

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as gc
import real_cases as rc
import sell_cases as sc

pytestmark = pytest.mark.gpu

POP_X, POP_W, POP_Y = 0, 2, 3
SELL = 3


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


def _bind(ctx, A, b, P, spmm=0):
    """A and b on the device under method 1 (the real copies are built with the bind), sliced ELL forced where asked for."""
    ctx.spmm_set_method(spmm, sc.FORCE if spmm else 0)
    ctx.real_set_method(1)
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(max(P, 1))
    if b is not None:
        ctx.set_rhs(b)


def _solve(ctx, real, P, shift, psi, jac, gm=0, ticks=True, rhs_mode=1, why=None, **kw):
    """One maus_gmres call over slots 0 .. P - 1 under (real method, gmres method) -> (x, info, inner, status), after the checks
    of the module docstring.  why: the plan's verdict of a call that must run complex although the method is 1."""
    from adaptive_matrix_solver_amd import _cabi
    n = ctx.rows
    ctx.real_set_method(1 if (real or why is not None) else 0)
    ctx.gmres_set_method(gm)
    slots = np.arange(P)
    shift = np.asarray(shift, dtype=np.complex128)
    ctx.pop_put(POP_W, slots, np.full((P, n), np.nan + 0j))
    plan = ctx.real_plan(rhs_mode, shift)
    ctx.profile_enable(True)
    try:
        info, inner, status = ctx.gmres(slots, shift, np.asarray(psi, dtype=np.float64), rhs_mode, np.asarray(jac, dtype=np.int32), **kw)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    x = ctx.pop_get(POP_W, slots, n)
    mine = ("gmres_real", "spmm_real") if real else (("gmres_wide" if gm else "vector"), "spmm")
    other = ("vector", "gmres_wide", "spmm") if real else ("gmres_real", "spmm_real")
    if real:
        assert plan["real"] and plan["why"] == _cabi.REAL_OK, plan
        assert plan["post"] == ctx.gmres_kernel_for(n, True) and plan["spmm"] == ctx.spmm_kernel_for(False)
        assert plan["bytes"] > 0
    else:
        assert not plan["real"] and plan["why"] == (_cabi.REAL_METHOD_OFF if why is None else why), plan
    if ticks:
        for k in mine:
            assert prof[k]["launches"] > 0 and prof[k]["bytes"] > 0, (k, real, prof[k])
    for k in other:
        assert prof[k]["launches"] == 0, (k, real, prof[k])
    return x, np.asarray(info), np.asarray(inner), np.asarray(status)


def _same(r, c, tag=""):
    for a, b, what in zip(r, c, ("x", "info", "inner", "status")):
        assert np.array_equal(a, b), (tag, what, int(np.sum(np.asarray(a) != np.asarray(b))))
    assert not np.any(r[0].imag.view(np.uint64)), (tag, "the real path leaves imaginary parts of +0.0")


def _pair(ctx, P, shift, psi, jac, gm=0, ticks=True, tag="", **kw):
    r = _solve(ctx, True, P, shift, psi, jac, gm, ticks, **kw)
    c = _solve(ctx, False, P, shift, psi, jac, gm, ticks, **kw)
    _same(r, c, tag)
    assert np.all(np.isfinite(c[0])) and np.all(c[0].imag == 0.0), tag
    return c


def _batch(P, seed=1):
    """P candidates: real shifts and psi of their own, Jacobi off / on / mixed by thirds of the batch."""
    rng = np.random.default_rng(seed)
    shift = 0.2 * rng.standard_normal(P) + 0j
    psi = np.where(np.arange(P) % 2 == 0, 1e-19, 1e-3)
    jac = (np.arange(P) % 3 == 1).astype(np.int32)
    return shift, psi, jac


# ---- 1. products ------------------------------------------------------------------------------------------------------------
def _random_real(n, per_row, seed=1):
    return rc.real_csr(sc.random_pattern(n, per_row, seed))


PRODUCTS = {
    "tridiagonal_n1": lambda: rc.real_csr(sc.tridiagonal(1)),
    "tridiagonal_n63": lambda: rc.real_csr(sc.tridiagonal(63)),
    "tridiagonal_n64": lambda: rc.real_csr(sc.tridiagonal(64)),
    "tridiagonal_n65": lambda: rc.real_csr(sc.tridiagonal(65)),
    "random5_n129": lambda: _random_real(129, 5),
    "empty_slice_200": lambda: rc.real_csr(sc.empty_slice_200()),          # a whole empty slice: rows of no entry
    "ragged_256": lambda: rc.real_csr(sc.ragged_256()),                    # ragged slices: two rows of 64 among rows of 1
    "rows_of_33_n64": lambda: rc.rows_of_33(64),                           # the wave-per-row schedule, lanes 0 .. 32 busy
    "dense_rows_n65": lambda: _random_real(65, 60),                        # the wave-per-row schedule, rows of ~39
    "dense_rows_n129": lambda: _random_real(129, 90),
}
WAVE = ("rows_of_33_n64", "dense_rows_n65", "dense_rows_n129")


@pytest.mark.parametrize("spmm", [0, 1], ids=["csr", "sell"])
@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_products_are_the_complex_kernels_real_part(ctx, name, spmm):
    A = PRODUCTS[name]()
    n = A.shape[0]
    _bind(ctx, A, None, 33, spmm)
    kind = ctx.spmm_kernel_for(False)
    assert kind == (2 if name in WAVE else (SELL if spmm else 1)), (name, kind)      # the wave schedule has no sliced-ELL copy
    X = np.random.default_rng(4).standard_normal((33, n)) + 0j
    ctx.pop_put(POP_X, np.arange(33), X)
    ref = np.asarray(A @ X.T).T
    for count in (1, 8, 9, 33):
        slots = np.arange(33)[::-1][:count].copy()                         # gathered rows: not the identity list
        ctx.pop_put(POP_Y, slots, np.full((count, n), np.nan + 0j))
        ctx.profile_enable(True)
        ctx.matvec_rayleigh(slots)
        prof_c = ctx.profile_read()
        ctx.profile_enable(False)
        Yc = ctx.pop_get(POP_Y, slots, n)
        ctx.pop_put(POP_Y, slots, np.full((count, n), np.nan + 0j))
        ctx.profile_enable(True)
        ctx.real_spmm(slots)
        prof_r = ctx.profile_read()
        ctx.profile_enable(False)
        Yr = ctx.pop_get(POP_Y, slots, n)
        assert prof_c["spmm"]["launches"] == 1 and prof_c["spmm_real"]["launches"] == 0
        assert prof_r["spmm_real"]["launches"] == 1 and prof_r["spmm"]["launches"] == 0
        assert np.all(Yc.imag == 0.0) and not np.any(Yr.imag.view(np.uint64)), (name, count)
        assert np.array_equal(Yr.real, Yc.real), (name, count, int(np.sum(Yr.real != Yc.real)))
        assert np.allclose(Yc, ref[slots], rtol=1e-12, atol=1e-12), (name, count)


# ---- 2. solves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spmm", [0, 1], ids=["csr", "sell"])
@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
@pytest.mark.parametrize("n", [1, 2, 64, 511, 512, 513, 1023, 1025])
def test_solves_at_the_size_edges(ctx, n, gm, spmm):
    """Both sides of one piece of the wide step (512), of 1024 (the register kernels' first boundary and two pieces) and n below
    the restart length; 15 candidates with Jacobi off / on / mixed within the call, every one converged."""
    A, b = rc.banded(n), rc.real_vec(n, n)
    _bind(ctx, A, b, 15, spmm)
    assert ctx.spmm_kernel_for(False) == (SELL if spmm else 1)
    shift, psi, jac = _batch(15)
    x, info, inner, status = _pair(ctx, 15, shift, psi, jac, gm, tag=f"n{n}")
    assert np.all(info == 0) and np.all(status == 0) and np.all(inner >= 1)


@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
@pytest.mark.parametrize("n", [16384, 16385])
def test_register_and_stream_boundary(ctx, n, gm):
    """One tridiagonal system on either side of the last register kernel (n = 16384) and the stream kernel (16385)."""
    A, b = rc.tridiagonal(n), rc.real_vec(3, n)
    _bind(ctx, A, b, 1)
    ctx.gmres_set_method(gm)
    assert ctx.gmres_kernel_for(n, True) == (2 if gm else (0 if n == 16384 else 1))
    x, info, inner, status = _pair(ctx, 1, [0.0], [1e-20], [0], gm, tag=f"n{n}")
    assert info[0] == 0 and status[0] == 0


@pytest.mark.parametrize("jacobi", ["off", "on", "mixed"])
@pytest.mark.parametrize("P", [1, 15, 33])
def test_candidate_counts_and_jacobi(ctx, P, jacobi):
    n = 513
    _bind(ctx, rc.banded(n, 1, 2.2), rc.real_vec(n, n), P)
    shift, psi, jac = _batch(P, seed=P)
    jac = {"off": np.zeros(P, dtype=np.int32), "on": np.ones(P, dtype=np.int32), "mixed": jac}[jacobi]
    for gm in (0, 1):
        x, info, inner, status = _pair(ctx, P, shift, psi, jac, gm, tag=f"P{P} {jacobi} gm{gm}")
        assert np.all(info == 0) and inner.max() > 20                      # more than one restart cycle


def _diag40():
    return sp.csr_matrix(np.diag(np.arange(1.0, 41.0)).astype(np.complex128)), gc.unit_vector(40, 3, 2.0)


EXITS = {
    # name: (A, b, jacobi, kwargs, (info, inner), ticks)
    "inner1_breakdown": lambda: _diag40() + (0, {}, (0, 1), True),
    "inner1_breakdown_j1": lambda: _diag40() + (1, {}, (0, 1), True),
    "inner20_cyclic": lambda: (rc.cyclic(20), gc.unit_vector(20, 0), 0, {}, (0, 20), True),
    "inner20_restart_boundary": lambda: (rc.banded(300, 1, 2.2), rc.real_vec(300, 300), 0, dict(rtol=1e-4), (0, 20), True),
    "inner21_second_cycle": lambda: (rc.banded(300, 1, 1.0), rc.real_vec(300, 300), 0, dict(rtol=1e-10), (0, 21), True),
    "maxiter_exit": lambda: (rc.cyclic(21), gc.unit_vector(21, 0), 0, dict(maxiter=4), (4, 80), True),
    "zero_rhs": lambda: (rc.banded(33), np.zeros(33, dtype=np.complex128), 0, {}, (0, 0), False),
    "restart1": lambda: (rc.banded(64), rc.real_vec(64, 64), 0, dict(restart=1), None, True),
    "restart1_j1": lambda: (rc.banded(64), rc.real_vec(64, 64), 1, dict(restart=1), None, True),
    "n_below_restart": lambda: (rc.cyclic(8), gc.unit_vector(8, 0), 0, {}, (0, 8), True),
}


@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
@pytest.mark.parametrize("name", sorted(EXITS))
def test_exits_and_restart_edges(ctx, name, gm):
    """Convergence at inner 1 (breakdown at column 0), at the end of the first cycle (inner 20: stagnation that closes, and a
    banded system whose tolerance is met by the 20th column), in the first column of the second cycle (inner 21), exhaustion
    (info = maxiter after 4 cycles of 20), b = 0 (no tick at all), restart = 1 and n below the restart length.  The counts of
    the banded systems come from gmres_cases.traced on the CPU, 0.2 away (in the logarithm) from the nearest decision."""
    A, b, jac, kw, expect, ticks = EXITS[name]()
    _bind(ctx, A, b, 1)
    x, info, inner, status = _pair(ctx, 1, [0.0], [0.0], [jac], gm, ticks=ticks, tag=name, **kw)
    if expect is not None:
        assert (int(info[0]), int(inner[0])) == expect, (name, info, inner)
    assert status[0] == 0


@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
def test_a_candidate_alone_and_among_33(ctx, gm):
    n = 513
    _bind(ctx, rc.banded(n, 1, 2.2), rc.real_vec(n, n), 33)
    shift, psi, jac = _batch(33, seed=9)
    many = _solve(ctx, True, 33, shift, psi, jac, gm)
    for k in (0, 16, 32):
        one = _solve(ctx, True, 1, shift[k:k + 1], psi[k:k + 1], jac[k:k + 1], gm)
        _same(one, tuple(a[k:k + 1] for a in many), f"candidate {k}")


# ---- 3. the rule ------------------------------------------------------------------------------------------------------------
def _system(n=300):
    return rc.banded(n), rc.real_vec(n, n)


def test_rule_negative_zero_is_real(ctx):
    A, b = _system()
    An = sp.csr_matrix((np.conj(A.data), A.indices, A.indptr), shape=A.shape)          # imaginary parts -0.0
    assert np.all(np.signbit(An.data.imag)) and np.all(np.signbit(np.conj(b).imag))
    _bind(ctx, An, np.conj(b), 3)
    shift = np.array([complex(0.1, -0.0), complex(-0.2, 0.0), complex(0.0, -0.0)])
    for gm in (0, 1):
        _pair(ctx, 3, shift, [1e-19] * 3, [0, 1, 0], gm, tag="-0.0")


def test_rule_what_runs_complex(ctx):
    from adaptive_matrix_solver_amd import _cabi
    A, b = _system()
    n = A.shape[0]
    shift3, psi3, jac3 = np.array([0.1, -0.2, 0.0]) + 0j, [1e-19] * 3, [0, 1, 0]
    # a smallest denormal in one imaginary part of the matrix
    Ad = A.copy()
    Ad.data.view(np.float64)[2 * n + 1] = 5e-324
    _bind(ctx, Ad, b, 3)
    bytes_b = ctx.real_plan(1, shift3)["bytes"]
    assert bytes_b == 8 * n                                                             # b's copy alone: no operand copy
    _solve(ctx, False, 3, shift3, psi3, jac3, why=_cabi.REAL_MATRIX_COMPLEX)
    # a complex b (also: the smallest denormal, NaN in an imaginary part)
    _bind(ctx, A, b, 3)
    full = ctx.real_plan(1, shift3)["bytes"]
    assert full == 8 * (A.nnz + 2 * n)                                                  # values, diagonal, b
    tiny, nan = b.copy(), b.copy()
    tiny.view(np.float64)[2 * 7 + 1] = 5e-324
    nan.view(np.float64)[2 * 7 + 1] = np.nan
    for bad in (b + 1j * b, tiny, nan):
        ctx.set_rhs(bad)
        assert ctx.real_plan(1, shift3)["bytes"] == 8 * (A.nnz + n)
        _solve(ctx, False, 3, shift3, psi3, jac3, why=_cabi.REAL_RHS_COMPLEX)
    ctx.set_rhs(b)
    assert ctx.real_plan(1, shift3)["bytes"] == full
    # one complex shift in the call: the whole call
    for bad in (np.array([0.1, -0.2 + 1e-3j, 0.0]), np.array([0.1, -0.2, complex(0.0, 5e-324)])):
        _solve(ctx, False, 3, bad, psi3, jac3, why=_cabi.REAL_SHIFT_COMPLEX)
    # the population rows as right-hand sides
    ctx.pop_put(POP_X, np.arange(3), np.stack([b, 2 * b, -b]))
    _solve(ctx, False, 3, shift3, psi3, jac3, rhs_mode=0, why=_cabi.REAL_RHS_ROWS)
    # and all of it real again: the same context still takes the real path
    _pair(ctx, 3, shift3, psi3, jac3, tag="back")
    # a dense matrix
    ctx.real_set_method(1)                                                              # _pair left the complex run's method 0
    ctx.set_matrix(A.toarray())
    ctx.set_rhs(b)
    plan = ctx.real_plan(1, shift3)
    assert not plan["real"] and plan["why"] == _cabi.REAL_NOT_CSR and plan["post"] == -1 and plan["bytes"] == 8 * n


def test_rule_method_0_allocates_nothing_and_rebinding_drops_the_copies():
    from adaptive_matrix_solver_amd import Context, _cabi
    A, b = _system()
    n = A.shape[0]
    c = Context(0)
    try:
        assert c.real_method() == 0
        c.set_matrix_csr(A)
        c.pop_reserve(2)
        c.set_rhs(b)
        x0 = _solve(c, False, 2, [0.1, 0.0], [0.0, 0.0], [0, 1])
        plan = c.real_plan(1, np.zeros(2))
        assert plan == dict(plan, real=False, why=_cabi.REAL_METHOD_OFF, allocs=0, bytes=0)
        with pytest.raises(_cabi.MausHipError, match="maus_real_spmm"):
            c.real_spmm([0])
        with pytest.raises(_cabi.MausHipError, match="method must be 0"):
            c.real_set_method(2)
        assert c.real_method() == 0
        c.real_set_method(1)                                                            # with a matrix and b bound: built now
        plan = c.real_plan(1, np.zeros(2))
        assert plan["real"] and plan["allocs"] == 3 and plan["bytes"] == 8 * (A.nnz + 2 * n)
        x1 = _solve(c, True, 2, [0.1, 0.0], [0.0, 0.0], [0, 1])
        _same(x1, x0, "set after the bind")
        assert c.real_plan(1, np.zeros(2))["allocs"] == 3                               # a solve allocates none of them
        c.spmm_set_method(1, sc.FORCE)                                                  # the sliced-ELL copy brings its real values
        plan = c.real_plan(1, np.zeros(2))
        assert plan["spmm"] == SELL and plan["allocs"] == 4 and plan["bytes"] == 8 * (A.nnz + 2 * n + c.spmm_sell_info(False)[1])
        _same(_solve(c, True, 2, [0.1, 0.0], [0.0, 0.0], [0, 1]), x0, "sell")
        c.spmm_set_method(0)
        assert c.real_plan(1, np.zeros(2))["bytes"] == 8 * (A.nnz + 2 * n)
        c.set_matrix_csr(gc.banded(n, 1, 1.0))                                          # a complex matrix of the same shape
        plan = c.real_plan(1, np.zeros(2))
        assert not plan["real"] and plan["why"] == _cabi.REAL_MATRIX_COMPLEX and plan["bytes"] == 8 * n
        c.set_rhs(b + 1j * b)
        assert c.real_plan(1, np.zeros(2))["bytes"] == 0
        c.set_matrix_csr(A)                                                             # the method is kept across matrices
        c.set_rhs(b)
        assert c.real_method() == 1 and c.real_plan(1, np.zeros(2))["real"]
        c.real_set_method(0)
        plan = c.real_plan(1, np.zeros(2))
        assert plan["bytes"] == 0 and plan["why"] == _cabi.REAL_METHOD_OFF
        _same(_solve(c, False, 2, [0.1, 0.0], [0.0, 0.0], [0, 1]), x0, "off again")
    finally:
        c.close()


# ---- 4. non-finite data -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
def test_nan_in_b_ends_at_once_with_the_complex_outcome(ctx, gm):
    A, b = _system()
    b = b.copy()
    b[17] = np.nan
    _bind(ctx, A, b, 2)
    r = _solve(ctx, True, 2, [0.0, 0.1], [0.0, 0.0], [0, 1], gm)
    c = _solve(ctx, False, 2, [0.0, 0.1], [0.0, 0.0], [0, 1], gm)
    for i in (1, 2, 3):
        assert np.array_equal(r[i], c[i]), i
    assert np.all(c[1] == 50) and np.all(c[2] == 0)                        # info = maxiter from the first residual, no iteration
    assert np.array_equal(np.isfinite(r[0].real), np.isfinite(c[0].real))


@pytest.mark.parametrize("gm", [0, 1], ids=["auto", "wide"])
def test_inf_in_the_matrix_gives_the_complex_info_and_status(ctx, gm):
    A, b = _system()
    A = A.copy()
    A.data[40] = np.inf
    assert rc.flagged_real(A.data)
    _bind(ctx, A, b, 2)
    r = _solve(ctx, True, 2, [0.0, 0.1], [0.0, 0.0], [0, 1], gm, maxiter=3)
    c = _solve(ctx, False, 2, [0.0, 0.1], [0.0, 0.0], [0, 1], gm, maxiter=3)
    assert np.array_equal(r[1], c[1]) and np.array_equal(r[3], c[3])
    assert np.all(c[1] == 3)


# ---- 5. loop bodies ---------------------------------------------------------------------------------------------------------
def _bodies(A, b, kind, real_arith, bodies=4, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    ptype = ProblemType.EIGENVALUE if kind == "eig" else ProblemType.SOLVE_LINEAR_SYSTEM
    s = MAUS_Solver(A, ptype, b_vector=b if kind == "lin" else None, initial_num_candidates=6, quiet=True, gmres_compat="rtol",
                    sparse_mode="device", diag_info=diag, real_arith=real_arith, **kw)
    ctx = s.engine.ctx
    try:
        ctx.profile_enable(True)
        rows = []
        for it in range(bodies):
            s.loop_body(it + 1)
            rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                         np.array([float(c.residual_k) for c in s.candidates]),
                         np.random.get_state()[2], np.random.get_state()[1].copy(), random.getstate()))
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        cap, n = ctx.pop_capacity(), A.shape[0]
        dev = [ctx.pop_get(w, np.arange(cap), n) for w in (0, 1, 2, 3)]
        method = ctx.real_method()
        plan = ctx.real_plan(1, np.zeros(1)) if kind == "lin" else None
    finally:
        ctx.close()
    return rows, dev, prof, method, plan


def _same_bodies(off, on):
    for (r_rows, r_res, r_pos, r_key, r_py), (g_rows, g_res, g_pos, g_key, g_py) in zip(off[0], on[0]):
        assert r_rows == g_rows
        assert np.array_equal(r_res, g_res, equal_nan=True)
        assert r_pos == g_pos and np.array_equal(r_key, g_key) and r_py == g_py
    for a, b in zip(off[1], on[1]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["tridiagonal_n600", "five_point_n625"])
def test_loop_bodies_register_kernels(name):
    A = rc.tridiagonal(600) if name == "tridiagonal_n600" else rc.five_point(25)
    b = rc.real_vec(42, A.shape[0])
    off = _bodies(A, b, "lin", "off")
    on = _bodies(A, b, "lin", "on")
    assert on[3] == 1 and on[4]["real"] and on[4]["post"] == 0 and off[3] == 0
    # `vector` also counts the relax / residual kernels of a loop body: the post steps are what the real run has fewer of
    assert on[2]["gmres_real"]["launches"] > 0 and on[2]["spmm_real"]["launches"] > 0
    assert off[2]["gmres_real"]["launches"] == 0 and off[2]["spmm_real"]["launches"] == 0
    assert off[2]["vector"]["launches"] - on[2]["vector"]["launches"] == on[2]["gmres_real"]["launches"]
    assert off[2]["spmm"]["launches"] - on[2]["spmm"]["launches"] == on[2]["spmm_real"]["launches"]
    assert on[2]["spmm"]["launches"] > 0                                   # the residual products stay complex
    _same_bodies(off, on)


@pytest.mark.parametrize("gmres", ["auto", "wide"])
def test_loop_bodies_n20000_stream_and_wide(gmres):
    """n = 20000 under sparse_direct='narrow', sparse_split='on': the GMRES solves run real (the stream kernel, or the wide
    step), the direct fallback and the residual products complex as ever."""
    A = rc.tridiagonal(20000)
    b = rc.real_vec(43, 20000)
    kw = dict(sparse_direct="narrow", sparse_split="on", sparse_gmres=gmres)
    off = _bodies(A, b, "lin", "off", **kw)
    on = _bodies(A, b, "lin", "on", **kw)
    assert on[3] == 1 and on[4]["real"] and on[4]["post"] == (2 if gmres == "wide" else 1)
    assert on[2]["gmres_real"]["launches"] > 0 and on[2]["spmm_real"]["launches"] > 0
    assert off[2]["gmres_real"]["launches"] == 0 and off[2]["spmm_real"]["launches"] == 0
    post = "gmres_wide" if gmres == "wide" else "vector"               # `vector` also counts the relax / residual kernels
    assert off[2][post]["launches"] - on[2][post]["launches"] == on[2]["gmres_real"]["launches"]
    assert on[2]["gmres_wide"]["launches"] == 0
    assert off[2]["spmm"]["launches"] - on[2]["spmm"]["launches"] == on[2]["spmm_real"]["launches"]
    for k in ("band", "band_split"):
        assert on[2][k]["launches"] == off[2][k]["launches"]
    _same_bodies(off, on)


def test_eigenvalue_problem_takes_no_real_path_call():
    A = rc.tridiagonal(600)
    off = _bodies(A, None, "eig", "off")
    on = _bodies(A, None, "eig", "on")
    assert on[3] == 1 and off[3] == 0
    assert on[2]["gmres_real"]["launches"] == 0 and on[2]["spmm_real"]["launches"] == 0
    assert on[2]["vector"]["launches"] == off[2]["vector"]["launches"] > 0
    _same_bodies(off, on)
