"""The lane-per-row SpMM on a sliced-ELL copy of the operand (sparse_spmm="sell", maus_spmm_set_method(ctx, 1), csrc/spmm.hip;
DESIGN §10 "SpMM on a sliced-ELL copy").

A lane still owns a row and adds its nonzeros in CSR order with the same fused operations, so every comparison here is
np.array_equal on the complex arrays against a second context under method 0 -- no tolerance anywhere.  Every case first asks
the library (spmm_kernel_for) which kernel really runs, and maus_spmm_plan must agree with it on the NumPy restatement of the
layout (tests/sell_cases.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import sell_cases as sc

pytestmark = pytest.mark.gpu

POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3
ROWS, WAVE, SELL = 1, 2, 3
CAP = 64                                       # population rows reserved by the product tests


@pytest.fixture(scope="module")
def pair():
    """(context under method 0, context under method 1): the same binds go to both"""
    from adaptive_matrix_solver_amd import Context
    c0, c1 = Context(0), Context(0)
    yield c0, c1
    c0.close()
    c1.close()


def _vectors(A, count=CAP, seed=3):
    rng = np.random.default_rng(seed)
    m, n = A.shape
    return (rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n)),
            rng.standard_normal((count, m)) + 1j * rng.standard_normal((count, m)))


def _bind(pair, A, cap, count=CAP):
    """Bind A to both contexts, the second under (method 1, cap); the kernels both report must be what maus_spmm_plan says for
    the NumPy layout, and what is resident must be that layout's size."""
    from adaptive_matrix_solver_amd._cabi import spmm_plan
    c0, c1 = pair
    c0.spmm_set_method(0)
    c1.spmm_set_method(1, cap)
    kinds = []
    for c, method in ((c0, 0), (c1, 1)):
        c.set_matrix_csr(A)
        c.pop_reserve(count)
        for adjoint, M in ((False, A), (True, sc.adjoint(A))):
            off, _ln, padded = sc.sell_layout(M)
            kind = c.spmm_kernel_for(adjoint)
            # the schedule belongs to the matrix: plan takes the rows of A for both operands
            assert kind == spmm_plan(method, cap if method else 0, A.shape[0], M.nnz, padded) == sc.expected_kind(M, method, cap, A.shape[0])
            want = (len(off) - 1, padded, 20 * padded + 4 * M.shape[0] + 8 * len(off)) if kind == SELL else (0, 0, 0)
            assert c.spmm_sell_info(adjoint) == want
            kinds.append(kind)
    assert kinds[0] != SELL and kinds[1] != SELL
    return kinds[2], kinds[3]


def _products(ctx, A, V, U, slots):
    """(A v, A^H u) of the rows `slots` through the SVD residual: Y = A X and W = A^H U, both always recomputed there."""
    m, n = A.shape
    ctx.pop_put(POP_X, slots, V[slots])
    ctx.pop_put(POP_U, slots, U[slots])
    ctx.residual(3, slots, np.zeros(len(slots), dtype=np.complex128))
    return ctx.pop_get(POP_Y, slots, m), ctx.pop_get(POP_W, slots, n)


def _same_products(pair, A, V, U, slots):
    got0, got1 = (_products(c, A, V, U, slots) for c in pair)
    for a, b in zip(got0, got1):
        assert np.array_equal(np.isnan(a.real), np.isnan(b.real)) and np.array_equal(np.isnan(a.imag), np.isnan(b.imag))
        assert np.array_equal(a.view(np.float64), b.view(np.float64), equal_nan=True)
    return got1


def _bit_identity(pair, A, count=CAP, Ps=(1, 7, 8, 9, 33)):
    V, U = _vectors(A, count)
    order = np.random.default_rng(11).permutation(count)
    for P in Ps:                                                       # scattered, permuted slots
        _same_products(pair, A, V, U, order[:P].tolist())
    # the same rows alone, among 33 and in another order, under the sliced-ELL kernel
    base = order[:33].tolist()
    y, w = _same_products(pair, A, V, U, base)
    for k in (0, 16, 32):
        y1, w1 = _same_products(pair, A, V, U, [base[k]])
        assert np.array_equal(y1[0], y[k]) and np.array_equal(w1[0], w[k])
    shuffled = np.random.default_rng(12).permutation(33)
    y2, w2 = _same_products(pair, A, V, U, [base[k] for k in shuffled])
    assert np.array_equal(y2, y[shuffled]) and np.array_equal(w2, w[shuffled])
    want_y, want_w = (A @ V[base].T).T, (sc.adjoint(A) @ U[base].T).T
    assert np.linalg.norm(y - want_y) <= 1e-13 * np.linalg.norm(want_y) + 1e-300
    assert np.linalg.norm(w - want_w) <= 1e-13 * np.linalg.norm(want_w) + 1e-300


# ---- 1. bit identity, both operands --------------------------------------------------------------------------------------
FORCED = {
    "1x1": lambda: sc.tridiagonal(1),
    "tridiag63": lambda: sc.tridiagonal(63),
    "tridiag64": lambda: sc.tridiagonal(64),
    "tridiag65": lambda: sc.tridiagonal(65),
    "tridiag129": lambda: sc.tridiagonal(129),
    "empty_slice200": sc.empty_slice_200,
    "ragged256": sc.ragged_256,
    "rect200x70": lambda: sc.rect(200, 70, 3),
    "rect70x200": lambda: sc.rect(70, 200, 4),
    "tall1000x10": sc.tall_1000x10,
}


@pytest.mark.parametrize("name", list(FORCED))
def test_bit_identity_forced(pair, name):
    A = FORCED[name]()
    assert _bind(pair, A, sc.FORCE) == (SELL, SELL)
    _bit_identity(pair, A)


def test_bit_identity_27_per_row_4096_unforced(pair):
    A = sc.random_pattern(4096, 27)
    assert _bind(pair, A, 0, count=256) == (SELL, SELL)                # fills 1.00 and 1.47: inside the default cap
    V, U = _vectors(A, 256)
    y, w = _same_products(pair, A, V, U, list(range(256)))
    want = (A @ V.T).T
    assert np.linalg.norm(y - want) <= 1e-13 * np.linalg.norm(want)
    perm = np.random.default_rng(9).permutation(256)
    y2, w2 = _same_products(pair, A, V, U, perm.tolist())
    assert np.array_equal(y2, y[perm]) and np.array_equal(w2, w[perm])
    y1, w1 = _same_products(pair, A, V, U, [5])
    assert np.array_equal(y1[0], y[5]) and np.array_equal(w1[0], w[5])


def test_wide_matrix_keeps_the_wave_schedule_for_both_operands(pair):
    """10 x 1000 with nnz > 32 rows: the CSR kernels run A and A^H a wave per row, whose sums are joined by a tree; A^H alone
    (1000 rows of at most a few entries) would pass for a lane-per-row operand, and a copy of it would change the bits."""
    A = sc.wide_10x1000()
    assert A.nnz > 32 * A.shape[0] and A.nnz <= 32 * A.shape[1]
    for cap in (0, sc.FORCE):
        assert _bind(pair, A, cap) == (WAVE, WAVE)
        assert pair[1].matrix_is_sparse() == "wave" and pair[1].spmm_sell_info(True) == (0, 0, 0)
    _bit_identity(pair, A)


# ---- 2. exactness ---------------------------------------------------------------------------------------------------------
def test_small_integers_are_exact(pair):
    n = 65
    rng = np.random.default_rng(21)
    d = [rng.integers(-9, 10, n - abs(o)) + 1j * rng.integers(-9, 10, n - abs(o)) for o in (-1, 0, 1)]
    d = [np.where(x == 0, 1 + 1j, x) for x in d]                       # every stored entry nonzero
    A = sc.csr(sp.diags(d, [-1, 0, 1], shape=(n, n)))
    assert _bind(pair, A, sc.FORCE) == (SELL, SELL)
    V = (rng.integers(-9, 10, (CAP, n)) + 1j * rng.integers(-9, 10, (CAP, n))).astype(np.complex128)
    U = (rng.integers(-9, 10, (CAP, n)) + 1j * rng.integers(-9, 10, (CAP, n))).astype(np.complex128)
    slots = list(range(33))
    AH = sc.adjoint(A)
    for c in pair:                                                     # under both methods
        y, w = _products(c, A, V, U, slots)
        assert np.array_equal(y, (A @ V[slots].T).T) and np.array_equal(w, (AH @ U[slots].T).T)


# ---- 3. padding is never multiplied ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cols", [("tridiag129", (0, 70)), ("ragged256", (0, 200))])
def test_padding_is_never_multiplied(pair, name, cols):
    """Padding slots carry index 0: a kernel that multiplied them would put 0 * inf = NaN into every padded row once x[0] = inf.
    ragged256 pads 64 slots in every lane of its second slice."""
    A = FORCED[name]()
    assert _bind(pair, A, sc.FORCE) == (SELL, SELL)
    V, U = _vectors(A)
    for X in (V, U):
        X[:, cols[0]] = np.inf
        X[:, cols[1]] = np.nan
    slots = list(range(9))
    y, w = _same_products(pair, A, V, U, slots)                        # NaN positions included
    for M, out in ((A, y), (sc.adjoint(A), w)):
        touched = np.zeros(M.shape[0], dtype=bool)
        for j in cols:
            touched |= np.asarray((M[:, [j]] != 0).todense()).ravel()
        assert touched.any() and not touched.all()
        assert np.isfinite(out[:, ~touched]).all()                     # rows that reference neither column
        assert not np.isfinite(out[:, touched]).all()


# ---- 4. the rule ----------------------------------------------------------------------------------------------------------
def test_rule_under_the_default_cap(pair):
    A = sc.random_pattern(200, 5)
    assert round(sc.fill(A), 2) == 1.29 and round(sc.fill(sc.adjoint(A)), 2) == 2.58
    assert _bind(pair, A, 0) == (SELL, ROWS)                           # A and A^H are judged separately
    _bit_identity(pair, A, Ps=(9,))
    B = sc.random_pattern(2048, 100)
    assert _bind(pair, B, 0) == (WAVE, WAVE)
    assert pair[1].matrix_is_sparse() == "wave"
    assert pair[1].spmm_sell_info(False) == (0, 0, 0) and pair[1].spmm_sell_info(True) == (0, 0, 0)
    assert _bind(pair, B, sc.FORCE) == (WAVE, WAVE)                    # no cap puts the wave schedule on the copy
    _bit_identity(pair, B, Ps=(9,))


# ---- 5. lifetime ----------------------------------------------------------------------------------------------------------
def test_lifetime():
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import MausHipError
    A, B = sc.tridiagonal(129), sc.random_pattern(200, 5)
    V, U = _vectors(A)
    slots = list(range(9))
    c = Context(0)
    try:
        assert c.spmm_method() == 0 and c.spmm_kernel_for(False) == 0 and c.spmm_sell_info(False) == (0, 0, 0)
        c.spmm_set_method(1)                                           # before any matrix: kept
        assert c.spmm_method() == 1 and c.spmm_kernel_for(False) == 0
        c.set_matrix_csr(A)                                            # built at bind time
        c.pop_reserve(CAP)
        info = c.spmm_sell_info(False)
        assert c.spmm_kernel_for(False) == SELL and info[1] == 512 and info[2] > 0
        ref = _products(c, A, V, U, slots)
        c.set_matrix_csr(B)                                            # the method survives a rebind
        assert c.spmm_method() == 1 and (c.spmm_kernel_for(False), c.spmm_kernel_for(True)) == (SELL, ROWS)
        assert c.spmm_sell_info(True) == (0, 0, 0)
        c.set_matrix(A.toarray())                                      # sparse -> dense frees
        assert c.spmm_method() == 1 and c.spmm_kernel_for(False) == 0 and c.spmm_sell_info(False) == (0, 0, 0)
        c.set_matrix_csr(A)                                            # ... -> sparse rebuilds: the same arrays' sizes
        c.pop_reserve(CAP)
        assert c.spmm_sell_info(False) == info and c.spmm_sell_info(True) == info
        for bad in ((2, 0), (-1, 0), (1, 99), (1, 1000001), (0, 50)):  # an error that changes nothing
            with pytest.raises(MausHipError, match="maus_spmm_set_method"):
                c.spmm_set_method(*bad)
            assert c.spmm_method() == 1 and c.spmm_sell_info(False) == info and c.spmm_kernel_for(False) == SELL
        c.spmm_set_method(0)                                           # frees at once
        assert c.spmm_kernel_for(False) == ROWS and c.spmm_sell_info(False) == (0, 0, 0)
        got = _products(c, A, V, U, slots)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        c.spmm_set_method(1)                                           # after the bind: builds at once
        assert c.spmm_kernel_for(False) == SELL and c.spmm_sell_info(False) == info
        got = _products(c, A, V, U, slots)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref))
        c.spmm_set_method(1, 100)                                      # another cap re-judges the bound operands (fill 1.33)
        assert c.spmm_kernel_for(False) == ROWS and c.spmm_sell_info(False) == (0, 0, 0)
    finally:
        c.close()


# ---- 6. through the stack -------------------------------------------------------------------------------------------------
def _same(a, b, path="run"):
    """plain equality of nested results, NaN equal to NaN"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype, path
        assert np.array_equal(a, b, equal_nan=True), path
    elif isinstance(a, (float, complex, np.floating, np.complexfloating)):
        assert a == b or (a != a and b != b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def _plan_agrees(ctx, A, cap):
    """maus_spmm_kernel_for of both operands of the bound sparse matrix A against maus_spmm_plan on the NumPy layout, under the
    context's method and the cap it was given; returns the two kinds"""
    from adaptive_matrix_solver_amd._cabi import spmm_plan
    A = sc.csr(A)
    kinds = []
    for adjoint, M in ((False, A), (True, sc.adjoint(A))):
        padded = sc.sell_layout(M)[2]
        kinds.append(ctx.spmm_kernel_for(adjoint))
        assert kinds[-1] == spmm_plan(ctx.spmm_method(), cap, A.shape[0], M.nnz, padded)
        assert ctx.spmm_sell_info(adjoint)[1] == (padded if kinds[-1] == SELL else 0)
    return tuple(kinds)


def _engine(mode):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    eng = DeviceEngine(gmres_compat=mode[0], sparse_mode="device", **({"sparse_spmm": mode[1]} if mode[1] else {}))
    if mode[1] == "sell":
        assert eng.ctx.spmm_method() == 1
        eng.ctx.spmm_set_method(1, sc.FORCE)                           # these matrices are tiny: the copy for every operand
    else:
        assert eng.sparse_spmm == "auto" and eng.ctx.spmm_method() == 0
    calls = []
    inner = eng.ctx.gmres

    def gmres(*a, **kw):
        out = inner(*a, **kw)
        calls.append(tuple(np.array(x) for x in out))
        return out

    eng.ctx.gmres = gmres
    return eng, calls


def _scenario_names():
    import sparse_scenarios
    return [(n, m) for n, s in sparse_scenarios.SPARSE_TRAJECTORIES.items() for m in s["modes"]]


@pytest.mark.parametrize("name,compat", _scenario_names())
def test_loop_bodies_are_identical(name, compat):
    """Every trajectory of the sparse scenarios: vectors, lambda / sigma, residuals, bookkeeping, both RNG stream positions (the
    rows of test_gpu_sparse._run) and every GMRES call's (info, inner counts, status)."""
    import sparse_scenarios
    import test_gpu_sparse as tgs
    iters = sparse_scenarios.SPARSE_TRAJECTORIES[name]["iters"]
    runs = []
    for spmm in (None, "sell"):
        eng, calls = _engine((compat, spmm))
        try:
            out, _ = tgs._run(name, iters, eng, compat)
            if eng.ctx.matrix_is_sparse():
                kinds = _plan_agrees(eng.ctx, eng._bound, sc.FORCE if spmm == "sell" else 0)
                if eng.ctx.matrix_is_sparse() == "rows":
                    assert kinds == ((SELL, SELL) if spmm == "sell" else (ROWS, ROWS))
            runs.append((out, calls))
        finally:
            eng.ctx.close()
    _same(runs[0], runs[1])


def _hermitian_tridiagonal(n, seed=31):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    return sc.csr(sp.diags([e.conj(), 4.0 * rng.standard_normal(n), e], [-1, 0, 1], shape=(n, n)))


def test_lanczos_is_identical():
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd.engine import thick_restart_lanczos
    n = 4096
    A = _hermitian_tridiagonal(n)
    v0 = np.random.default_rng(32).standard_normal(n) + 0j
    anorm = float(abs(A).sum(axis=0).max())
    runs = []
    for method in (0, 1):
        c = Context(0)
        try:
            c.spmm_set_method(method)
            c.set_matrix_csr(A)
            assert _plan_agrees(c, A, 0) == ((SELL, SELL) if method else (ROWS, ROWS))
            steps, extend = [], c.lanczos_extend

            def recording(*a, _steps=steps, _extend=extend):
                out = _extend(*a)
                _steps.append(tuple(np.array(x) for x in out))
                return out

            c.lanczos_extend = recording
            run = thick_restart_lanczos(c, n, 6, 20, 1e-10, np.finfo(float).eps * anorm, 60, v0, lambda: 1 / 0)
            rows = c.get_ritz_rows() if run["converged"] else None
            runs.append((run, steps, rows))
        finally:
            c.close()
    assert runs[0][0]["products"] > 20 and len(runs[0][1]) >= 1
    _same(runs[0], runs[1])                                            # alpha, beta, the Ritz values and rows, the restart count


def test_band_solve_is_unchanged():
    """The H build of the band solve reads the CSR arrays, which stay resident beside the copy."""
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd.band import band_order
    n, P = 4096, 9
    A = sc.tridiagonal(n)
    rng = np.random.default_rng(41)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    shift = 0.1 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3)
    out = []
    for method in (0, 1):
        c = Context(0)
        try:
            c.spmm_set_method(method)
            c.set_matrix_csr(A)
            assert _plan_agrees(c, A, 0) == ((SELL, SELL) if method else (ROWS, ROWS))
            c.band_prepare(band_order(A)[0])
            c.pop_reserve(P)
            c.pop_put(POP_X, list(range(P)), X)
            st = c.band_solve(list(range(P)), shift, psi, 0)
            out.append((st, c.pop_get(POP_W, list(range(P)), n)))
        finally:
            c.close()
    assert not out[0][0].any()
    _same(out[0], out[1])
    H = A - sp.diags(shift[0] - psi[0] + np.zeros(n))
    assert np.linalg.norm(H @ out[1][1][0] - X[0]) <= 1e-10 * np.linalg.norm(X[0])
