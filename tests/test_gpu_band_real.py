"""Band solves in real arithmetic (real_direct="on", maus_band_set_real; csrc/band.hip, DESIGN §11 "Band solves in real
arithmetic") on the device: the real path against the complex path of the same context under numpy.array_equal -- x, ipiv and
status -- for the column kernel, the narrow method and the split, on every side of the chunk, window, ring and partition edges.

No test claims equality before it has seen the real path run: maus_band_real_plan says so for a band_solve call, and for every
call the profile class band_real has counted launches while band, band_split and the other band classes have counted none (and
the other way round for the complex run).  W is filled with NaN before every band_solve, so a solve that wrote nothing cannot
pass.  Where a system is singular or its solution overflows, status and ipiv are compared and x is not: past a zero pivot the
complex path holds NaN (Smith's 0 / 0) where the real path may hold Inf (1 / 0), which the ABI comment states."""
import os
import random

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp

import band_real_cases as brc
import real_cases as rc
import split_cases as sc
from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order, runs_split, split_len

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED, NARROW = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_NARROW
COMPLEX_CLASSES = ("band", "band_split", "band_blocked", "band_tiled", "band_wide")
# tests/test_gpu_band_narrow.py's: every side of the chunk (16), of the three resident chunks (48) and of the ring (64)
SHAPES = [(1, 1), (2, 2), (0, 4), (4, 0), (3, 2), (7, 24), (15, 15), (15, 16), (1, 30), (0, 0)]
SIZES = [1, 5, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 129, 700]


@pytest.fixture
def ctx():
    c = _cabi.Context(0)
    yield c
    c.close()


def _counted(prof, real, tag=""):
    """The classes of the path that ran have counted launches and bytes, those of the other path nothing."""
    mine = sum(prof[k]["launches"] for k in (("band_real",) if real else COMPLEX_CLASSES))
    other = sum(prof[k]["launches"] for k in (COMPLEX_CLASSES if real else ("band_real",)))
    assert mine > 0 and other == 0, (tag, real, {k: prof[k]["launches"] for k in COMPLEX_CLASSES + ("band_real",)})
    if real:
        assert prof["band_real"]["bytes"] > 0 and prof["band_real"]["flops"] >= 0


def _lu(ctx, ab, b, kl, ku, real, method, split=None):
    """band_lu under (mode, method, split: None or the partition length, 0 for the rule) -> (x, ipiv, status); the switches are
    off again afterwards."""
    ab, b = np.asarray(ab), np.asarray(b)
    if ab.ndim == 2:
        ab, b = ab[None], b[None]
    ctx.band_set_real(1 if real else 0)
    ctx.band_set_split(split is not None, split or 0)
    ctx.profile_enable(True)
    try:
        out = ctx.band_lu(ab, b, kl, ku, method=method)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
        ctx.band_set_split(False, 0)
        ctx.band_set_real(0)
    _counted(prof, real, (kl, ku, ab.shape, method, split))
    return out


def _same_lu(r, c, tag):
    """The real run against the complex run: ipiv and status equal; x equal with imaginary bits +0.0 where the status is 0."""
    (xr, pr, sr), (xc, pc, stc) = r, c
    assert np.array_equal(sr, stc), (tag, sr, stc)
    assert np.array_equal(pr, pc), (tag, np.argwhere(pr != pc)[:5])
    ok = stc == 0
    assert np.all(np.isfinite(xc[ok])), tag
    assert np.array_equal(xr[ok], xc[ok]), (tag, int(np.sum(xr[ok] != xc[ok])))
    assert brc.imag_bits_zero(xr[ok]), (tag, "the real path leaves imaginary parts of +0.0")
    return stc


def _pair_lu(ctx, ab, b, kl, ku, method, split=None, tag=""):
    r = _lu(ctx, ab, b, kl, ku, True, method, split)
    c = _lu(ctx, ab, b, kl, ku, False, method, split)
    _same_lu(r, c, tag)
    return r


def _dgbtrf(ab, kl, ku):
    _, piv, info = lapack.dgbtrf(np.ascontiguousarray(ab.real), kl, ku)
    return piv, info


# ---- 1. band_lu, real against complex of the same context ---------------------------------------------------------------------
@pytest.mark.parametrize("method", [NARROW, COLUMN], ids=["narrow", "column"])
@pytest.mark.parametrize("kl,ku", SHAPES)
def test_band_lu_real_equals_complex_and_dgbtrf_pivots(ctx, kl, ku, method):
    assert ctx.band_real() == 0
    for n in SIZES:
        _, ab, b = brc.band_case(n, kl, ku, 7 + n + kl)
        x, ipiv, st = _pair_lu(ctx, ab, b, kl, ku, method, tag=f"({kl},{ku}) n={n}")
        piv, info = _dgbtrf(ab, kl, ku)
        assert max(st[0], 0) == info == 0 and np.array_equal(ipiv[0], piv), (n, st, info)   # st -2: a solution that overflowed


@pytest.mark.parametrize("kl,ku", [(16, 1), (40, 3), (100, 5)])
def test_band_lu_column_kernel_above_the_narrow_range(ctx, kl, ku):
    for method in (COLUMN, NARROW):                                     # narrow's plan falls back to the column kernel here
        assert _cabi.band_real_kinds(method, False, 0, 300, kl, ku) == (True, COLUMN, False)
    for n in (130, 300):
        _, ab, b = brc.band_case(n, kl, ku, 7 + n + kl)
        x, ipiv, st = _pair_lu(ctx, ab, b, kl, ku, COLUMN, tag=f"({kl},{ku}) n={n}")
        piv, info = _dgbtrf(ab, kl, ku)
        assert st[0] == info == 0 and np.array_equal(ipiv[0], piv)


def test_band_lu_runs_complex_where_the_rule_fails(ctx):
    """Mode 1 with an imaginary part somewhere in ab or b (the fill rows count), or under a method without real kernels: the
    complex path, counted as complex.  -0.0 imaginary parts count as real."""
    kl, ku, n = 3, 2, 70
    _, ab, b = brc.band_case(n, kl, ku, 5)
    ctx.band_set_real(1)

    def run(ab_, b_, method, kl_=kl, ku_=ku):
        ctx.profile_enable(True)
        try:
            out = ctx.band_lu(ab_[None], b_[None], kl_, ku_, method=method)
            return out, ctx.profile_read()
        finally:
            ctx.profile_enable(False)

    ref, prof = run(ab, b, NARROW)
    _counted(prof, True)
    neg = ab.copy()
    neg.imag = -0.0
    out, prof = run(neg, b, NARROW)
    _counted(prof, True, "-0.0")
    assert np.array_equal(out[0], ref[0])
    for what in ("fill", "entry", "tiny", "nan", "rhs"):
        ab2, b2 = ab.copy(), b.copy()
        if what == "fill":
            ab2[0, 5] = 1j
        elif what == "entry":
            ab2[kl + ku, 9] += 1j
        elif what == "tiny":
            ab2.view(np.float64).reshape(ab2.shape + (2,))[kl + ku, 9, 1] = 5e-324
        elif what == "nan":
            ab2.view(np.float64).reshape(ab2.shape + (2,))[1, 9, 1] = np.nan       # a fill row: workspace
        else:
            b2[3] += 1e-3j
        out, prof = run(ab2, b2, NARROW)
        _counted(prof, False, what)
        if what in ("fill", "nan"):                            # the same system: the complex path's x is the real path's
            assert np.array_equal(out[0].real, ref[0].real) and np.array_equal(out[1], ref[1]), what
    _, ab25, b25 = brc.band_case(130, 25, 3, 6)
    out, prof = run(ab25, b25, BLOCKED, 25, 3)
    _counted(prof, False, "blocked")
    ctx.band_set_real(0)
    with pytest.raises(_cabi.MausHipError, match="maus_band_set_real"):
        ctx.band_set_real(2)
    assert ctx.band_real() == 0


# ---- 2. zero pivots -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [NARROW, COLUMN], ids=["narrow", "column"])
@pytest.mark.parametrize("kl,ku", [(1, 1), (3, 2), (15, 16), (0, 4)])
def test_zero_pivot_columns(ctx, kl, ku, method):
    n = 81
    for cols in ((0,), (15,), (16,), (64,), (n - 1,), (15, 16, 64)):
        _, ab, b = brc.band_case(n, kl, ku, 11, zero_cols=cols)
        x, ipiv, st = _pair_lu(ctx, ab, b, kl, ku, method, tag=f"({kl},{ku}) zero {cols}")
        piv, info = _dgbtrf(ab, kl, ku)
        assert st[0] == info == cols[0] + 1                             # info names the first ...
        assert np.array_equal(ipiv[0], piv)                             # ... and the steps after it go on as LAPACK's


# ---- 3. the split -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [NARROW, COLUMN], ids=["narrow", "column"])
@pytest.mark.parametrize("kl,ku", sc.SHAPES + [(4, 5)])                # (4, 5): 2 w + 2 = 20, the group of 32 lanes
def test_split_real_equals_complex_split(ctx, kl, ku, method):
    """tests/test_gpu_band_split.py's table with real parts: the smallest legal partition with n one above it (a last partition
    of one column), at and beside 3 and 5 partitions, a forced length of 64 with a short last partition, the rule at n = 700.
    The complex split's own tests hold it against LAPACK; here the real split returns its values."""
    w = kl + ku
    m = 2 * w + 2
    gs = 8 if m <= 8 else 16 if m <= 16 else 32 if m <= 32 else 64
    assert gs == {(1, 1): 8, (2, 2): 16, (0, 4): 16, (4, 0): 16, (3, 2): 16, (4, 5): 32}.get((kl, ku), 64)
    for n, part in [(m + 1, m), (3 * m, m), (5 * m + 1, m), (3 * 64 + 5, 64), (700, 0)]:
        assert runs_split(n, kl, ku, part) and _cabi.band_real_kinds(method, True, part, n, kl, ku)[0::2] == (True, True)
        _, ab, b = brc.split_case(n, kl, ku, 1000 + n)
        x, ipiv, st = _pair_lu(ctx, ab, b, kl, ku, method, split=part, tag=f"({kl},{ku}) n={n} m={part or split_len(n, kl, ku)}")
        assert st[0] == 0


@pytest.mark.parametrize("kl,ku,n", [(2, 2, 100), (1, 1, 40), (15, 15, 200)])
def test_split_zero_pivot_in_an_interior_and_in_a_separator(ctx, kl, ku, n):
    m = 2 * (kl + ku) + 2
    for cols in ((m + 1,), (m - 1,), (2 * m + 3, m - (kl + ku), n - 2)):
        _, ab, b = brc.split_case(n, kl, ku, 31, zero_cols=cols)
        x, ipiv, st = _pair_lu(ctx, ab, b, kl, ku, NARROW, split=m, tag=f"({kl},{ku}) zero {cols}")
        assert st[0] == min(cols) + 1 == lapack.dgbtrf(np.ascontiguousarray(ab.real), kl, ku)[2]


def test_split_reduced_system_without_real_kernels_runs_complex(ctx):
    """(15, 15) split: the reduced system is 44 wide -- the blocked method has no real instantiation, the whole call runs complex."""
    _, ab, b = brc.split_case(5 * 62 + 9, 15, 15, 5)
    assert _cabi.band_real_kinds(BLOCKED, True, 62, 5 * 62 + 9, 15, 15) == (False, COLUMN, True)
    ctx.band_set_real(1)
    ctx.band_set_split(True, 62)
    ctx.profile_enable(True)
    try:
        x, ipiv, st = ctx.band_lu(ab[None], b[None], 15, 15, method=BLOCKED)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
        ctx.band_set_split(False, 0)
        ctx.band_set_real(0)
    _counted(prof, False)
    assert st[0] == 0 and prof["band_split"]["launches"] > 0


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [NARROW, COLUMN], ids=["narrow", "column"])
def test_batch_of_70_by_band_lu(ctx, method):
    """70 systems of one shape in one call: one with a NaN (status -1, its neighbours untouched), one singular; each equals its
    own lone solve and the complex batch."""
    n, kl, ku, G = 130, 3, 2, 70
    cases = [brc.band_case(n, kl, ku, 100 + s, zero_cols=(33,) if s == 41 else ()) for s in range(G)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[17, kl + ku, 50] = np.nan                                        # a real NaN: the imaginary part stays +0.0
    xr, pr, sr = _pair_lu(ctx, ab, b, kl, ku, method, tag="batch")
    assert sr[17] == -1 and sr[41] == 34
    keep = [g for g in range(G) if g not in (17, 41)]
    assert (sr[keep] == 0).all() and np.isfinite(xr[keep]).all()
    for g in range(G):
        x1, p1, s1 = _lu(ctx, ab[g], b[g], kl, ku, True, method)
        assert s1[0] == sr[g] and np.array_equal(p1[0], pr[g]), g
        if sr[g] == 0:
            assert np.array_equal(x1[0], xr[g]), g
    for g in (0, 16, 18, 69):
        assert sc.omega(cases[g][0], xr[g], b[g]) <= 8 * max(sc.omega(cases[g][0], np.linalg.solve(cases[g][0], b[g]), b[g]), sc.EPS)


# ---- 5. band_solve on a CSR-bound matrix --------------------------------------------------------------------------------------
def _bind(ctx, A, b, P, method, split=False):
    ctx.band_set_method(method)
    ctx.band_set_split(split, 0)
    ctx.set_matrix_csr(A)
    perm, kl, ku = band_order(A)
    assert ctx.band_prepare(perm) == (kl, ku)
    ctx.pop_reserve(max(P, 1))
    if b is not None:
        ctx.set_rhs(b)
    ctx.kl_ku = (kl, ku)                                                # for _solve: what the plan's kind is checked against
    return perm, kl, ku


def _solve(ctx, real, shift, psi, rhs_mode=1, why=None):
    """One maus_band_solve call over slots 0 .. P - 1 -> (W rows, status), after the checks of the module docstring.  why: the
    plan's verdict of a call that must run complex although the mode is 1."""
    n = ctx.rows
    shift = np.atleast_1d(np.asarray(shift, dtype=np.complex128))
    P = shift.shape[0]
    psi = np.broadcast_to(np.asarray(psi, dtype=np.float64), (P,)).copy()
    slots = np.arange(P)
    ctx.band_set_real(1 if (real or why is not None) else 0)
    ctx.pop_put(_cabi.POP_W, slots, np.full((P, n), np.nan + 0j))
    plan = ctx.band_real_plan(rhs_mode, shift)
    if real:
        assert plan["real"] and plan["why"] == _cabi.BAND_REAL_OK, plan
    else:
        assert not plan["real"] and plan["why"] == (_cabi.BAND_REAL_MODE_OFF if why is None else why), plan
    assert plan["kind"] == ctx.band_kernel_for(n, *ctx.kl_ku)[0]
    ctx.profile_enable(True)
    try:
        st = ctx.band_solve(slots, shift, psi, rhs_mode)
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    _counted(prof, real, (shift[:3], rhs_mode, why))
    return ctx.pop_get(_cabi.POP_W, slots, n), np.asarray(st)


def _pair_solve(ctx, shift, psi, tag=""):
    xr, sr = _solve(ctx, True, shift, psi)
    xc, stc = _solve(ctx, False, shift, psi)
    assert np.array_equal(sr, stc), (tag, sr, stc)
    ok = stc == 0
    assert np.all(np.isfinite(xc[ok])) and np.array_equal(xr[ok], xc[ok]) and brc.imag_bits_zero(xr[ok]), tag
    return xr, sr


def _pentadiagonal_shuffled(n, seed=3):
    rng = np.random.default_rng(seed)
    d = [rng.standard_normal(n - abs(k)) for k in (-2, -1, 0, 1, 2)]
    d[2] = 4.0 + np.abs(d[2])
    A = sp.diags(d, [-2, -1, 0, 1, 2], format="csr")
    p = rng.permutation(n)
    return rc.real_csr(A[p][:, p].tocsr())


OPERATORS = {
    "tridiagonal_n600": (lambda: rc.tridiagonal(600), NARROW, False),
    "tridiagonal_n600_split": (lambda: rc.tridiagonal(600), NARROW, True),
    "banded_n300": (lambda: rc.banded(300), NARROW, False),
    "pentadiagonal_rcm_n500": (lambda: _pentadiagonal_shuffled(500), NARROW, False),
    "pentadiagonal_rcm_n500_column": (lambda: _pentadiagonal_shuffled(500), COLUMN, False),
    "five_point_n625": (lambda: rc.five_point(25), COLUMN, False),
}


@pytest.mark.parametrize("name", list(OPERATORS))
def test_band_solve_real_shifts_and_psi_per_candidate(ctx, name):
    make, method, split = OPERATORS[name]
    A = make()
    n = A.shape[0]
    b = rc.real_vec(42, n)
    perm, kl, ku = _bind(ctx, A, b, 33, method, split)
    if name.startswith("pentadiagonal"):
        assert not np.array_equal(perm, np.arange(n)) and kl <= 15
    if split:
        assert ctx.band_real_plan(1, np.zeros(1))["split"]
    allocs = None
    for P in (1, 15, 33):
        rng = np.random.default_rng(P)
        shift = 0.2 * rng.standard_normal(P) + 0j
        psi = np.where(np.arange(P) % 2 == 0, 1e-19, 1e-3)
        x, st = _pair_solve(ctx, shift, psi, f"{name} P={P}")
        allocs = ctx.band_workspace_allocations() if allocs is None else allocs
        assert (st == 0).all()
        for k in (0, P // 2, P - 1):
            H = (A - shift[k] * sp.identity(n) + psi[k] * sp.identity(n)).toarray()
            assert sc.omega(H, x[k], b) <= 8 * max(sc.omega(H, np.linalg.solve(H, b), b), sc.EPS), (name, P, k)
    # the same workspace served both paths (P = 1 sized it for one solve; the larger batches grew it once, to the cap)
    assert ctx.band_workspace_allocations() <= allocs + 1
    before = ctx.band_workspace_allocations()
    _pair_solve(ctx, np.full(33, 0.1 + 0j), 1e-3)
    assert ctx.band_workspace_allocations() == before


def test_the_rules_verdicts_one_by_one(ctx):
    A = rc.tridiagonal(600)
    n = 600
    b = rc.real_vec(7, n)
    shift3, psi3 = np.array([0.1, 0.0, -0.2]) + 0j, np.full(3, 1e-3)
    # no ordering: the plan says so (the solve itself is refused as ever)
    ctx.band_set_method(NARROW)
    ctx.band_set_real(1)
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(3)
    ctx.set_rhs(b)
    plan = ctx.band_real_plan(1, shift3)
    assert not plan["real"] and plan["why"] == _cabi.BAND_REAL_NOT_CSR
    with pytest.raises(_cabi.MausHipError, match="no ordering"):
        ctx.band_solve(np.arange(3), shift3, psi3, 1)
    _bind(ctx, A, b, 3, NARROW)
    allocs0 = ctx.band_workspace_allocations()
    ref, st = _solve(ctx, True, shift3, psi3)
    allocs = ctx.band_workspace_allocations()
    assert allocs == allocs0 + 1 and (st == 0).all()
    # mode off
    x, st = _solve(ctx, False, shift3, psi3)
    assert np.array_equal(x, ref)
    # -0.0 imaginary parts count as real
    neg = shift3.copy()
    neg.imag = -0.0
    x, st = _solve(ctx, True, neg, psi3)
    assert np.array_equal(x, ref)
    # one complex shift among three
    _solve(ctx, False, np.array([0.1, 0.0 + 1e-300j, -0.2]), psi3, why=_cabi.BAND_REAL_SHIFT_COMPLEX)
    # population rows as right-hand sides
    ctx.pop_put(_cabi.POP_X, np.arange(3), np.tile(b, (3, 1)))
    x, st = _solve(ctx, False, shift3, psi3, rhs_mode=0, why=_cabi.BAND_REAL_RHS_ROWS)
    assert np.array_equal(x, ref)                                       # the same systems: the complex path's values
    # a complex b (also: the smallest denormal, NaN in an imaginary part)
    tiny, nan = b.copy(), b.copy()
    tiny.view(np.float64)[2 * 7 + 1] = 5e-324
    nan.view(np.float64)[2 * 7 + 1] = np.nan
    for bad in (b + 1j * b, tiny, nan):
        ctx.set_rhs(bad)
        _solve(ctx, False, shift3, psi3, why=_cabi.BAND_REAL_RHS_COMPLEX)
    ctx.set_rhs(b)
    assert ctx.band_workspace_allocations() == allocs                   # switching paths allocates nothing
    # a complex matrix of the same shape
    Ac = A.copy()
    Ac.data[5] += 1e-3j
    _bind(ctx, Ac, b, 3, NARROW)
    _solve(ctx, False, shift3, psi3, why=_cabi.BAND_REAL_MATRIX_COMPLEX)
    # a method without real kernels: blocked at kl = 25
    F = rc.five_point(25)
    _, kl, ku = _bind(ctx, F, rc.real_vec(8, 625), 3, BLOCKED)
    assert kl >= 16 and ctx.band_kernel_for(625, kl, ku)[0] == BLOCKED
    _solve(ctx, False, shift3, psi3, why=_cabi.BAND_REAL_NO_KERNELS)
    ctx.band_set_method(COLUMN)
    _solve(ctx, True, shift3, psi3)


def test_batch_of_70_by_band_solve_and_a_chunked_workspace():
    """70 shifted systems of one operator, a NaN shift (status -1) and an exactly singular one among them: every row equals the
    complex path's, its lone solve, and the row of a workspace of 16 (five balanced chunks of 14)."""
    n, P, k0 = 600, 70, 300
    rng = np.random.default_rng(8)
    lo, di, up = rng.standard_normal(n - 1), 4.0 + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1)
    lo[[k0 - 1, k0]] = 0; up[[k0 - 1, k0]] = 0                           # row and column k0 hold the diagonal entry alone
    di[k0] = 2.5
    A = sp.diags([lo, di, up], [-1, 0, 1], format="csr")
    A.eliminate_zeros()
    A = rc.real_csr(A)
    b = rc.real_vec(9, n)
    shift = 0.3 * rng.standard_normal(P) + 0j
    psi = np.full(P, 1e-3)
    shift[23], psi[23] = 2.5, 0.0                                       # (a - lam) + psi = 0 exactly: singular at k0
    shift[55] = np.nan                                                  # a real NaN: the shift stays flagged real

    def fresh():
        c = _cabi.Context(0)
        _bind(c, A, b, P, NARROW)
        return c

    c1 = fresh()
    try:
        W, st = _pair_solve(c1, shift, psi, "batch")
        assert st[55] == -1 and st[23] == k0 + 1
        keep = [s for s in range(P) if s not in (23, 55)]
        assert (st[keep] == 0).all() and np.isfinite(W[keep]).all()
        for s in (0, 22, 23, 24, 54, 55, 56, 69):
            x1, s1 = _solve(c1, True, shift[[s]], psi[[s]])
            assert s1[0] == st[s]
            if st[s] == 0:
                assert np.array_equal(x1[0], W[s]), s
    finally:
        c1.close()
    os.environ["MAUS_BAND_BATCH"] = "16"
    try:
        c2 = fresh()
        try:
            assert c2.band_reserve(P) == 16
            W2, st2 = _solve(c2, True, shift, psi)
            assert c2.band_workspace_allocations() == 1
        finally:
            c2.close()
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert np.array_equal(st2, st) and np.array_equal(W2[keep], W[keep])


# ---- 6. overflow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,split", [(NARROW, None), (COLUMN, None), (NARROW, 12)], ids=["narrow", "column", "split"])
def test_overflow_gives_status_minus_2_on_both_paths(ctx, method, split):
    """Entries of 1e-200 and a right-hand side of 1e200: the multipliers are O(1), the quotients of the back substitution
    overflow.  x is not compared: Inf - Inf and 0 * Inf differ between the paths, the status does not."""
    _, ab, b = brc.split_case(100, 3, 2, 4)
    ab, b = ab * 1e-200, b * 1e200
    assert brc.imag_bits_zero(ab) and brc.imag_bits_zero(b)
    xr, pr, sr = _lu(ctx, ab, b, 3, 2, True, method, split)
    xc, pc, stc = _lu(ctx, ab, b, 3, 2, False, method, split)
    assert sr[0] == stc[0] == -2 and np.array_equal(pr, pc)
    assert not np.all(np.isfinite(xr)) and not np.all(np.isfinite(xc))


# ---- 7. loop bodies -----------------------------------------------------------------------------------------------------------
def _bodies(A, b, kind, real_direct, bodies=3, **kw):
    """tests/test_gpu_real_arith.py's _bodies with the real_direct keyword: per body the ids, states and counters, the
    residuals and both RNG stream positions; then every device row and the profile."""
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    ptype = ProblemType.EIGENVALUE if kind == "eig" else ProblemType.SOLVE_LINEAR_SYSTEM
    s = MAUS_Solver(A, ptype, b_vector=b if kind == "lin" else None, initial_num_candidates=6, quiet=True,
                    gmres_compat="scipy-legacy", sparse_mode="device", diag_info=diag, real_direct=real_direct, **kw)
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
        mode = ctx.band_real()
    finally:
        ctx.close()
    return rows, dev, prof, mode


def _same_bodies(off, on):
    for (r_rows, r_res, r_pos, r_key, r_py), (g_rows, g_res, g_pos, g_key, g_py) in zip(off[0], on[0]):
        assert r_rows == g_rows
        assert np.array_equal(r_res, g_res, equal_nan=True)
        assert r_pos == g_pos and np.array_equal(r_key, g_key) and r_py == g_py
    for a, b in zip(off[1], on[1]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", ["n20000_narrow_split", "n600_column"])
def test_loop_bodies_of_a_linear_system_under_scipy_legacy(name):
    """gmres_compat="scipy-legacy" sends every solve to the LU: under real_direct="on" those band solves run real and the
    bodies are those of "off"."""
    if name == "n20000_narrow_split":
        A, b, kw, cls = rc.tridiagonal(20000), rc.real_vec(43, 20000), dict(sparse_direct="narrow", sparse_split="on"), "band_split"
    else:
        A, b, kw, cls = rc.tridiagonal(600), rc.real_vec(42, 600), dict(sparse_direct="band"), "band"
    off = _bodies(A, b, "lin", "off", **kw)
    on = _bodies(A, b, "lin", "on", **kw)
    assert (off[3], on[3]) == (0, 1)
    assert on[2]["band_real"]["launches"] > 0 and off[2]["band_real"]["launches"] == 0
    assert off[2][cls]["launches"] == on[2]["band_real"]["launches"]
    assert all(on[2][k]["launches"] == 0 for k in COMPLEX_CLASSES)
    _same_bodies(off, on)


def test_eigenvalue_problem_takes_no_real_band_solve():
    A = rc.tridiagonal(600)
    off = _bodies(A, None, "eig", "off", sparse_direct="band")
    on = _bodies(A, None, "eig", "on", sparse_direct="band")
    assert (off[3], on[3]) == (0, 1)
    assert on[2]["band_real"]["launches"] == 0 and on[2]["band"]["launches"] == off[2]["band"]["launches"] > 0
    _same_bodies(off, on)


# ---- 8. one size run ----------------------------------------------------------------------------------------------------------
def test_tridiagonal_2_pow_20_narrow_and_split(ctx):
    """A lone tridiagonal solve at n = 2^20 under narrow + the split: every index of the real path is computed in elements of
    doubles, none reuses a byte offset of the complex layout."""
    n, kl, ku = 1 << 20, 1, 1
    rng = np.random.default_rng(11)
    ab = np.zeros((4, n), dtype=np.complex128)
    ab[1, 1:] = rng.uniform(0.1, 1.0, n - 1) * rng.choice([-1.0, 1.0], n - 1)
    ab[2, :] = rng.uniform(4.0, 5.0, n) * rng.choice([-1.0, 1.0], n)
    ab[3, :-1] = rng.uniform(0.1, 1.0, n - 1) * rng.choice([-1.0, 1.0], n - 1)
    b = rng.standard_normal(n) + 0j
    assert runs_split(n, kl, ku)
    xr, pr, sr = _lu(ctx, ab, b, kl, ku, True, NARROW, split=0)
    xc, pc, stc = _lu(ctx, ab, b, kl, ku, False, NARROW, split=0)
    assert sr[0] == stc[0] == 0 and np.array_equal(pr, pc)
    assert np.array_equal(xr, xc) and brc.imag_bits_zero(xr) and np.all(np.isfinite(xr))
    # rows strictly diagonally dominant (|a_ii| >= 4, off-diagonal sum <= 2): the residual of a backward-stable solve
    r = ab[2] * xr[0]
    r[:-1] += ab[1, 1:] * xr[0][1:]
    r[1:] += ab[3, :-1] * xr[0][:-1]
    assert np.abs(r - b).max() <= 64 * sc.EPS * (7.0 * np.abs(xr[0]).max() + np.abs(b).max())
