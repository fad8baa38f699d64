"""The streaming band LU for narrow bands (sparse_direct="narrow", maus_band_set_method(ctx, 8), csrc/band.hip) on the device:
the rule, the bits of the column kernel and LAPACK's pivots on every side of the ring and chunk boundaries, batches and
chunked workspaces, the CSR path, n = 2^20, and the solvers."""
import os
import random

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order, runs_narrow
from test_gpu_band import _band_case, _bind, _ctx
from test_gpu_band_tiled import _same_bits

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED, TILED, WIDE = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE
NARROW = getattr(_cabi, "BAND_NARROW", None)             # None without the feature: every test below then fails in its first call

# (kl, ku): tridiagonal, pentadiagonal, one-sided, kl != ku, kv = 31 three ways (7 + 24, 15 + 16, 1 + 30), kl = ku = 15, diagonal
SHAPES = [(1, 1), (2, 2), (0, 4), (4, 0), (3, 2), (7, 24), (15, 15), (15, 16), (1, 30), (0, 0)]
# every side of the chunk (16), of the three resident chunks (48) and of the ring (64); n < kl + ku + 1; several turns of the ring
SIZES = [1, 5, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 129, 700]
CORNERS_IN = [(0, 0), (1, 1), (15, 15), (15, 16), (1, 30), (0, 31)]
CORNERS_OUT = [(16, 1), (15, 17), (0, 32)]


def test_narrow_rule():
    ctx = _ctx()
    ctx.band_set_method(NARROW)
    assert ctx.band_method() == NARROW == 8
    for kl, ku in CORNERS_IN:
        assert runs_narrow(kl, ku)
        for n in (1, 40, 1 << 20):
            assert ctx.band_kernel_for(n, kl, ku) == (NARROW, 1), (kl, ku)
            assert ctx.band_outer_nb(n, kl, ku) == 0
    for kl, ku in CORNERS_OUT + [(100, 5), (2000, 5)]:
        assert not runs_narrow(kl, ku)
        assert ctx.band_kernel_for(5000, kl, ku) == (COLUMN, 1), (kl, ku)
        assert ctx.band_outer_nb(5000, kl, ku) == 0
    for bad in (3, 5, 6, 7, 9, 16, -1):
        with pytest.raises(_cabi.MausHipError):
            ctx.band_set_method(bad)
        assert ctx.band_method() == NARROW
    for m in (COLUMN, BLOCKED, TILED, WIDE):                            # below kl = 16 the other methods run what they ran
        ctx.band_set_method(m)
        for kl, ku in CORNERS_IN + [(15, 40)]:
            assert ctx.band_kernel_for(5000, kl, ku) == (COLUMN, 1), (m, kl, ku)
    ctx.band_set_method(TILED)
    assert ctx.band_kernel_for(3000, 100, 5) == (TILED, 16)
    with pytest.raises(_cabi.MausHipError):
        ctx.band_set_method(3)
    assert ctx.band_method() == TILED


def _compare(ctx, A, ab, b, kl, ku, tag):
    """One system under the narrow method against the column kernel (bits) and LAPACK (pivots, info, x within the contract
    of test_band_lu_matches_zgbtrf)."""
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)
    xn, pn, sn = ctx.band_lu(ab[None], b[None], kl, ku, method=NARROW)
    xc, pc, sc = ctx.band_lu(ab[None], b[None], kl, ku, method=COLUMN)
    assert np.array_equal(pn[0], piv), (tag, np.flatnonzero(pn[0] != piv)[:10])
    assert sn[0] == info, (tag, sn[0], info)
    assert np.array_equal(pn, pc) and np.array_equal(sn, sc), tag
    assert _same_bits(xn, xc), (tag, np.flatnonzero(xn[0] != xc[0])[:10])
    if info == 0:
        xr, _ = lapack.zgbtrs(lu, kl, ku, b, piv)
        cond = np.linalg.cond(A)
        err = np.linalg.norm(xn[0] - xr)
        print(f"{tag}: cond {cond:.3g}, |x - xr| / |xr| = {err / np.linalg.norm(xr):.3g}")
        assert err <= 1e-12 * cond * np.linalg.norm(xr), tag
    return info


@pytest.mark.parametrize("kl,ku", SHAPES)
def test_narrow_gives_the_bits_of_the_column_kernel_and_lapacks_pivots(kl, ku):
    ctx = _ctx()
    ctx.band_set_method(NARROW)
    assert ctx.band_kernel_for(700, kl, ku) == (NARROW, 1)
    ctx.band_set_method(COLUMN)
    for n in SIZES:
        A, ab, b = _band_case(n, kl, ku, 7 + n + kl)
        assert _compare(ctx, A, ab, b, kl, ku, f"n={n} kl={kl} ku={ku}") == 0
    assert ctx.band_method() == COLUMN                                  # method= holds for the one call


@pytest.mark.parametrize("kl,ku", [(1, 1), (3, 2), (15, 16), (0, 4)])
@pytest.mark.parametrize("where", ["first", "chunk_end", "chunk_start", "ring_edge", "last", "several"])
def test_narrow_zero_pivot_columns(kl, ku, where):
    """An exactly singular column at column 0, on both sides of a chunk edge, at the ring's edge and at n - 1: info names the
    first one, the steps after it go on as the column kernel's do."""
    ctx = _ctx()
    n = 81
    cols = {"first": (0,), "chunk_end": (15,), "chunk_start": (16,), "ring_edge": (64,), "last": (n - 1,),
            "several": (0, 16, 47, 48, n - 1)}[where]
    A, ab, b = _band_case(n, kl, ku, 11 + kl, zero_cols=cols)
    assert _compare(ctx, A, ab, b, kl, ku, f"{where} kl={kl} ku={ku}") == cols[0] + 1


def test_narrow_ignores_what_lies_outside_the_matrix():
    """Fill rows with anything in them are zeroed as zgbtf2 zeroes them; the corners above row 0 are never used."""
    ctx = _ctx()
    kl, ku, n = 3, 4, 70
    M, ab, b = _band_case(n, kl, ku, 5)
    xc, pc, sc = ctx.band_lu(ab[None], b[None], kl, ku, method=COLUMN)
    ab[:kl, :] = 1e300 + 3j                              # the fill rows: workspace on entry
    ab[kl, 0] = np.nan                                   # row kl of column 0 lies above the matrix
    xn, pn, sn = ctx.band_lu(ab[None], b[None], kl, ku, method=NARROW)
    assert sn[0] == 0 and np.array_equal(pn, pc)
    assert _same_bits(xn, xc)


def test_narrow_batch_by_band_lu():
    """70 different systems of one shape in one call: one with a NaN (status -1, its neighbours untouched), one singular;
    each equals its own lone solve and the column kernel's batch bit for bit."""
    ctx = _ctx()
    n, kl, ku, G = 130, 3, 2, 70
    cases = [_band_case(n, kl, ku, 100 + s, zero_cols=(33,) if s == 41 else ()) for s in range(G)]
    ab = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    ab[17, kl + ku, 50] = np.nan
    xn, pn, sn = ctx.band_lu(ab, b, kl, ku, method=NARROW)
    xc, pc, sc = ctx.band_lu(ab, b, kl, ku, method=COLUMN)
    assert sn[17] == -1 and sn[41] == 34
    keep = [g for g in range(G) if g not in (17, 41)]
    assert (sn[keep] == 0).all() and np.isfinite(xn[keep]).all()
    assert np.array_equal(sn, sc) and np.array_equal(pn, pc) and _same_bits(xn, xc)
    for g in range(G):
        x1, p1, s1 = ctx.band_lu(ab[g][None], b[g][None], kl, ku, method=NARROW)
        assert s1[0] == sn[g] and np.array_equal(p1[0], pn[g]) and _same_bits(x1[0], xn[g]), g
    for g in (0, 16, 18, 69):
        assert np.linalg.norm(cases[g][0] @ xn[g] - b[g]) <= 1e-11 * np.linalg.norm(b[g]) * np.linalg.cond(cases[g][0])


def _shuffled(A, seed):
    p = np.random.default_rng(seed).permutation(A.shape[0])
    return A[p][:, p].tocsr()


def _diagonals(n, kd, seed):
    """Non-Hermitian complex operator with kd sub- and superdiagonals of modulus <= 1 / kd and a diagonal near 4 + i."""
    rng = np.random.default_rng(seed)
    ds, offs = [], []
    for d in range(-kd, kd + 1):
        m = n - abs(d)
        if d == 0:
            ds.append(4.0 + 1j + 0.1 * rng.standard_normal(n))
        else:
            ds.append(rng.uniform(0.2, 1.0, m) / kd * np.exp(2j * np.pi * rng.random(m)))
        offs.append(d)
    return sp.diags(ds, offs, format="csr")


_OPS = {}


def _operator(which):
    """Shuffled tridiagonal / pentadiagonal operator at n = 20000, built once."""
    if which not in _OPS:
        _OPS[which] = _shuffled(_diagonals(20000, 1 if which == "tri" else 2, 31), 32)
    return _OPS[which]


def _kappa_inf(H):
    """Upper bound on cond_inf of a strictly row diagonally dominant sparse H: |H^-1|_inf <= 1 / min_i(|h_ii| - sum_{j != i}
    |h_ij|) (Varah), so kappa_inf <= |H|_inf / that gap.  Derived from the matrix, not from a solve."""
    d = np.abs(H.diagonal())
    rows = np.asarray(abs(H).sum(axis=1)).ravel()
    gap = (2.0 * d - rows).min()
    assert gap > 0.5
    return rows.max() / gap


@pytest.mark.parametrize("which", ["tri", "penta"])
def test_narrow_band_solve_path(which):
    ctx = _ctx()
    A = _operator(which)
    n, P = A.shape[0], 40
    perm, kl, ku = _bind(ctx, A, P)
    assert not np.array_equal(perm, np.arange(n))                       # the ordering had work to do
    assert runs_narrow(kl, ku) and kl >= (1 if which == "tri" else 2)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    shift = 0.3 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3)
    slots = np.arange(P)
    assert ctx.band_kernel_for(n, kl, ku) == (COLUMN, 1)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    Wc = ctx.pop_get(_cabi.POP_W, slots, n)
    allocs = ctx.band_workspace_allocations()
    ctx.band_set_method(NARROW)
    assert ctx.band_kernel_for(n, kl, ku) == (NARROW, 1)
    ctx.profile_enable(True)
    assert (ctx.band_solve(slots, shift, psi, 0) == 0).all()
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert prof["band"]["launches"] > 0 and prof["band"]["flops"] > 0 and prof["band"]["bytes"] > 0
    assert all(prof[k]["launches"] == 0 for k in ("band_blocked", "band_tiled", "band_wide"))
    Wn = ctx.pop_get(_cabi.POP_W, slots, n)
    assert _same_bits(Wn, Wc), np.flatnonzero((Wn != Wc).any(axis=1))
    assert ctx.band_workspace_allocations() == allocs                   # the column kernel's workspace, as it is
    ctx.band_set_method(COLUMN)
    assert (ctx.band_solve(slots[:3], shift[:3], psi[:3], 0) == 0).all()
    assert ctx.band_workspace_allocations() == allocs
    I = sp.identity(n, format="csr", dtype=np.complex128)
    for k in (0, 17, 39):
        H = (A - shift[k] * I + psi[k] * I).tocsc()
        cond = _kappa_inf(H)
        xr = spla.spsolve(H, X[k])
        err = np.linalg.norm(Wn[k] - xr) / np.linalg.norm(xr)
        print(f"{which} k={k}: kl={kl} ku={ku} kappa_inf <= {cond:.3g}, |x - xr| / |xr| = {err:.3g}")
        assert err <= 1e-12 * cond


def test_narrow_rows_do_not_depend_on_the_batch():
    """70 shifted systems of one operator through maus_band_solve: a NaN shift (status -1) and an exactly singular one among
    them; every row equals its lone solve, the column kernel's row, and the row of a workspace of 16 (balanced chunks)."""
    n, P, k0 = 600, 70, 300
    rng = np.random.default_rng(8)
    lo, di, up = (rng.standard_normal(n - 1) + 0j, 4.0 + 1j + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1) * 1j)
    lo[[k0 - 1, k0]] = 0; up[[k0 - 1, k0]] = 0                           # row and column k0 hold the diagonal entry alone
    di[k0] = 2.5 + 0.5j
    A = sp.diags([lo, di, up], [-1, 0, 1], format="csr")
    A.eliminate_zeros()
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    shift = 0.3 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3)
    shift[23], psi[23] = 2.5 + 0.5j, 0.0                                # (a - lam) + psi = 0 exactly: singular at k0
    shift[55] = np.nan
    slots = np.arange(P)

    def fresh(method):
        c = _ctx()
        c.band_set_method(method)
        perm, kl, ku = _bind(c, A, P)
        assert (kl, ku) == (1, 1) and np.array_equal(perm, np.arange(n))
        c.pop_put(_cabi.POP_X, slots, X)
        c.pop_put(_cabi.POP_W, slots, np.zeros((P, n), dtype=np.complex128))
        return c

    ctx = fresh(NARROW)
    st = ctx.band_solve(slots, shift, psi, 0)
    assert st[55] == -1 and st[23] == k0 + 1
    keep = [s for s in range(P) if s not in (23, 55)]
    assert (st[keep] == 0).all()
    W = ctx.pop_get(_cabi.POP_W, slots, n)
    assert np.isfinite(W[keep]).all()
    cc = fresh(COLUMN)
    stc = cc.band_solve(slots, shift, psi, 0)
    assert np.array_equal(st, stc) and _same_bits(W, cc.pop_get(_cabi.POP_W, slots, n))
    lone = fresh(NARROW)
    for s in (0, 22, 23, 24, 54, 55, 56, 69):
        st1 = lone.band_solve([s], shift[[s]], psi[[s]], 0)
        assert st1[0] == st[s]
        assert _same_bits(lone.pop_get(_cabi.POP_W, [s], n)[0], W[s]), s
    os.environ["MAUS_BAND_BATCH"] = "16"
    try:
        c2 = fresh(NARROW)
        assert c2.band_reserve(P) == 16
        st2 = c2.band_solve(slots, shift, psi, 0)                       # five chunks of 14
        assert c2.band_workspace_allocations() == 1
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert np.array_equal(st2, st) and _same_bits(c2.pop_get(_cabi.POP_W, slots, n), W)


def test_narrow_tridiagonal_2_pow_20():
    """One lone tridiagonal solve at n = 2^20 against host zgbtrf / zgbtrs.  The operator is strictly diagonally dominant by
    rows (|a_ii| >= 4, two off-diagonal entries of modulus <= 1), so |A^-1|_inf <= 1 / min_i(|a_ii| - sum_{j != i} |a_ij|)
    (Varah) and kappa_inf <= |A|_inf / that gap: the bound on |x - xr| / |xr| is 1e-12 times a number derived from the matrix."""
    ctx = _ctx()
    n, kl, ku = 1 << 20, 1, 1
    rng = np.random.default_rng(11)
    ab = np.zeros((4, n), dtype=np.complex128)
    ab[1, 1:] = rng.uniform(0.1, 1.0, n - 1) * np.exp(2j * np.pi * rng.random(n - 1))          # superdiagonal: A[j - 1, j]
    ab[2, :] = rng.uniform(4.0, 5.0, n) * np.exp(2j * np.pi * rng.random(n))
    ab[3, :-1] = rng.uniform(0.1, 1.0, n - 1) * np.exp(2j * np.pi * rng.random(n - 1))         # subdiagonal: A[j + 1, j]
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    off = np.zeros(n)                                                   # sum over the row of |a_ij|, j != i
    off[:-1] += np.abs(ab[1, 1:])
    off[1:] += np.abs(ab[3, :-1])
    gap = (np.abs(ab[2]) - off).min()
    assert np.abs(ab[2]).min() >= 4.0 and gap >= 2.0
    kappa = (np.abs(ab[2]) + off).max() / gap
    lu, piv, info = lapack.zgbtrf(ab, kl, ku)
    xr, _ = lapack.zgbtrs(lu, kl, ku, b, piv)
    x, ipiv, st = ctx.band_lu(ab[None], b[None], kl, ku, method=NARROW)
    assert st[0] == info == 0
    assert np.array_equal(ipiv[0], piv)
    err = np.linalg.norm(x[0] - xr) / np.linalg.norm(xr)
    print(f"n = 2^20: kappa_inf <= {kappa:.3g}, |x - xr| / |xr| = {err:.3g}")
    assert err <= 1e-12 * kappa


def test_narrow_widest_band_65536_against_the_column_kernel():
    ctx = _ctx()
    n, kl, ku = 65536, 15, 15
    rng = np.random.default_rng(12)
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    ab[kl:] = rng.standard_normal((kl + ku + 1, n)) + 1j * rng.standard_normal((kl + ku + 1, n))
    ab[kl + ku] *= 3.0                                                  # pivots move, but not at every column
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xn, pn, sn = ctx.band_lu(ab[None], b[None], kl, ku, method=NARROW)
    xc, pc, sc = ctx.band_lu(ab[None], b[None], kl, ku, method=COLUMN)
    assert sn[0] == sc[0] == 0
    moved = int((pn[0] != np.arange(n)).sum())
    assert 0 < moved < n
    assert np.array_equal(pn, pc), np.flatnonzero(pn[0] != pc[0])[:10]
    assert _same_bits(xn, xc), np.flatnonzero(xn[0] != xc[0])[:10]


def _solver_run(A, b, kind, mode, iters=2):
    """`iters` loop bodies of MAUS_Solver on a real DeviceEngine under sparse_direct=mode; scipy-legacy: every solve direct."""
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    eng = DeviceEngine(gmres_compat="scipy-legacy", sparse_mode="device", sparse_direct=mode)
    ptype = ProblemType.EIGENVALUE if kind == "eig" else ProblemType.SOLVE_LINEAR_SYSTEM
    s = MAUS_Solver(A, ptype, b_vector=b if kind == "lin" else None, initial_num_candidates=6, quiet=True,
                    sparse_mode="device", diag_info=diag, engine=eng)
    eng.ctx.profile_enable(True)
    rows = []
    for it in range(iters):
        s.loop_body(it + 1)
        rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                     np.random.get_state()[2], np.random.get_state()[1].copy(), random.getstate()))
    prof = eng.ctx.profile_read()
    eng.ctx.profile_enable(False)
    vecs = [np.array(c.v_k if kind == "eig" else c.x_k) for c in s.candidates]
    lams = [complex(c.lambda_k) if kind == "eig" and c.lambda_k is not None else 0j for c in s.candidates]
    return s, rows, vecs, lams, prof


@pytest.mark.parametrize("kind", ["eig", "lin"])
def test_narrow_solver_loop_bodies_equal_band(kind):
    A = _diagonals(20000, 1, 41)
    n = A.shape[0]
    b = np.random.default_rng(42).standard_normal(n) + 0j
    sb, rows_b, vecs_b, lams_b, prof_b = _solver_run(A, b, kind, "band")
    sn, rows_n, vecs_n, lams_n, prof_n = _solver_run(A, b, kind, "narrow")
    assert sb.engine._band and sb.engine.ctx.band_method() == COLUMN
    assert sn.engine._band and sn.engine.ctx.band_method() == NARROW
    perm, kl, ku = sn.engine.band_shape(sn.M)
    assert (kl, ku) == (1, 1) and sn.engine.ctx.band_kernel_for(n, kl, ku) == (NARROW, 1)
    for (r_rows, r_pos, r_key, r_py), (g_rows, g_pos, g_key, g_py) in zip(rows_b, rows_n):
        assert r_rows == g_rows
        assert r_pos == g_pos and np.array_equal(r_key, g_key)          # NumPy's stream ...
        assert r_py == g_py                                             # ... and Python's
    assert len(vecs_b) == len(vecs_n) and lams_b == lams_n
    for vb, vn in zip(vecs_b, vecs_n):
        assert _same_bits(vb, vn)
    assert prof_n["band"]["launches"] > 0 and prof_b["band"]["launches"] > 0
    assert all(prof_n[k]["launches"] == 0 for k in ("band_blocked", "band_tiled", "band_wide"))


def test_inverse_iterate_solver_narrow():
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    _ctx()
    A = _operator("penta")
    n = A.shape[0]
    b = np.random.default_rng(5).standard_normal(n) + 0j
    x, tries = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="narrow").solve(A, b, 0)
    ctx = InverseIterateSolver._ctx()
    assert tries == 0 and ctx.band_method() == NARROW
    xb, tries = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="band").solve(A, b, 0)
    assert tries == 0 and ctx.band_method() == COLUMN                   # the next solver asks for the column kernel again
    assert _same_bits(x, xb)
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b)
