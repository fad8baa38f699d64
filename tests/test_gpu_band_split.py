"""The split band solve (sparse_split="on", maus_band_set_split, csrc/band.hip) on the device: backward error against LAPACK on
the column-reordered matrix and the pivot rows of the NumPy model (tests/split_cases.py) at the smallest legal partition on
every side of 2, 3 and 5 partitions, the shifted Toeplitz family, planted zero columns, NaN, batches and chunked workspaces,
the CSR path, the solvers, and the switch: off is the method alone, on leaves every band out of range alone."""
import os
import random

import numpy as np
import pytest
import scipy.linalg.lapack as lapack
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import split_cases as sc
from adaptive_matrix_solver_amd import _cabi
from adaptive_matrix_solver_amd.band import band_order, runs_split, split_len, split_shape
from test_gpu_band import _bind, _ctx
from test_gpu_band_tiled import _same_bits
from test_gpu_step_parity import TOL_VEC

pytestmark = pytest.mark.gpu

COLUMN, BLOCKED, TILED, WIDE, NARROW = (_cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE, _cabi.BAND_NARROW)
RATIOS = {}                                                             # (kl, ku) -> largest omega_dev / max(omega_model, eps) seen


def _split_lu(ctx, ab, b, kl, ku, m, method=NARROW):
    """band_lu under `method` with the split on at partition length m (0: the rule); the switch is off again afterwards."""
    ctx.band_set_split(True, m)
    try:
        return ctx.band_lu(ab, b, kl, ku, method=method)
    finally:
        ctx.band_set_split(False, 0)


def _check(ctx, H, ab, b, kl, ku, m, method, tag, pivots=True):
    """One system: status 0, omega_dev <= 8 max(omega_model, eps) with LAPACK on H[:, Q] as the model, and the model's pivot
    rows wherever its choice had a margin.  Returns omega_dev."""
    n = H.shape[0]
    mm = m or split_len(n, kl, ku)
    assert runs_split(n, kl, ku, m)
    x, ipiv, st = _split_lu(ctx, ab[None], b[None], kl, ku, m, method)
    assert st[0] == 0, (tag, st)
    om, om_ref = sc.omega(H, x[0], b), sc.model_omega(H, b, kl, ku, mm)
    ratio = om / max(om_ref, sc.EPS)
    RATIOS[(kl, ku)] = max(RATIOS.get((kl, ku), 0.0), ratio)
    print(f"{tag}: omega_dev {om:.3g}, LAPACK on H[:, Q] {om_ref:.3g}, ratio {ratio:.3g}")
    assert om <= 8 * max(om_ref, sc.EPS), (tag, om, om_ref)
    if not pivots:
        return om
    _, st_m, piv, sure = sc.split_reference(ab, b, kl, ku, mm)
    assert st_m == 0
    assert np.array_equal(ipiv[0][sure], piv[sure]), (tag, np.flatnonzero((ipiv[0] != piv) & sure)[:10])
    return om


@pytest.mark.parametrize("kl,ku", sc.SHAPES)
def test_split_smallest_partition_on_every_side(kl, ku):
    """part_len = 2 w + 2, where every step touches a partition edge: n = p m - 1, p m, p m + 1 for p = 2, 3, 5 -- a last
    partition of length 1 (shorter than w) among them -- and n = 700 with the rule's own length."""
    ctx = _ctx()
    w = kl + ku
    m = 2 * w + 2
    for p in (2, 3, 5):
        for n in (p * m - 1, p * m, p * m + 1):
            H, ab, b = sc.band_case(n, kl, ku, 1000 * p + n)
            _check(ctx, H, ab, b, kl, ku, m, NARROW, f"({kl},{ku}) n={n} m={m}")
    H, ab, b = sc.band_case(700, kl, ku, 77)
    assert split_shape(700, kl, ku)[0] >= 3
    _check(ctx, H, ab, b, kl, ku, 0, NARROW, f"({kl},{ku}) n=700 rule m={split_len(700, kl, ku)}")
    print(f"({kl},{ku}): largest omega_dev / max(omega_model, eps) = {RATIOS[(kl, ku)]:.3g}")


@pytest.mark.parametrize("method", [COLUMN, BLOCKED, TILED, WIDE])
def test_split_reduced_system_under_every_method(method):
    """The reduced system runs the plan of the context's method: kl_red = 44 (blocked, tiled, and tiled under wide) and 3."""
    ctx = _ctx()
    for kl, ku, n in ((15, 15, 5 * 62 + 9), (1, 1, 333)):
        m = 2 * (kl + ku) + 2
        _, _, klr, kur = split_shape(n, kl, ku, m)
        kind = _cabi.band_plan(method, 10, klr, kur)[0]
        assert kind == ({BLOCKED: BLOCKED, TILED: TILED, WIDE: TILED}.get(method, COLUMN) if klr >= 16 else COLUMN)
        H, ab, b = sc.band_case(n, kl, ku, 5 + method)
        _check(ctx, H, ab, b, kl, ku, m, method, f"method {method} ({kl},{ku}) n={n}")


def test_split_shifted_toeplitz():
    """kl = ku = 15, n = 700, shifted onto an eigenvalue to 1e-9: the family whose element growth differs most from zgbtrf's
    in the CPU model.  The bound is the model's; narrow's omega on the same system is printed beside it."""
    ctx = _ctx()
    H, ab, b = sc.toeplitz_shifted(700, 15)
    xn, _, stn = ctx.band_lu(ab[None], b[None], 15, 15, method=NARROW)
    assert stn[0] == 0
    for m in (0, 62, 100):
        om = _check(ctx, H, ab, b, 15, 15, m, NARROW, f"toeplitz m={m or split_len(700, 15, 15)}", pivots=False)
        print(f"toeplitz m={m}: omega split {om:.3g}, narrow {sc.omega(H, xn[0], b):.3g}")


@pytest.mark.parametrize("kl,ku,n", [(2, 2, 100), (0, 4, 61), (4, 0, 61), (1, 1, 40), (15, 15, 200), (7, 24, 400)])
def test_split_planted_zero_columns(kl, ku, n):
    """Zero columns in an interior, in a separator, first, last and several at once: zgbtrf's info, and the regular systems of
    the batch keep the bits of their lone solves."""
    ctx = _ctx()
    w = kl + ku
    m = 2 * w + 2
    sets = [(), (m + 1,), (m - 1,), (0,), (n - 1,), (), (2 * m + 3, m - w, n - 2)]
    cases = [sc.band_case(n, kl, ku, 31 + k, zero_cols=z) for k, z in enumerate(sets)]
    AB, B = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    x, _, st = _split_lu(ctx, AB, B, kl, ku, m)
    for k, z in enumerate(sets):
        info = lapack.zgbtrf(AB[k], kl, ku)[2]
        assert info == (min(z) + 1 if z else 0)
        assert st[k] == info, (k, z, st[k], info)
    for k in (0, 5):
        x1, _, st1 = _split_lu(ctx, AB[k][None], B[k][None], kl, ku, m)
        assert st1[0] == 0 and _same_bits(x1[0], x[k])
        assert sc.omega(cases[k][0], x[k], B[k]) <= 8 * max(sc.model_omega(cases[k][0], B[k], kl, ku, m), sc.EPS)


def test_split_nan_is_its_own_systems():
    ctx = _ctx()
    kl, ku, n, m = 2, 2, 95, 10
    cases = [sc.band_case(n, kl, ku, 50 + k) for k in range(4)]
    AB, B = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    x0, _, st0 = _split_lu(ctx, AB, B, kl, ku, m)
    assert (st0 == 0).all()
    AB2, B2 = AB.copy(), B.copy()
    AB2[1, kl + ku, 37] = np.nan                                         # a diagonal entry of an interior
    B2[3, 58] = np.inf                                                   # a right-hand side entry
    x, _, st = _split_lu(ctx, AB2, B2, kl, ku, m)
    assert list(st) == [0, -1, 0, -1]
    assert _same_bits(x[[0, 2]], x0[[0, 2]])


def test_split_rows_do_not_depend_on_the_batch():
    """70 shifted systems of one operator through maus_band_solve with the split on: a NaN shift and an exactly singular one
    among them; every row equals its lone solve and the row of a workspace of 16 (balanced chunks)."""
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
    shift[23], psi[23] = 2.5 + 0.5j, 0.0                                # (a - lam) + psi = 0 exactly: column k0 is zero
    shift[55] = np.nan
    slots = np.arange(P)
    assert split_len(n, 1, 1) == 64 and k0 % 64 < 62                     # an interior column

    def fresh():
        c = _ctx()
        c.band_set_method(NARROW)
        c.band_set_split(True, 0)
        perm, kl, ku = _bind(c, A, P)
        assert (kl, ku) == (1, 1) and np.array_equal(perm, np.arange(n))
        c.pop_put(_cabi.POP_X, slots, X)
        c.pop_put(_cabi.POP_W, slots, np.zeros((P, n), dtype=np.complex128))
        return c

    ctx = fresh()
    ctx.profile_enable(True)
    st = ctx.band_solve(slots, shift, psi, 0)
    prof = ctx.profile_read()
    ctx.profile_enable(False)
    assert prof["band_split"]["launches"] > 0 and prof["band_split"]["flops"] > 0 and prof["band_split"]["bytes"] > 0
    assert prof["band"]["launches"] == 0
    assert st[55] == -1 and st[23] == k0 + 1
    keep = [s for s in range(P) if s not in (23, 55)]
    assert (st[keep] == 0).all()
    W = ctx.pop_get(_cabi.POP_W, slots, n)
    assert np.isfinite(W[keep]).all()
    I = sp.identity(n, format="csr", dtype=np.complex128)
    for s in (0, 69):
        H = (A - shift[s] * I + psi[s] * I).toarray()
        assert sc.omega(H, W[s], X[s]) <= 8 * max(sc.model_omega(H, X[s], 1, 1, 64), sc.EPS)
    lone = fresh()
    for s in (0, 22, 23, 24, 54, 55, 56, 69):
        st1 = lone.band_solve([s], shift[[s]], psi[[s]], 0)
        assert st1[0] == st[s]
        assert _same_bits(lone.pop_get(_cabi.POP_W, [s], n)[0], W[s]), s
    os.environ["MAUS_BAND_BATCH"] = "16"
    try:
        c2 = fresh()
        assert c2.band_reserve(P) == 16
        st2 = c2.band_solve(slots, shift, psi, 0)                       # five chunks of 14
        assert c2.band_workspace_allocations() == 1
    finally:
        del os.environ["MAUS_BAND_BATCH"]
    assert np.array_equal(st2, st) and _same_bits(c2.pop_get(_cabi.POP_W, slots, n), W)


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


def _kappa_inf(H):
    """Varah's bound for a strictly row diagonally dominant H, as tests/test_gpu_band_narrow.py derives it from the matrix."""
    d = np.abs(H.diagonal())
    rows = np.asarray(abs(H).sum(axis=1)).ravel()
    gap = (2.0 * d - rows).min()
    assert gap > 0.5
    return rows.max() / gap


@pytest.mark.parametrize("which,rhs_mode", [("tri", 0), ("tri", 1), ("penta", 0), ("penta", 1)])
def test_split_band_solve_path(which, rhs_mode):
    """maus_band_solve on a permuted 1-D operator: the ordering, the build kernel, slots and the inverse permutation."""
    ctx = _ctx()
    n, P = 3000, 5
    A = _shuffled(_diagonals(n, 1 if which == "tri" else 2, 31), 32)
    ctx.band_set_method(NARROW)
    ctx.band_set_split(True, 0)
    perm, kl, ku = _bind(ctx, A, P)
    assert not np.array_equal(perm, np.arange(n)) and runs_split(n, kl, ku)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
    bvec = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ctx.pop_put(_cabi.POP_X, np.arange(P), X)
    ctx.set_rhs(bvec)
    shift = 0.3 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3)
    slots = np.array([3, 0, 4, 1, 2])
    assert (ctx.band_solve(slots, shift, psi, rhs_mode) == 0).all()
    W = ctx.pop_get(_cabi.POP_W, slots, n)
    I = sp.identity(n, format="csr", dtype=np.complex128)
    for k in range(P):
        H = (A - shift[k] * I + psi[k] * I).tocsc()
        xr = spla.spsolve(H, X[slots[k]] if rhs_mode == 0 else bvec)
        err = np.linalg.norm(W[k] - xr) / np.linalg.norm(xr)
        assert err <= 1e-12 * _kappa_inf(H), (k, err)


def _solver_run(A, b, kind, split, iters=2):
    """`iters` loop bodies of MAUS_Solver on a real DeviceEngine under sparse_direct='narrow'; scipy-legacy: every solve direct."""
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    ptype = ProblemType.EIGENVALUE if kind == "eig" else ProblemType.SOLVE_LINEAR_SYSTEM
    s = MAUS_Solver(A, ptype, b_vector=b if kind == "lin" else None, initial_num_candidates=6, quiet=True, gmres_compat="scipy-legacy",
                    sparse_mode="device", sparse_direct="narrow", sparse_split=split, diag_info=diag)
    s.engine.ctx.profile_enable(True)
    rows = []
    for it in range(iters):
        s.loop_body(it + 1)
        rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                     np.random.get_state()[2], np.random.get_state()[1].copy(), random.getstate()))
    prof = s.engine.ctx.profile_read()
    s.engine.ctx.profile_enable(False)
    vecs = [np.array(c.v_k if kind == "eig" else c.x_k) for c in s.candidates]
    return s, rows, vecs, prof


@pytest.mark.parametrize("kind", ["eig", "lin"])
def test_split_solver_loop_bodies(kind):
    """Every candidate-step is compared (none left out): the bookkeeping and both random streams of sparse_split='off', the
    vectors to the tolerance of the step-parity comparisons."""
    A = _diagonals(600, 1, 41)
    n = A.shape[0]
    b = np.random.default_rng(42).standard_normal(n) + 0j
    s0, rows0, vecs0, prof0 = _solver_run(A, b, kind, "off")
    s1, rows1, vecs1, prof1 = _solver_run(A, b, kind, "on")
    assert s1.engine._band and s1.engine.ctx.band_split() == (True, 0) and s0.engine.ctx.band_split() == (False, 0)
    assert prof1["band_split"]["launches"] > 0 and prof1["band"]["launches"] == 0
    assert prof0["band_split"]["launches"] == 0 and prof0["band"]["launches"] > 0
    for (r_rows, r_pos, r_key, r_py), (g_rows, g_pos, g_key, g_py) in zip(rows0, rows1):
        assert r_rows == g_rows
        assert r_pos == g_pos and np.array_equal(r_key, g_key) and r_py == g_py
    assert len(vecs0) == len(vecs1)
    for v0, v1 in zip(vecs0, vecs1):
        n0, n1 = np.linalg.norm(v0), np.linalg.norm(v1)
        assert abs(n0 - n1) <= TOL_VEC * max(n0, 1e-300)
        assert np.linalg.norm(v0 - v1) <= TOL_VEC * n0


def test_split_inverse_iterate_solver():
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    _ctx()
    A = _shuffled(_diagonals(3000, 2, 31), 32)
    n = A.shape[0]
    b = np.random.default_rng(5).standard_normal(n) + 0j
    x, tries = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="narrow", sparse_split="on").solve(A, b, 0)
    ctx = InverseIterateSolver._ctx()
    assert tries == 0 and ctx.band_split() == (True, 0)
    xb, tries = InverseIterateSolver(n, 1e-20, 3, is_sparse=True, sparse_mode="device", sparse_direct="narrow").solve(A, b, 0)
    assert tries == 0 and ctx.band_split() == (False, 0)                 # the next solver asks for the method alone again
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b)
    assert np.linalg.norm(x - xb) <= 1e-12 * _kappa_inf(A.tocsr()) * np.linalg.norm(xb)


def test_split_switch_and_rule():
    """Off is the method alone, bit for bit; on, a band out of range (kl = 16, kl + ku = 32, w = 0, n below two partitions)
    runs the method's own kernel with its bits; bad values are refused and change nothing."""
    ctx = _ctx()
    never = _ctx()                                                       # a context whose switch was never touched
    assert ctx.band_split() == (False, 0)
    for kl, ku, n in ((1, 1, 300), (3, 2, 257), (15, 15, 400)):
        _, ab, b = sc.band_case(n, kl, ku, 9)
        xs, _, _ = _split_lu(ctx, ab[None], b[None], kl, ku, 0)          # on, then off again
        x0, p0, s0 = ctx.band_lu(ab[None], b[None], kl, ku, method=NARROW)
        x1, p1, s1 = never.band_lu(ab[None], b[None], kl, ku, method=NARROW)
        assert _same_bits(x0, x1) and np.array_equal(p0, p1) and np.array_equal(s0, s1)
        assert np.array_equal(p0[0], lapack.zgbtrf(ab, kl, ku)[1])
        assert not _same_bits(xs, x0)                                    # the split did run: another pivot order
    for kl, ku, n, m in ((16, 3, 500, 0), (15, 17, 500, 0), (0, 0, 500, 0), (2, 2, 64, 0), (2, 2, 40, 40), (16, 15, 300, 8)):
        assert not runs_split(n, kl, ku, m if kl + ku <= 31 and kl <= 15 else 0)
        _, ab, b = sc.band_case(n, kl, ku, 10)
        for method in (NARROW, TILED):
            ctx.profile_enable(True)
            xs, ps, ss = _split_lu(ctx, ab[None], b[None], kl, ku, m, method)
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            assert prof["band_split"]["launches"] == 0
            x0, p0, s0 = never.band_lu(ab[None], b[None], kl, ku, method=method)
            assert _same_bits(xs, x0) and np.array_equal(ps, p0) and np.array_equal(ss, s0)
    ctx.band_set_split(True, 77)
    for bad in ((2, 0), (-1, 0), (1, -1)):
        with pytest.raises(_cabi.MausHipError):
            ctx.band_set_split(*bad)
        assert ctx.band_split() == (True, 77)
    _, ab, b = sc.band_case(300, 15, 15, 11)
    ctx.band_set_split(True, 61)                                         # below 2 w + 2 = 62: refused where it is used
    with pytest.raises(_cabi.MausHipError, match="partition length"):
        ctx.band_lu(ab[None], b[None], 15, 15, method=NARROW)
    ctx.band_set_split(False, 0)
    with pytest.raises(_cabi.MausHipError):                             # the method table is what it was
        ctx.band_set_method(16)
