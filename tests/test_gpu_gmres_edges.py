"""Batched device GMRES at its edge paths, size boundaries and batch shapes (GPU box only).

The cases, their references and the checkers are tests/gmres_cases.py; tests/test_gmres_cases_host.py has already shown on
the CPU that SciPy and the oracle's restatement agree on every case, that no case has a decision within 1 % of its threshold
(so the inner counts can be demanded equal), and that the checkers reject planted errors.  DESIGN section 4 maps every edge
path of csrc/gmres.hip to the test here that reaches it."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as gc
import scenarios
from fake_ctx import FakeContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


_got = {}


def _run(ctx, name):
    """One device run per case and module, shared by the tests that look at it."""
    if name not in _got:
        _got[name] = gc.run_case(ctx, gc.BY_NAME[name])
    return _got[name]


@pytest.mark.parametrize("name", [c["name"] for c in gc.EXACT])
def test_exact_cases_bit_for_bit(ctx, name):
    """Breakdown at column 0, complete stagnation with every rotation in the f == 0 branch and the last in g == 0 (R = n < 20,
    R = 20, exhaustion after 4 cycles), the zero-pivot rule with f = g = 0, x0 = b already a solution, b = 0: through the zgemm,
    the dense GEMV and the SpMM product; SciPy's x bit for bit, its info and inner count, status 0."""
    gc.check_case(gc.BY_NAME[name], _run(ctx, name))


@pytest.mark.parametrize("name", [c["name"] for c in gc.ROUNDED])
def test_rounded_cases(ctx, name):
    """Both sides of every size at which another post kernel is launched (CSR, one and several cycles, with and without Jacobi),
    the dense shared matrix at 1024 / 1025, restart 1, 2, 5, 19, maxiter = 1, n < 20, right-hand sides scaled by 1e+-120."""
    gc.check_case(gc.BY_NAME[name], _run(ctx, name))


def test_scaled_right_hand_sides_give_the_scaled_iterate(ctx):
    X0, info0, inner0, _ = _run(ctx, "restart19_n64")              # the same system, restart 19: 19 iterations in one cycle
    for name, f in (("scale_up_n64", 1e120), ("scale_down_n64", 1e-120)):
        X, info, inner, status = _run(ctx, name)
        assert (info[0], inner[0], status[0]) == (0, 19, 0), (name, info, inner, status)
        assert inner0[0] == 19 and np.linalg.norm(X[0] / f - X0[0]) <= 1e-9 * np.linalg.norm(X0[0]), name


@pytest.mark.parametrize("name", [c["name"] for c in gc.ONE_CYCLE_CASES])
def test_one_cycle_is_the_krylov_minimiser(ctx, name):
    """rtol = 0, maxiter = 1, restart = m: after m steps x minimises ||M (b - H x)|| over x0 + K_m; the reference is a twice
    reorthogonalised basis and lstsq, the bound 64 x the restatement's own deviation from it.  Worst device / restatement ratio
    seen on an MI355X: DESIGN section 4."""
    case = gc.BY_NAME[name]
    got = _run(ctx, name)
    gc.check_case(case, got)
    ratio, own = gc.check_one_cycle(case, got)
    print(f"{name}: restatement {own:.2e} from the minimiser, device / restatement {ratio:.2f}")


@pytest.mark.parametrize("name", [c["name"] for c in gc.DENSE_TAILS])
def test_dense_mode_tails_and_shared_mode_agree(ctx, name):
    """maus_gmres_pert with PERT_NONE (materialised H_k, gemv_dense_kernel) at n that are no multiple of 16 or 64, three
    candidates with their own shift, psi and Jacobi: against the restatement, and the iterate against the shared-matrix mode
    on the same inputs to 1e-12."""
    case = gc.BY_NAME[name]
    got = _run(ctx, name)
    gc.check_case(case, got)
    X2, info2, inner2, status2 = gc.run_case(ctx, dict(case, mode="shared"))
    assert np.array_equal(info2, got[1]) and np.array_equal(inner2, got[2]) and (status2 == 0).all()
    for i in range(X2.shape[0]):
        assert np.linalg.norm(X2[i] - got[0][i]) <= 1e-12 * np.linalg.norm(X2[i]), (name, i)


def _pert_alone_and_together(ctx, A, B, shift, psi, jac, **kw):
    k, n = B.shape
    ctx.set_matrix(A)
    ctx.pop_reserve(k)
    slots = list(range(k))
    ctx.pop_put(0, slots, B)
    info, inner, status, used = ctx.gmres_pert(slots, shift, psi, 0, jac, 0, None, **kw)
    X = ctx.pop_get(2, slots, n)
    for i in range(k):
        i1, n1, s1, u1 = ctx.gmres_pert([i], shift[[i]], psi[[i]], 0, jac[[i]], 0, None, **kw)
        x1 = ctx.pop_get(2, [i], n)[0]
        assert (i1[0], n1[0], s1[0], u1[0]) == (info[i], inner[i], status[i], used[i]), i
        assert gc.same_bits(x1, X[i]), i
    return X, info, inner, status


def test_dense_mode_in_chunks_of_the_lu_workspace(monkeypatch):
    """count = workspace capacity + 6 (MAUS_LU_BATCH = 64): the chunk loop of maus_gmres_pert runs twice; every candidate is
    bit-identical to its run alone, and three of the second chunk are checked against the restatement."""
    from adaptive_matrix_solver_amd import Context
    monkeypatch.setenv("MAUS_LU_BATCH", "64")
    c = Context(0)
    try:
        n, k = 65, 70
        A = gc.spread(n, 77)
        B = gc.crand(78, k, n)
        rng = np.random.default_rng(79)
        shift = (rng.standard_normal(k) + 1j * rng.standard_normal(k)) * 0.2
        psi = 10.0 ** rng.uniform(-9, -3, k)
        jac = (np.arange(k) % 3 != 0).astype(np.int32)
        assert c.lu_reserve(n, k) == 64
        X, info, inner, status = _pert_alone_and_together(c, A, B, shift, psi, jac)
        assert (status == 0).all() and (info == 0).all()
        for i in (64, 66, 69):
            H = gc.dense_h(A, shift[i], psi[i])
            ref = gc.traced(H, B[i], B[i], (1.0 / np.diag(H)) if jac[i] else None)
            if ref[4] >= gc.GUARD:
                assert inner[i] == ref[2], (i, inner[i], ref[2])
            assert np.linalg.norm(X[i] - ref[0]) <= 1e-9 * np.linalg.norm(ref[0]), i
    finally:
        c.close()


def _linear_batch(P):
    n = 96
    A, b = scenarios.wide_diag_system(n, 4321, decades=2.0)
    rng = np.random.default_rng(100 + P)
    psi = 10.0 ** rng.uniform(-19, -12, P)
    jac = (np.arange(P) % 2).astype(np.int32)
    return A, b, np.zeros(P, dtype=np.complex128), psi, jac


def _solve_linear(ctx, order, shift, psi, jac, n, maxiter=6):
    """Candidates `order` (indices into shift / psi / jac) as one rhs_mode = 1 batch in that order -> X, info, inner, status."""
    order = np.asarray(order)
    slots = list(range(len(order)))
    ctx.pop_reserve(len(order))
    info, inner, status = ctx.gmres(slots, shift[order], psi[order], 1, jac[order], maxiter=maxiter)
    return ctx.pop_get(2, slots, n), info, inner, status


def _differences(X, X1):
    """(candidates whose bits differ, largest relative distance) between two sets of iterates."""
    rel = [np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(X, X1)]
    return sum(not gc.same_bits(a, b) for a, b in zip(X, X1)), max(rel)


@pytest.mark.parametrize("P", [33, 34, 65])
def test_linear_batch_equals_each_candidate_alone(ctx, P):
    """rhs_mode = 1 around the batch size (34) from which the first product is 33 rows of the zgemm and a broadcast
    (bcast_row_kernel): per-candidate psi and alternating Jacobi let the candidates finish at different ticks; x, info and inner
    of every candidate bit-identical to its run alone.

    The product kernel the zgemm launcher picks depends on the number of rows (4M kernels up to 32 rows, the DMA-staged 3M
    kernel above, for n a multiple of 8 and >= 64 as here), and 3M and 4M round differently: maus_gmres_run pads a product of
    fewer than 33 rows to 33, so a candidate alone and in any batch is multiplied by the same kernel.  Without the padding all
    33 / 34 / 65 iterates differed from the run alone, by up to 3.2e-14 relative (info and inner were equal)."""
    A, b, shift, psi, jac = _linear_batch(P)
    n = A.shape[0]
    ctx.set_matrix(A)
    ctx.set_rhs(b)
    X, info, inner, status = _solve_linear(ctx, np.arange(P), shift, psi, jac, n)
    assert (status == 0).all() and len(set(inner.tolist())) > 1 and (info[jac == 1] == 0).all()
    alone = [_solve_linear(ctx, [i], shift, psi, jac, n) for i in range(P)]
    for i in range(P):
        assert (alone[i][1][0], alone[i][2][0], alone[i][3][0]) == (info[i], inner[i], 0), (i, alone[i][1:], info[i], inner[i])
    ndiff, worst = _differences(X, [a[0][0] for a in alone])
    print(f"linear batch P = {P}: {ndiff} of {P} iterates differ from the run alone, at most {worst:.2e} relative")
    assert ndiff == 0, (ndiff, worst)


@pytest.mark.parametrize("P", [33, 34, 65])
def test_linear_batch_does_not_depend_on_the_order(ctx, P):
    """The same batch in reverse order: the candidates whose first product was computed (positions 0 .. 32) and those that
    received the broadcast copy change places, every tick has the same number of active rows and therefore the same product
    kernel -- every candidate bit for bit the same.  Against the run alone: info and inner equal, x within 1e-9; and the first
    two candidates against the restatement."""
    A, b, shift, psi, jac = _linear_batch(P)
    n = A.shape[0]
    ctx.set_matrix(A)
    ctx.set_rhs(b)
    X, info, inner, status = _solve_linear(ctx, np.arange(P), shift, psi, jac, n)
    Xr, info_r, inner_r, status_r = _solve_linear(ctx, np.arange(P)[::-1], shift, psi, jac, n)
    assert np.array_equal(info, info_r[::-1]) and np.array_equal(inner, inner_r[::-1]) and (status == 0).all() and (status_r == 0).all()
    assert _differences(X, Xr[::-1])[0] == 0
    for i in range(P):
        x1, i1, n1, s1 = _solve_linear(ctx, [i], shift, psi, jac, n)
        assert (i1[0], n1[0], s1[0]) == (info[i], inner[i], 0), i
        if info[i] == 0:
            assert np.linalg.norm(x1[0] - X[i]) <= 1e-9 * np.linalg.norm(x1[0]), i
    for i in (0, 1):
        H = gc.dense_h(A, 0.0, psi[i])
        ref = gc.traced(H, b, b, (1.0 / np.diag(H)) if jac[i] else None, maxiter=6)
        assert info[i] == ref[1], (i, info[i], ref[1])
        if ref[1] == 0:
            assert np.linalg.norm(X[i] - ref[0]) <= 1e-9 * np.linalg.norm(ref[0]), i


@pytest.mark.parametrize("P", [33, 34, 65])
def test_linear_batch_as_csr_equals_each_candidate_alone(ctx, P):
    """The same systems with the matrix stored as CSR: a row of the SpMM product does not depend on the other rows, so here the
    demand of test_linear_batch_equals_each_candidate_alone holds as it stands -- x, info, inner bit-identical alone and in the
    batch.  Compaction, the per-candidate state machine and the finish kernel contribute no dependence on the batch."""
    A, b, shift, psi, jac = _linear_batch(P)
    n = A.shape[0]
    ctx.set_matrix_csr(sp.csr_matrix(A))
    ctx.set_rhs(b)
    X, info, inner, status = _solve_linear(ctx, np.arange(P), shift, psi, jac, n)
    assert (status == 0).all() and len(set(inner.tolist())) > 1
    for i in range(P):
        x1, i1, n1, s1 = _solve_linear(ctx, [i], shift, psi, jac, n)
        assert (i1[0], n1[0], s1[0]) == (info[i], inner[i], 0), i
        assert gc.same_bits(x1[0], X[i]), i


def _solve_batch(ctx, order, B, shift, psi, jac):
    order = np.asarray(order)
    slots = list(range(len(order)))
    ctx.pop_reserve(len(order))
    ctx.pop_put(0, slots, B[order])
    info, inner, status = ctx.gmres(slots, shift[order], psi[order], 0, jac[order])
    return ctx.pop_get(2, slots, B.shape[1]), info, inner, status


def test_batch_of_1100_candidates(ctx):
    """rhs_mode = 0, 1100 candidates at n = 64: the compaction kernel's second pass (candidates 1024 ..), its wave and
    64-candidate boundaries, and every 37th candidate breaking down at column 0 while its neighbours run on.  Ten candidates
    against the restatement (the four that break down: bit for bit); the batch in reverse order (candidates 0 .. 75 and
    1024 .. 1099 change places) bit for bit the same; candidates 0, 63, 64, 1023, 1024, 1099 alone: info, inner, x to 1e-9;
    and the same batch with the matrix as CSR bit-identical to those six alone."""
    A, B, shift, psi, jac = gc.batch_system()
    P, n = B.shape
    ctx.set_matrix(A)
    X, info, inner, status = _solve_batch(ctx, np.arange(P), B, shift, psi, jac)
    assert (status == 0).all() and (info == 0).all()
    assert (inner[::37] == 1).all() and (np.delete(inner, np.arange(0, P, 37)) > 5).all()
    for i in gc.BATCH_RESTATED:
        H = gc.dense_h(A, shift[i], psi[i])
        ref = gc.traced(H, B[i], B[i], (1.0 / np.diag(H)) if jac[i] else None)
        got = (X[i], info[i], inner[i], status[i])
        if i % 37 == 0:
            gc.check_exact(got, ref, f"batch[{i}]")
        else:
            gc.check_rounded(got, ref, H, B[i], 1e-8, f"batch[{i}]")
    Xr, info_r, inner_r, status_r = _solve_batch(ctx, np.arange(P)[::-1], B, shift, psi, jac)
    assert np.array_equal(info, info_r[::-1]) and np.array_equal(inner, inner_r[::-1]) and (status_r == 0).all()
    assert _differences(X, Xr[::-1])[0] == 0
    for i in gc.BATCH_ALONE:
        x1, i1, n1, s1 = _solve_batch(ctx, [i], B, shift, psi, jac)
        assert (i1[0], n1[0], s1[0]) == (info[i], inner[i], 0), i
        assert np.linalg.norm(x1[0] - X[i]) <= 1e-9 * np.linalg.norm(x1[0]), i
    ctx.set_matrix_csr(sp.csr_matrix(A))
    Xs, info_s, inner_s, status_s = _solve_batch(ctx, np.arange(P), B, shift, psi, jac)
    assert np.array_equal(info_s, info) and np.array_equal(inner_s, inner) and (status_s == 0).all()
    for i in gc.BATCH_ALONE:
        x1, i1, n1, s1 = _solve_batch(ctx, [i], B, shift, psi, jac)
        assert (i1[0], n1[0], s1[0]) == (info_s[i], inner_s[i], 0), i
        assert gc.same_bits(x1[0], Xs[i]), i


def test_batch_of_1100_candidates_equals_runs_alone(ctx):
    """Candidates 0, 63, 64, 1023, 1024 and 1099 of the 1100-candidate batch (dense shared matrix) bit-identical to their runs
    alone.

    Holds through the padded product of test_linear_batch_equals_each_candidate_alone (n = 64 takes the 3M kernel too);
    without it 5 of the 6 iterates differed, by up to 1.2e-15 relative."""
    A, B, shift, psi, jac = gc.batch_system()
    P, n = B.shape
    ctx.set_matrix(A)
    X, info, inner, status = _solve_batch(ctx, np.arange(P), B, shift, psi, jac)
    alone = [_solve_batch(ctx, [i], B, shift, psi, jac) for i in gc.BATCH_ALONE]
    for i, a in zip(gc.BATCH_ALONE, alone):
        assert (a[1][0], a[2][0], a[3][0]) == (info[i], inner[i], 0), i
    ndiff, worst = _differences(X[list(gc.BATCH_ALONE)], [a[0][0] for a in alone])
    print(f"batch of 1100: {ndiff} of {len(gc.BATCH_ALONE)} iterates differ from the run alone, at most {worst:.2e} relative")
    assert gc.same_bits(alone[0][0][0], X[0])
    assert ndiff == 0, (ndiff, worst)


def _gate_matrices():
    """(A, [(shift, psi, expected)]) at n = 300: past the first 256 entries of jacobi_check_kernel's stride loop."""
    n = 300
    base = gc.spread(n, 5)
    out = []
    A = base.copy(); A[299, 299] = 0.0
    out.append((A, [(0j, 0.0, False), (0j, 1e-3, True)]))                          # a zero entry at the end / repaired by psi
    A = base.copy(); A[256, 256] = 0.0
    out.append((A, [(0j, 0.0, False), (0j, 1e-3, True)]))                          # the first entry of the second pass
    A = base.copy(); A[299, 299] = 1e-12
    out.append((A, [(0j, 0.0, False)]))                                            # |d| = 1e-12 exactly: the test is `>`
    A = base.copy(); A[299, 299] = 1.0000001e-12
    out.append((A, [(0j, 0.0, True)]))
    A = base.copy(); A[270, 270] = 1e-310
    out.append((A, [(0j, 0.0, False)]))                                            # subnormal: the reciprocal overflows
    A = base.copy(); A[257, 257] = complex(np.nan, 0.0)
    out.append((A, [(0j, 0.0, False), (0j, 1e-3, False)]))
    last = base[299, 299]
    out.append((base, [(0j, 0.0, True), (last, 0.0, False), (last, 1e-3, True), (base[0, 0], 0.0, False)]))
    return out


def test_jacobi_gate_thresholds_and_late_entries(ctx):
    """maus_jacobi_check against FakeContext.jacobi_check and the stated outcomes, and the same gate read back through
    jacobi_out of maus_gmres_pert (jacobi_gate_dense_kernel on the materialised H_k)."""
    fake = FakeContext()
    for A, rows in _gate_matrices():
        n = A.shape[0]
        shift = np.array([r[0] for r in rows], dtype=np.complex128)
        psi = np.array([r[1] for r in rows], dtype=np.float64)
        want = [r[2] for r in rows]
        fake.set_matrix(A)
        assert list(fake.jacobi_check(shift, psi)) == want
        ctx.set_matrix(A)
        assert list(ctx.jacobi_check(shift, psi)) == want
        k = len(rows)
        ctx.pop_reserve(k)
        ctx.pop_put(0, list(range(k)), gc.crand(9, k, n))
        ones = np.ones(k, dtype=np.int32)
        _, _, _, used = ctx.gmres_pert(list(range(k)), shift, psi, 0, ones, 0, None, restart=1, maxiter=1)
        assert list(used) == want
        _, _, _, used = ctx.gmres_pert(list(range(k)), shift, psi, 0, 0 * ones, 0, None, restart=1, maxiter=1)
        assert not used.any()                                                   # never without being asked for


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_non_finite_data_is_reported_as_not_converged(ctx, form):
    """Data, not a fault: a NaN in one candidate's right-hand side, an Inf in the matrix.  maus_gmres ends with info = maxiter
    and status 0 (what SciPy reports after maxiter cycles of NaN; the inner count is not compared: the device stops at once),
    never info = 0 with a non-finite x, and the neighbour with finite data is solved."""
    n = 300
    A = gc.spread(n, 3, 0.5 / np.sqrt(n))
    b = gc.crand(4, n)
    bad = b.copy()
    bad[n - 1] = complex(1.0, np.nan)

    def bind(M):
        if form == "csr":
            ctx.set_matrix_csr(sp.csr_matrix(M))
        else:
            ctx.set_matrix(M)
        ctx.pop_reserve(3)
        ctx.pop_put(0, [0, 1, 2], np.stack([b, bad, b]))

    z3 = np.zeros(3, dtype=np.complex128)
    for jac in (0, 1):
        bind(A)
        info, inner, status = ctx.gmres([0, 1, 2], z3, np.zeros(3), 0, np.full(3, jac, dtype=np.int32), maxiter=7)
        X = ctx.pop_get(2, [0, 1, 2], n)
        assert list(info) == [0, 7, 0] and list(status) == [0, 0, 0] and inner[1] == 0, (info, inner, status)
        assert np.isfinite(X[[0, 2]].view(np.float64)).all() and gc.same_bits(X[0], X[2])
        Ainf = A.copy()
        Ainf[5, 7] = np.inf
        bind(Ainf)
        info, inner, status = ctx.gmres([0, 1, 2], z3, np.zeros(3), 0, np.full(3, jac, dtype=np.int32), maxiter=7)
        assert list(info) == [7, 7, 7] and list(status) == [0, 0, 0], (info, status)
    if form == "dense":
        # maus_gmres_pert scans H_k and the right-hand side (AMS:94 analogue): status -1 for the candidate with the NaN only
        bind(A)
        info, inner, status, used = ctx.gmres_pert([0, 1, 2], z3, np.full(3, 1e-6), 0, np.zeros(3, dtype=np.int32), 0, None, maxiter=7)
        assert list(status) == [0, -1, 0] and info[0] == 0 and info[2] == 0, (info, status)
        # and the double of the shared-matrix mode agrees with the device about it
        fake = FakeContext()
        fake.set_matrix(A)
        fake.pop_reserve(3)
        fake.pop_put(0, [0, 1, 2], np.stack([b, bad, b]))
        finfo, _, fstatus = fake.gmres([0, 1, 2], z3, np.zeros(3), 0, np.zeros(3, dtype=np.int32), maxiter=7)
        assert list(finfo) == [0, 7, 0] and list(fstatus) == [0, 0, 0]


@pytest.mark.parametrize("restart", [0, -3, 21, 50])
def test_restart_outside_1_to_20_is_an_error(ctx, restart):
    """The Krylov basis holds 20 vectors; a larger restart used to run restart = 20 silently."""
    from adaptive_matrix_solver_amd._cabi import MausHipError
    n = 40
    A = gc.spread(n, 3)
    b = gc.crand(1, n)
    ctx.set_matrix(A)
    ctx.pop_reserve(1)
    ctx.pop_put(0, [0], b)
    args = ([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 0, np.zeros(1, dtype=np.int32))
    with pytest.raises(MausHipError, match="between 1 and 20"):
        ctx.gmres(*args, restart=restart)
    with pytest.raises(MausHipError, match="between 1 and 20"):
        ctx.gmres_pert(*args, 0, None, restart=restart)
    info, inner, status = ctx.gmres(*args, restart=20)                          # the context is still good
    ref = gc.traced(A, b, b, None)
    assert (info[0], inner[0], status[0]) == (ref[1], ref[2], 0)
