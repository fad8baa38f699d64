"""The device-wide GMRES post step (sparse_gmres="wide", maus_gmres_set_method(ctx, 1), csrc/gmres.hip) on the
device (GPU box only): against the traced restatement of SciPy's gmres on the CSR cases of tests/gmres_cases.py and on the
sizes around one piece and around the second level of the join (tests/gmres_wide_cases.py), a candidate alone against the same
candidate in any batch, order and chunk bit for bit, non-finite data, the method round trip, and MAUS_Solver end to end.

Every test runs under `_wide`: method 1 on a context of its own module, maus_gmres_kernel_for == 2 for the size at hand, and
afterwards the profile class `gmres_wide` has counted launches while `vector` (the class of the register and stream post
kernels; nothing else of maus_gmres on a CSR matrix is counted there) has none -- no test passes with the method silently off."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as gc
import gmres_wide_cases as gw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    c.gmres_set_method(1)
    yield c
    c.close()


@contextlib.contextmanager
def _wide(ctx, n, solves=True):
    ctx.gmres_set_method(1)
    assert ctx.gmres_method() == 1 and ctx.gmres_kernel_for(n, True) == 2
    ctx.profile_enable(True)
    try:
        yield
        prof = ctx.profile_read()
    finally:
        ctx.profile_enable(False)
    if solves:
        assert prof["gmres_wide"]["launches"] > 0 and prof["gmres_wide"]["bytes"] > 0 and prof["gmres_wide"]["flops"] == 0
    assert prof["vector"]["launches"] == 0, "a register / stream post kernel ran under method 1"


def _n_of(case):
    return case["build"]()["B"].shape[1]


# ---- 1. exact cases: SciPy's x bit for bit -------------------------------------------------------------------------------------
EXACT_CSR = [c["name"] for c in gc.EXACT if c["name"].endswith("_csr")]


@pytest.mark.parametrize("name", EXACT_CSR)
def test_exact_csr_cases_bit_for_bit(ctx, name):
    """Complete stagnation with every rotation in the f == 0 branch and the last in g == 0 (R = n < 20, R = 20, exhaustion after
    4 cycles) and the breakdown at column 0 with and without Jacobi, through the state kernel: every intermediate is a small
    dyadic number, so the order of the sums plays no part and x is SciPy's bit for bit."""
    assert len(EXACT_CSR) == 10
    case = gc.BY_NAME[name]
    with _wide(ctx, _n_of(case)):
        got = gc.run_case(ctx, case)
    gc.check_case(case, got)


# ---- 2. rounded cases -----------------------------------------------------------------------------------------------------------
BAND_CSR = [c["name"] for c in gc.ROUNDED if c["name"].startswith("band_n")]


@pytest.mark.parametrize("name", BAND_CSR)
def test_boundary_sizes_of_the_old_table(ctx, name):
    """band_n* at all eleven BOUNDARY_SIZES, both weights, Jacobi 0 / 1: info, inner count, x to 1e-9 and the long-double
    residual, the bounds the stream kernel is held to."""
    assert len(BAND_CSR) == 44
    case = gc.BY_NAME[name]
    assert case["build"]()["csr"]
    with _wide(ctx, _n_of(case)):
        got = gc.run_case(ctx, case)
    gc.check_case(case, got)


@pytest.mark.parametrize("name", [c["name"] for c in gw.CASES])
def test_sizes_around_one_piece_and_around_the_join(ctx, name):
    """n = 511, 512, 513 (one piece of 512 entries and the first entry of a second) and 131071, 131072, 131073 (256 pieces: the
    last n at which every joining thread adds one partial sum, and the first at which thread 0 adds two)."""
    case = gw.BY_NAME[name]
    with _wide(ctx, _n_of(case)):
        got = gc.run_case(ctx, case)
    gw.check_case(case, got)


# ---- 3. restart and cycle edges, small n, trivial exits ------------------------------------------------------------------------
def _csr_twin(name):
    """A dense-matrix case of tests/gmres_cases.py with its matrix wrapped in sp.csr_matrix."""
    case = gc.BY_NAME[name]

    def build():
        d = case["build"]()
        return dict(d, A=sp.csr_matrix(d["A"]), csr=True)
    return dict(case, build=build)


def _check_twin(case, got):
    X, info, inner, status = got
    (H, b, inv), = gc.systems(case)
    ref = gc.traced(H, b, b, inv, rtol=case["rtol"], maxiter=case["maxiter"], restart=case["restart"])
    g = (X[0], info[0], inner[0], status[0])
    if case["exact"]:
        gc.check_exact(g, ref, case["name"])
    else:
        assert ref[4] >= gc.GUARD, (case["name"], ref[4])
        gc.check_rounded(g, ref, H, b, case["rtol"], case["name"])
    if case["expect"] is not None:
        assert (int(info[0]), int(inner[0])) == tuple(case["expect"]), (case["name"], info, inner)
    return ref


EDGES = ([f"restart{R}_n64" for R in (1, 2, 5, 19)] + ["maxiter1_restart4_n64", "scale_up_n64", "scale_down_n64"]
         + [f"small_n{n}_j{j}" for n in (1, 2, 3, 5, 19) for j in (0, 1)] + ["zero_rhs_n33", "x0_solves_n50", "x0_solves_n50_j1"])


@pytest.mark.parametrize("name", EDGES)
def test_restart_cycle_and_size_edges_as_csr(ctx, name):
    """spread(64, 7) as CSR with restart 1, 2, 5, 19 (the cycle ends on col == R - 1, many new cycles through the phase-1
    kernels), restart 4 with maxiter 1 (exhaustion), right-hand sides scaled by 1e+-120; shifted_ginibre at n = 1, 2, 3, 5, 19
    (R = n < 20, one piece that is mostly empty); b = 0 and x0 = b already a solution (no tick, and one phase-1 tick)."""
    case = _csr_twin(name)
    with _wide(ctx, _n_of(case), solves=name != "zero_rhs_n33"):           # b = 0 ends in the init kernel: no tick at all
        got = gc.run_case(ctx, case)
    _check_twin(case, got)


# ---- 4. a batch of 1100 ---------------------------------------------------------------------------------------------------------
def _solve_batch(ctx, order, B, shift, psi, jac):
    order = np.asarray(order)
    slots = list(range(len(order)))
    ctx.pop_reserve(len(order))
    ctx.pop_put(0, slots, B[order])
    info, inner, status = ctx.gmres(slots, shift[order], psi[order], 0, jac[order])
    return ctx.pop_get(2, slots, B.shape[1]), info, inner, status


def test_batch_of_1100_candidates_as_csr(ctx):
    """gc.batch_system() as CSR: n = 64, 1100 candidates (the compact kernel's second pass), every 37th breaking down at column
    0 and finished while its neighbours sit at other columns and in phase 1, Jacobi on the odd ones.  BATCH_RESTATED against the
    restatement (those that break down bit for bit), BATCH_ALONE bit-identical to their lone runs, and the batch in reverse
    order bit-identical row for row."""
    A, B, shift, psi, jac = gc.batch_system()
    P, n = B.shape
    As = sp.csr_matrix(A)
    with _wide(ctx, n):
        ctx.set_matrix_csr(As)
        X, info, inner, status = _solve_batch(ctx, np.arange(P), B, shift, psi, jac)
        Xr, info_r, inner_r, status_r = _solve_batch(ctx, np.arange(P)[::-1], B, shift, psi, jac)
        alone = [_solve_batch(ctx, [i], B, shift, psi, jac) for i in gc.BATCH_ALONE]
    assert (status == 0).all() and (info == 0).all()
    assert (inner[::37] == 1).all() and (np.delete(inner, np.arange(0, P, 37)) > 5).all()
    for i in gc.BATCH_RESTATED:
        H = gc.sparse_h(As, shift[i], psi[i])
        ref = gc.traced(H, B[i], B[i], (1.0 / H.diagonal()) if jac[i] else None)
        got = (X[i], info[i], inner[i], status[i])
        if i % 37 == 0:
            gc.check_exact(got, ref, f"batch[{i}]")
        else:
            assert ref[4] >= gc.GUARD, (i, ref[4])
            gc.check_rounded(got, ref, H, B[i], 1e-8, f"batch[{i}]")
    assert np.array_equal(info, info_r[::-1]) and np.array_equal(inner, inner_r[::-1]) and (status_r == 0).all()
    assert all(gc.same_bits(a, b) for a, b in zip(X, Xr[::-1]))
    for i, (x1, i1, n1, s1) in zip(gc.BATCH_ALONE, alone):
        assert (i1[0], n1[0], s1[0]) == (info[i], inner[i], 0), i
        assert gc.same_bits(x1[0], X[i]), i


# ---- 5. linear batches ----------------------------------------------------------------------------------------------------------
def _solve_linear(ctx, order, psi, jac, n):
    order = np.asarray(order)
    slots = list(range(len(order)))
    ctx.pop_reserve(len(order))
    info, inner, status = ctx.gmres(slots, np.zeros(len(order), dtype=np.complex128), psi[order], 1, jac[order])
    return ctx.pop_get(2, slots, n), info, inner, status


@pytest.mark.parametrize("P", [33, 34, 65])
def test_linear_batch_equals_each_candidate_alone(ctx, P):
    """rhs_mode = 1 at n = 1025 (three pieces, the last with one entry): one right-hand side, per-candidate psi and alternating
    Jacobi, so the candidates reach different columns and finish at different ticks; x, info and inner of every candidate
    bit-identical to its run alone."""
    n = 1025
    A = gc.banded(n, 1, 2.2)
    b = gc.crand(n, n)
    rng = np.random.default_rng(100 + P)
    psi = 10.0 ** rng.uniform(-3, -0.5, P)                               # up to 0.3 on a diagonal of modulus 2: other iteration counts
    jac = (np.arange(P) % 2).astype(np.int32)
    with _wide(ctx, n):
        ctx.set_matrix_csr(A)
        ctx.set_rhs(b)
        X, info, inner, status = _solve_linear(ctx, np.arange(P), psi, jac, n)
        alone = [_solve_linear(ctx, [i], psi, jac, n) for i in range(P)]
    assert (status == 0).all() and (info == 0).all() and len(set(inner.tolist())) > 1
    for i, (x1, i1, n1, s1) in enumerate(alone):
        assert (i1[0], n1[0], s1[0]) == (info[i], inner[i], 0), i
        assert gc.same_bits(x1[0], X[i]), i
    H = gc.sparse_h(A, 0.0, psi[1])
    ref = gc.traced(H, b, b, 1.0 / H.diagonal())
    assert info[1] == ref[1] and np.linalg.norm(X[1] - ref[0]) <= 1e-9 * np.linalg.norm(ref[0])


# ---- 6. non-finite data ---------------------------------------------------------------------------------------------------------
def test_non_finite_data_is_reported_as_not_converged(ctx):
    """A NaN in one candidate's right-hand side, an Inf and a NaN in the matrix, a NaN in one candidate's shift: info = maxiter
    and status 0, as the stream kernel reports it (tests/test_gpu_gmres_edges.py), and the neighbours with finite data are
    solved to the bits they have without the bad candidate."""
    n = 700                                                              # two pieces; the bad entries sit in the second
    A = sp.csr_matrix(gc.spread(n, 3, 0.5 / np.sqrt(n)))
    b = gc.crand(4, n)
    bad = b.copy()
    bad[n - 1] = complex(1.0, np.nan)
    z3 = np.zeros(3, dtype=np.complex128)

    def bind(M):
        ctx.set_matrix_csr(M)
        ctx.pop_reserve(3)
        ctx.pop_put(0, [0, 1, 2], np.stack([b, bad, b]))

    with _wide(ctx, n):
        for jac in (0, 1):
            j3 = np.full(3, jac, dtype=np.int32)
            bind(A)
            info, inner, status = ctx.gmres([0, 1, 2], z3, np.zeros(3), 0, j3, maxiter=7)
            X = ctx.pop_get(2, [0, 1, 2], n)
            assert list(info) == [0, 7, 0] and list(status) == [0, 0, 0] and inner[1] == 0, (info, inner, status)
            assert np.isfinite(X[[0, 2]].view(np.float64)).all() and gc.same_bits(X[0], X[2])
            ctx.pop_put(0, [0], b[None])
            i1, n1, s1 = ctx.gmres([0], z3[:1], np.zeros(1), 0, j3[:1], maxiter=7)
            assert (i1[0], n1[0], s1[0]) == (0, inner[0], 0) and gc.same_bits(ctx.pop_get(2, [0], n)[0], X[0])
            # a NaN shift: that candidate alone is lost
            bind(A)
            sh = z3.copy()
            sh[2] = complex(np.nan, 0.0)
            info, inner2, status = ctx.gmres([0, 1, 2], sh, np.zeros(3), 0, j3, maxiter=7)
            assert list(info) == [0, 7, 7] and list(status) == [0, 0, 0], (info, status)
            assert gc.same_bits(ctx.pop_get(2, [0], n)[0], X[0]) and inner2[0] == inner[0]
            for value in (np.inf, np.nan):
                Abad = A.toarray()
                Abad[n - 5, n - 7] = value
                bind(sp.csr_matrix(Abad))
                info, inner, status = ctx.gmres([0, 1, 2], z3, np.zeros(3), 0, j3, maxiter=7)
                assert list(info) == [7, 7, 7] and list(status) == [0, 0, 0], (value, info, status)


# ---- 7. chunks at n = 2^20 ------------------------------------------------------------------------------------------------------
def test_gmres_2_pow_20_in_chunks_equals_lone_runs(ctx):
    """The tridiagonal operator and shifts of test_gmres_2_pow_20_runs_large_batches_in_chunks.  First P = 50 with restart = 2,
    maxiter = 1, rtol = 0: two Arnoldi steps, info = 1 for all, W rows of candidates 0, 45, 46 and 49 bit-identical to their
    lone runs.  The chunk rule of maus_gmres counts restart + 3 rows per candidate against 1/16 of the device's memory, so that
    batch is ONE chunk on any device (and at restart = 20 an MI355X, 309 GB, holds 50 per chunk, not 46).  The run that is split
    is the second: restart = 20, maxiter = 1, rtol = 0 (twenty steps, info = 1) with four candidates more than the largest chunk
    this device can hold; the rows on both sides of the chunk boundary and the last one against their lone runs."""
    n = 1 << 20
    cmax = ctx.device_info()["hbm_total"] // 16 // (16 * (20 + 3) * n)            # no chunk of the restart = 20 run is larger
    P = max(50, cmax + 4)
    rng = np.random.default_rng(14)
    A = sp.diags([rng.standard_normal(n - 1) + 0j, 4.0 + 1j + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1) + 0j],
                 [-1, 0, 1], format="csr")
    with _wide(ctx, n):
        ctx.set_matrix_csr(A)
        ctx.pop_reserve(P)
        for k0 in range(0, P, 10):
            k1 = min(P, k0 + 10)
            ctx.pop_put(0, np.arange(k0, k1), rng.standard_normal((k1 - k0, n)) + 1j * rng.standard_normal((k1 - k0, n)))
        shift = 0.5 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
        psi = np.full(P, 1e-20)
        jac = np.zeros(P, dtype=np.int32)
        for restart, count, probe in ((2, 50, [0, 45, 46, 49]), (20, P, [0, cmax - 1, cmax, P - 1])):
            kw = dict(rtol=0.0, restart=restart, maxiter=1)
            info, inner, status = ctx.gmres(np.arange(count), shift[:count], psi[:count], 0, jac[:count], **kw)
            Wb = ctx.pop_get(2, probe, n)
            assert (status == 0).all() and (info == 1).all() and (inner == restart).all(), (restart, info, inner)
            for i, s in enumerate(probe):
                info1, inner1, _ = ctx.gmres([s], shift[[s]], psi[[s]], 0, jac[[s]], **kw)
                assert (info1[0], inner1[0]) == (1, restart)
                assert gc.same_bits(ctx.pop_get(2, [s], n)[0], Wb[i]), (restart, s)


# ---- 8. the method round trip ---------------------------------------------------------------------------------------------------
def test_method_round_trip_dense_ignores_it_and_default_comes_back():
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import GMRES_DEFAULT, GMRES_WIDE, MausHipError
    case = gc.BY_NAME["band_n1025_w1_j1"]
    dense = gc.BY_NAME["spread_conv_n1025_j1"]
    fresh = Context(0)
    try:
        assert fresh.gmres_method() == GMRES_DEFAULT
        assert [fresh.gmres_kernel_for(n, True) for n in (1, 16384, 16385, 1 << 20)] == [0, 0, 1, 1]
        ref_csr = gc.run_case(fresh, case)
        ref_dense = gc.run_case(fresh, dense)
    finally:
        fresh.close()
    c = Context(0)
    try:
        with pytest.raises(MausHipError, match="method"):
            c.gmres_set_method(2)
        c.gmres_set_method(GMRES_WIDE)
        assert c.gmres_method() == GMRES_WIDE
        assert [c.gmres_kernel_for(n, True) for n in (1, 16384, 16385, 1 << 20)] == [2, 2, 2, 2]      # every CSR size: no lower limit
        assert [c.gmres_kernel_for(n, False) for n in (1, 1025, 16384)] == [0, 0, 0]                  # a dense matrix ignores it
        with _wide(c, 1025):
            wide = gc.run_case(c, case)
        gc.check_case(case, wide)
        assert np.array_equal(wide[1], ref_csr[1]) and np.array_equal(wide[2], ref_csr[2])
        assert np.linalg.norm(wide[0] - ref_csr[0]) <= 1e-9 * np.linalg.norm(ref_csr[0])
        c.profile_enable(True)
        got_dense = gc.run_case(c, dense)                                # method 1, dense matrix: the register kernel, method 0's bits
        prof = c.profile_read()
        c.profile_enable(False)
        assert prof["gmres_wide"]["launches"] == 0 and prof["vector"]["launches"] > 0
        assert gc.same_bits(got_dense[0], ref_dense[0]) and np.array_equal(got_dense[2], ref_dense[2])
        c.gmres_set_method(GMRES_DEFAULT)
        assert c.gmres_method() == GMRES_DEFAULT and c.gmres_kernel_for(1025, True) == 0
        c.profile_enable(True)
        back = gc.run_case(c, case)
        prof = c.profile_read()
        c.profile_enable(False)
        assert prof["gmres_wide"]["launches"] == 0 and prof["vector"]["launches"] > 0
        assert gc.same_bits(back[0], ref_csr[0]) and np.array_equal(back[2], ref_csr[2])
    finally:
        c.close()


# ---- 9. through the API ---------------------------------------------------------------------------------------------------------
def _loop_bodies(A, b, mode, iters=3):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(31); random.seed(31); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": np.inf, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}                               # what the diagnostics report of a sparse matrix: GMRES preferred
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=24, quiet=True, sparse_mode="device",
                    sparse_gmres=mode, diag_info=diag)
    s.engine.ctx.profile_enable(True)
    rows = []
    for it in range(iters):
        s.loop_body(it + 1)
        rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates],
                     np.random.get_state()[2], np.random.get_state()[1].copy(), random.getstate()))
    prof = s.engine.ctx.profile_read()
    s.engine.ctx.profile_enable(False)
    return s, rows, prof


def test_maus_solver_wide_against_auto():
    """MAUS_Solver(sparse_mode='device', sparse_gmres='wide') on the 5-point operator + 2 I at n = 70^2 = 4900, 24 candidates,
    three loop bodies: the states, local_psi_retries_needed and the positions of both random streams of the 'auto' run, x within
    1e-9.  (The engine's own vector kernels share the class `vector`, so here only `gmres_wide` is looked at.)"""
    from test_band_host import five_point
    m = 70
    A = ((five_point(m) + 2.0 * sp.identity(m * m)) * (1.0 + 0.25j)).tocsr()
    n = A.shape[0]
    b = gc.crand(70, n)
    ref_s, ref, ref_prof = _loop_bodies(A, b, "auto")
    s, got, prof = _loop_bodies(A, b, "wide")
    assert s.engine.sparse_gmres == "wide" and s.engine.ctx.gmres_method() == 1 and s.engine.ctx.gmres_kernel_for(n, True) == 2
    assert ref_s.engine.ctx.gmres_method() == 0
    assert prof["gmres_wide"]["launches"] > 0 and ref_prof["gmres_wide"]["launches"] == 0
    assert len(s.candidates) == len(ref_s.candidates) >= 24
    for (r_rows, r_pos, r_key, r_py), (g_rows, g_pos, g_key, g_py) in zip(ref, got):
        assert r_rows == g_rows
        assert r_pos == g_pos and np.array_equal(r_key, g_key) and r_py == g_py
    for c, cr in zip(s.candidates, ref_s.candidates):
        assert np.linalg.norm(c.x_k - cr.x_k) <= 1e-9 * np.linalg.norm(cr.x_k), c.id
