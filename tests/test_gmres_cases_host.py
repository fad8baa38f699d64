"""CPU tier of the GMRES case table (tests/gmres_cases.py): the table's references are right (SciPy's gmres and the oracle's
restatement agree on every case, the traced copy is the restatement), every case keeps its decisions away from their
thresholds, the test doubles pass the checkers the GPU tier applies to the device, the checkers reject planted errors, and the
doubles keep the two contracts of maus_gmres that no trajectory shows (non-finite data, restart outside 1 .. 20)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import gmres_cases as gc
from fake_ctx import FakeContext
from oracle import maus_oracle as orc
from test_sparse_host import FakeSparseContext

NAMES = [c["name"] for c in gc.CASES]


def _scipy(H, b, inv, case):
    if inv is None:
        M = None
    else:
        M = sp.diags(inv, format="csc") if sp.issparse(H) else np.diag(inv)
    count = [0]
    with np.errstate(all="ignore"):
        x, info = spla.gmres(H, b, x0=b, rtol=case["rtol"], restart=case["restart"], maxiter=case["maxiter"], M=M,
                             callback=lambda r: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
    return x, info, count[0]


@pytest.mark.parametrize("name", NAMES)
def test_scipy_restatement_and_traced_copy_agree(name):
    case = gc.BY_NAME[name]
    for i, ((H, b, inv), ref) in enumerate(zip(gc.systems(case), gc.reference(name))):
        xr, info_r, inner_r, _ = orc.gmres_restated(H, b, b, inv, rtol=case["rtol"], maxiter=case["maxiter"], restart=case["restart"])
        assert gc.same_bits(xr, ref[0]) and (info_r, inner_r) == ref[1:3], (name, i, "traced() is not the restatement")
        xs, info_s, inner_s = _scipy(H, b, inv, case)
        assert (info_s, inner_s) == (info_r, inner_r), (name, i, info_s, inner_s, info_r, inner_r)
        if case["exact"]:
            assert gc.same_bits(xs, xr), (name, i)
        else:
            assert np.linalg.norm(xs - xr) <= 1e-12 * np.linalg.norm(xr), (name, i, np.linalg.norm(xs - xr) / np.linalg.norm(xr))
    if case["expect"] is not None:
        assert tuple(gc.reference(name)[0][1:3]) == tuple(case["expect"]), (name, gc.reference(name)[0][1:3])


@pytest.mark.parametrize("name", NAMES)
def test_every_case_keeps_its_decisions_off_the_thresholds(name):
    case = gc.BY_NAME[name]
    closest = min(r[4] for r in gc.reference(name))
    assert case["exact"] or closest >= gc.GUARD, (name, closest)


def test_boundary_cases_restart_as_intended():
    """Weight 1.0: one cycle; the second weight: 2 to 4 cycles at every size, with and without Jacobi."""
    for case in gc.ROUNDED:
        if case["name"].startswith("band_"):
            cyc = gc.reference(case["name"])[0][3]
            assert (cyc == 1) if "_w0_" in case["name"] else (2 <= cyc <= 4), (case["name"], cyc)


def _double(case):
    return FakeSparseContext() if case["build"]()["csr"] else FakeContext()


@pytest.mark.parametrize("name", NAMES)
def test_doubles_pass_the_device_checkers(name):
    case = gc.BY_NAME[name]
    got = gc.run_case(_double(case), case)
    gc.check_case(case, got)
    if case in gc.ONE_CYCLE_CASES:
        ratio, own = gc.check_one_cycle(case, got)
        assert ratio <= 1.0 + 1e-12 and own <= gc.ONE_CYCLE_OWN_MAX, (name, ratio, own)


@pytest.mark.parametrize("name", ["cyclic_im_n20_zgemm", "eigvec_diag40_j1_csr", "band_n257_w1_j0", "restart5_n64",
                                  "dense_tail_n65", "scale_up_n64", "onecycle_n64_m8_j1"])
def test_checkers_reject_planted_errors(name):
    case = gc.BY_NAME[name]
    good = gc.run_case(_double(case), case)
    gc.check_case(case, good)
    k = good[0].shape[0]

    def planted(what):
        X, info, inner, status = (np.array(a, copy=True) for a in good)
        if what == "x":
            X[k - 1, -1] += 1e-8 * np.linalg.norm(X[k - 1])       # the last element, off by 1e-8 of the vector's norm
        elif what == "inner":
            inner[k - 1] += 1
        elif what == "info":
            info[k - 1] = case["maxiter"] if info[k - 1] == 0 else 0
        else:
            status[k - 1] = -2
        return X, info, inner, status

    for what in ("x", "inner", "info", "status"):
        with pytest.raises(AssertionError):
            gc.check_case(case, planted(what))


def test_one_cycle_checker_rejects_a_last_element_off_by_1e12():
    """The bound against the independent minimiser is 64 x the restatement's own deviation (1e-15 .. 1e-13): it sees an error
    in one entry that is four orders below what the 1e-9 of check_rounded can see."""
    case = gc.BY_NAME["onecycle_n1025_m20_j0"]
    X, info, inner, status = gc.run_case(FakeContext(), case)
    gc.check_one_cycle(case, (X, info, inner, status))
    X[0, -1] += 1e-12 * np.linalg.norm(X[0])
    gc.check_case(case, (X, info, inner, status))
    with pytest.raises(AssertionError):
        gc.check_one_cycle(case, (X, info, inner, status))


def test_batch_candidates_checked_against_the_restatement_meet_the_guard():
    A, B, shift, psi, jac = gc.batch_system()
    for i in gc.BATCH_RESTATED:
        H = gc.dense_h(A, shift[i], psi[i])
        r = gc.traced(H, B[i], B[i], (1.0 / np.diag(H)) if jac[i] else None)
        assert r[4] >= gc.GUARD, (i, r[1:])
    for i in range(0, gc.BATCH_P, 37):
        H = gc.dense_h(A, shift[i], psi[i])
        r = gc.traced(H, B[i], B[i], (1.0 / np.diag(H)) if jac[i] else None)
        assert r[1:4] == (0, 1, 1), (i, r[1:])                  # breakdown at column 0, converged
    assert 37 in gc.BATCH_RESTATED and 1073 % 37 == 0 and 1073 in gc.BATCH_RESTATED


@pytest.mark.parametrize("make", [FakeContext, FakeSparseContext])
def test_non_finite_data_ends_with_info_maxiter_and_status_0(make):
    """maus_gmres scans nothing: with a NaN in the right-hand side or an Inf in the matrix the device ends with
    info = maxiter, status 0 (SciPy: the same after maxiter cycles of NaN); status -1 belongs to maus_gmres_pert."""
    n = 24
    A = gc.spread(n, 3)
    b = gc.crand(4, n)
    for what in ("rhs", "matrix"):
        Ab, bb = A.copy(), b.copy()
        if what == "rhs":
            bb[n - 1] = np.nan
        else:
            Ab[5, 7] = np.inf
        ctx = make()
        if make is FakeSparseContext:
            ctx.set_matrix_csr(sp.csr_matrix(Ab))
        else:
            ctx.set_matrix(Ab)
        ctx.pop_reserve(2)
        ctx.pop_put(0, [0, 1], np.stack([bb, b]))
        info, inner, status = ctx.gmres([0, 1], np.zeros(2, dtype=np.complex128), np.zeros(2), 0, np.zeros(2, dtype=np.int32), maxiter=7)
        assert info[0] == 7 and status[0] == 0, (what, info, status)
        if what == "rhs":
            assert info[1] == 0 and status[1] == 0           # the neighbour's data is finite
    # the dense mode does scan (AMS:94 analogue)
    ctx = FakeContext()
    ctx.set_matrix(A)
    ctx.pop_reserve(1)
    bb = b.copy()
    bb[0] = np.nan
    ctx.pop_put(0, [0], bb)
    assert ctx.gmres_pert([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 0, np.zeros(1, dtype=np.int32), 0, None)[2][0] == -1


@pytest.mark.parametrize("restart", [0, -1, 21, 50])
def test_doubles_refuse_a_restart_outside_1_to_20(restart):
    from adaptive_matrix_solver_amd._cabi import MausHipError
    A = gc.spread(8, 3)
    for make in (FakeContext, FakeSparseContext):
        ctx = make()
        ctx.set_matrix(A)
        ctx.pop_reserve(1)
        ctx.pop_put(0, [0], gc.crand(1, 8))
        args = ([0], np.zeros(1, dtype=np.complex128), np.zeros(1), 0, np.zeros(1, dtype=np.int32))
        with pytest.raises(MausHipError, match="between 1 and 20"):
            ctx.gmres(*args, restart=restart)
        if make is FakeContext:
            with pytest.raises(MausHipError, match="between 1 and 20"):
                ctx.gmres_pert(*args, 0, None, restart=restart)
