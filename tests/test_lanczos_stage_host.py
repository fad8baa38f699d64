"""tests/lanczos_stage_cases.py on the CPU: the whole table passes for FakeLanczosContext and for the float64 restatement, every
planted fault of the restatement fails a named check, the recorded restatement values of check O are recomputed, and the inputs
have the properties the checks rely on (no undecided candidate, cond(S) <= 10, more than 32 stored entries per row)."""
import numpy as np
import pytest

import lanczos_stage_cases as lc
from test_lanczos_host import FakeLanczosContext

STEPPERS = {"fake": FakeLanczosContext, "restatement": lc.Restatement}


def faulty(fault):
    return lambda: lc.Restatement(fault)


@pytest.fixture(params=list(STEPPERS))
def make(request):
    return STEPPERS[request.param]


# ---- the table passes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.STEP_NAMES)
def test_step_cases(make, name):
    lc.run_step_case(name, make)


def test_exact_cases(make):
    lc.run_exact_cases(make)


def test_threshold(make):
    lc.run_threshold(make)


@pytest.mark.parametrize("ncv,m,keep", lc.RESTARTS)
def test_restart(make, ncv, m, keep):
    lc.run_restart(make, ncv, m, keep)


@pytest.mark.parametrize("ncv,m,k,kind", lc.FINISHES)
def test_finish(make, ncv, m, k, kind):
    lc.run_finish(make, ncv, m, k, kind)


def test_finish_with_k_0_drops_everything(make):
    lc.run_finish_drops(make)


@pytest.mark.parametrize("n,k", lc.MATCH_CASES)
def test_match(make, n, k):
    lc.run_match_case(make, n, k)


def test_match_crafted_zero_row_and_stamps(make):
    lc.run_match_crafted(make)
    lc.run_match_zero_row(make)
    lc.run_match_stamps(make)


def test_match_second_chunk(make):
    lc.run_match_chunks(make)


def test_big(make):
    lc.run_big(make)


# ---- every planted fault fails, and which check it fails -----------------------------------------------------------------------------
# fault -> (the run that shows it, the check it must fail)
SHOWN_BY = {
    "dot_tail": (lambda mk: lc.run_step_case("tri_n513_ncv20", mk), "check S"),
    "norm_stretch": (lambda mk: lc.run_step_case("tri_n1023_ncv20", mk), "check S: row 0"),
    "join_blocks": (lambda mk: lc.run_step_case("tri_n131073_ncv4", mk), "check S"),
    "join_blocks_match": (lc.run_big, "match: n = 2\\^20 \\+ 1: idx"),
    "one_pass": (lambda mk: lc.run_step_case("shifted23x23_ncv20", mk), "check S: shifted23x23_ncv20: row"),
    "no_conj": (lambda mk: lc.run_step_case("tri_n513_ncv20", mk), "check S"),
    "alpha_prev": (lambda mk: lc.run_step_case("tri_n513_ncv20", mk), "check S: .*alpha\\[1\\]"),
    "threshold_ge": (lc.run_threshold, "threshold: beta == tol_abs"),
    "s_transposed": (lambda mk: lc.run_restart(mk, 20, 20, 12), "restart \\(20, 12\\): rows 0"),
    "restart_in_place": (lambda mk: lc.run_restart(mk, 20, 20, 12), "restart \\(20, 12\\): rows 0"),
    "keep_row_first": (lambda mk: lc.run_restart(mk, 32, 32, 31), "restart \\(32, 31\\): rows 0"),
    "tie_last": (lc.run_match_crafted, "match: crafted candidate 0: idx = 4"),
    "nan_ignored": (lc.run_match_crafted, "match: crafted candidate 1: idx = 0"),
    "wrong_norm": (lc.run_match_zero_row, "match: zero Ritz row: norm"),
}


def test_every_fault_is_listed():
    assert set(SHOWN_BY) == set(lc.FAULTS)


@pytest.mark.parametrize("fault", lc.FAULTS)
def test_planted_fault_fails_its_check(fault):
    run, check = SHOWN_BY[fault]
    with pytest.raises(AssertionError, match=check):
        run(faulty(fault))


@pytest.mark.parametrize("fault,run,check", [
    ("s_transposed", lambda mk: lc.run_finish(mk, 20, 20, 6, "eigh"), "finish"),
    ("s_transposed", lambda mk: lc.run_restart(mk, 20, 2, 1), None),
    ("restart_in_place", lambda mk: lc.run_restart(mk, 20, 2, 1), None),
    ("keep_row_first", lambda mk: lc.run_restart(mk, 20, 2, 1), "restart \\(2, 1\\): rows 0"),
    ("one_pass", lambda mk: lc.run_finish(mk, 20, 20, 6, "random"), None),
    ("dot_tail", lambda mk: lc.run_finish(mk, 20, 20, 6, "random"), "finish"),
    ("join_blocks", lc.run_big, "match: the unit Ritz rows"),
])
def test_faults_in_other_places(fault, run, check):
    """The same faults where they show elsewhere -- and where they cannot: a one-column S reads the same transposed, a one-row
    recombination reads nothing it has written, and one Gram-Schmidt pass is enough for rows with cond(S) <= 10."""
    if check is None:
        run(faulty(fault))
    else:
        with pytest.raises(AssertionError, match=check):
            run(faulty(fault))


# ---- recorded values and input conditions ------------------------------------------------------------------------------------------
def test_recorded_restatement_values():
    assert set(lc.RECORDED_O) == set(lc.STEP_NAMES) | {"big"}
    for name, (g, f) in lc.RECORDED_O.items():
        g0, f0 = lc.restatement_o(name)
        print(f"RECORDED_O {name}: g = {g0 / lc.EPS:.2f} eps, f = {f0 / lc.EPS:.2f} eps")
        for got, rec in ((g0 / lc.EPS, g), (f0 / lc.EPS, f)):
            assert rec / 2.0 <= got <= rec * 2.0 or max(got, rec) <= 0.05, (name, got, rec)


def test_one_pass_fails_check_o_on_the_shifted_lattice():
    name = "shifted23x23_ncv20"
    A, v0, ncv, tol = lc.case_inputs(name)
    B, alpha, beta = lc._sweep(lc.Restatement("one_pass"), A, v0, ncv, tol)
    g1, _ = lc.sweep_values(A, B, alpha, beta)
    g2, _ = lc.restatement_o(name)
    assert g2 <= 4 * lc.EPS and g1 >= 1e-8, (g1, g2)
    with pytest.raises(AssertionError, match="check O: .*B B\\^H - I"):
        lc.check_o(name, A, B, alpha, beta)


def test_input_conditions():
    A = lc.operator("wide", 513)
    assert A.nnz > 32 * 513 and abs(A - A.conj().T).max() == 0.0
    for i in range(513):
        assert np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
    S = lc.random_s(20, 6)
    assert np.linalg.cond(S) <= 10.0 and abs(np.linalg.norm(S.T @ S - np.eye(6))) > 1.0     # and far from orthonormal
    for n, k in lc.MATCH_CASES:
        R = np.array([lc.unit(n, p, lc.PHASES[j % 4]) for j, p in enumerate(lc.positions(n, k))])[::-1]
        for count in lc.MATCH_COUNTS:
            rng = np.random.default_rng([n, k, count])
            X = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
            assert lc.undecided(R, X) == 0
    # the pair-swap operator does what the exact cases say
    P = lc.operator("swap", 514)
    assert np.array_equal(P @ lc.unit(514, 0), lc.unit(514, 1)) and np.array_equal(P @ lc.unit(514, 1), lc.unit(514, 0))
    # the sizes reach the paths: a second trip of the strided joins, a second chunk
    assert lc._joins(131072) == 1 and lc._joins(131073) == 2 and lc._joins(lc.BIG_N) == 9
    assert (lc.BIG_N + lc.MSPAN - 1) // lc.MSPAN == 257 and lc.CHUNK + 1 == 32769


def test_bounds_are_far_above_the_restatement_and_below_a_wrong_entry():
    """The derived bounds leave the restatement room (it sits at a few per cent of them) and are still far below what one lost
    entry does: the two facts that make check S a test."""
    rec = lc.run_step_case("tri_n513_ncv20", lc.Restatement)
    assert max(rec["alpha"], rec["beta"], rec["row"]) <= 0.25
    assert rec["row_eps_s_beta"] <= 2.0 and rec["alpha_eps_s"] <= 2.0 and rec["beta_eps_s"] <= 2.0
