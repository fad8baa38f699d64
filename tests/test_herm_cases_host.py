"""The case table of tests/herm_cases.py on the CPU: the checks are satisfiable -- LAPACK (zhetrd + zungqr) and a plain NumPy
restatement of the unblocked reduction pass every one of them, LAPACK also the exact statements that apply to it (the split
zeros, the real Q, the lower triangle alone, the scaling law at 2^+-300) -- and they bite: the restatement fails them under
each of seven planted faults.  tests/test_gpu_herm_reduction.py then holds the device to the same table.

LAPACK's check-A values recomputed here (r / eps, u / eps): n = 65: 2.3, 3.1; 200: 3.4, 4.2; 600: 4.6, 5.1; 1100: 5.7, 5.9;
2100: 7.6, 7.1 (herm_cases.LAPACK_RECORDED holds the recorded ones; the test allows a factor of two)."""
import numpy as np
import pytest

import herm_cases as hc
import scenarios

@pytest.mark.parametrize("name", hc.NAMES)
def test_lapack_meets_every_check(name, monkeypatch):
    if name == "scaled":                                             # LAPACK's law is asserted at 2^+-300 only
        monkeypatch.setattr(hc, "SCALES", hc.SCALES[:2])
    hc.run_case(name, hc.lapack_reduce)


@pytest.mark.parametrize("name", [n for n in hc.NAMES if hc.matrix(n).shape[0] <= 321] + ["chunk8_n600"])
def test_restatement_meets_every_check(name):
    hc.run_case(name, hc.numpy_reduce)


@pytest.mark.parametrize("n", sorted(hc.LAPACK_RECORDED))
def test_lapack_check_a_values_are_the_recorded_ones(n):
    A = scenarios.hermitian(n, n)
    r, u = hc.Probe(A).values(*hc.lapack_reduce(A))
    r0, u0 = hc.LAPACK_RECORDED[n]
    print(f"n = {n}: r = {r / hc.EPS:.2f} eps, u = {u / hc.EPS:.2f} eps (recorded {r0}, {u0})")
    assert r0 / 2 <= r / hc.EPS <= 2 * r0 and u0 / 2 <= u / hc.EPS <= 2 * u0


def test_one_wrong_entry_is_twelve_orders_above_the_bound():
    """What check A is there to catch: one entry of A left out moves r by about |a| / (||A||_2 sqrt(n))."""
    name = "random_n321"
    A = hc.matrix(name).copy()
    A[200, 100] = 0.0
    with pytest.raises(AssertionError):
        hc.check_a(name, *hc.lapack_reduce(A))


# the case on which each planted fault must show
FAULT_CASE = {"skip_tile": "random_n257", "upper_tile": "lower_only", "diag_imag": "lower_only", "drop_chunk": "chunk8_n600",
              "beta_sign": "random_n130", "tau_conj": "random_n130", "unscaled": "scaled"}


@pytest.mark.parametrize("fault", hc.FAULTS)
def test_planted_fault_fails_the_checks(fault):
    name = FAULT_CASE[fault]
    hc.run_case(name, hc.numpy_reduce)                               # (the clean restatement passes the same case)
    with pytest.raises(AssertionError) as ex:
        hc.run_case(name, lambda A, chunk: hc.numpy_reduce(A, chunk, fault=fault))
    print(fault, "->", str(ex.value)[:160])


def test_fault_table_is_complete():
    assert set(FAULT_CASE) == set(hc.FAULTS) and len(hc.FAULTS) == 7


def test_restatement_scales_outside_the_safe_range_only():
    """The restatement's scaling rule is the device's (herm.hip): nothing is touched for 2^-400 <= max |a| < 2^400."""
    A = hc.matrix("scaled")
    d, e, Q = hc.numpy_reduce(A)
    for s in (2.0 ** -398, 2.0 ** 396):
        ds, es, Qs = hc.numpy_reduce(A * s, fault="unscaled")
        assert hc.bits(ds, es, Qs) == hc.bits(d * s, e * s, Q)


# ---- the rule for the tiles per workgroup (maus_herm_chunk_plan: no device work) -------------------------------------------------
def _strips(T, hch):
    return sum(tb // hch + 1 for tb in range(T))


def test_chunk_plan_ties_the_forced_cases_to_the_large_orders():
    """What the rule launches: 4 tiles per workgroup for every column up to n = 4096, 8 for the first column at n = 8192, 16 at
    n = 16384 -- the two values that tests/test_gpu_herm_reduction.py forces at n = 577 .. 1100."""
    from adaptive_matrix_solver_amd import Context
    from adaptive_matrix_solver_amd._cabi import MausHipError
    plan = Context.herm_chunk_plan
    for n in (2, 3, 64, 65, 200, 777, 1100, 1536, 4096):
        cols = range(n - 1) if n <= 1100 else list(range(0, n - 1, 61)) + [n - 2]
        assert {plan(n, i)[1] for i in cols} == {4}, n
    assert plan(8192, 0) == (128, 8, _strips(128, 8))
    assert plan(16384, 0) == (256, 16, _strips(256, 16))
    # the rule itself: the largest of 16, 8, 4 with at least 768 workgroups, else 4; it moves with the column
    for n in (6000, 6600, 7000, 8192, 9000, 9200, 12000, 16384):
        for i in (0, 63, 64, 1000, n // 2, n - 65, n - 2):
            T, hch, ns = plan(n, i)
            assert T == (n + 63) // 64 - (i + 1) // 64
            want = next((h for h in (16, 8) if _strips(T, h) >= 768), 4)
            assert (hch, ns) == (want, _strips(T, want)), (n, i)
    # forced values and ns = sum_{tb < T} (tb / hch + 1) on a small grid
    for n in (1, 2, 63, 64, 65, 130, 577, 600, 1089, 1100, 2100):
        for i in sorted({0, 1, 62, 63, 64, 127, n // 2, n - 2, n - 1} & set(range(n))):
            for forced in (0, 4, 8, 16):
                T, hch, ns = plan(n, i, forced)
                if i == n - 1:
                    assert (T, hch, ns) == (0, 0, 0)                 # the last column has no matvec
                    continue
                assert T == (n + 63) // 64 - (i + 1) // 64 and T >= 1
                assert hch == (forced or 4) and ns == _strips(T, hch), (n, i, forced)
    # two chunks in a block row: first at these orders
    assert plan(577, 0, 8)[2] == 10 + 2 and plan(576, 0, 8)[2] == 9 + 1
    assert plan(1089, 0, 16)[2] == 18 + 2 and plan(1088, 0, 16)[2] == 17 + 1
    for bad in ((0, 0, 0), (5, -1, 0), (5, 5, 0), (5, 0, 3), (5, 0, 32)):
        with pytest.raises(MausHipError):
            plan(*bad)
