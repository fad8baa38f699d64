"""The stages of the device Lanczos (csrc/lanczos.hip), separated: the raw entry points of _cabi.Context driven step by step, the
live basis read back with lanczos_get_basis, and every step, restart, finish and match held by tests/lanczos_stage_cases.py to a
local extended-precision recomputation under a-priori bounds (check S), to the float64 restatement's orthogonality and Lanczos
relation (check O), and to the exact statements of the unit-vector cases -- at the edges of the 512-entry stretch (n = 255 .. 1025),
with a second trip of the strided joins (n = 131073 in a step, n = 2^20 + 1 in the match), at ncv = 32 and k = 8, on rows of more
than 32 entries (the wave schedule of the SpMM, writing the basis it reads), through the in-place restart, the second chunk of
32768 candidates, ties, NaN and the threshold itself.  tests/test_lanczos_stage_host.py shows on the CPU that the same checks
pass for a NumPy restatement and fail for each of its planted faults.

Measured on an MI355X, as error / bound (row 0; alpha, beta, rows of check S; g, f of check O), for the record only:
    tri n = 1, 2, 33      row 0 0.034, 0.11, 0.032; alpha <= 0.0047, beta <= 0.0009, rows <= 0.0034; g <= 0.047, f <= 0.028
    tri n = 255 .. 1025   row 0 <= 0.0090; alpha <= 0.0037, beta <= 0.0016, rows <= 0.0069; g <= 0.0102, f <= 0.0114
    lattice 32 x 33       row 0 0.0021; alpha 0.0011, beta 0.0010, rows 0.0055; g 0.0060, f 0.0081
    shifted 23 x 23       row 0 0.0028; alpha 0.0032, beta 0.0001, rows 0.0065; g 0.0102, f 0.0167
    wide rows 513         row 0 0.0027; alpha 0.00003, beta 0.00006, rows 0.0004; g 0.0072, f 0.0041
    tri n = 131072 / 3    alpha 0.0015 / 0.0007, beta 0.0015 / 0.0007, rows 0.0070 / 0.0074; g 0.041 / 0.048, f 0.014 / 0.014
    tri n = 2^20 + 1      alpha 0.0016, beta 0.0013, rows 0.0106; g 0.090, f 0.018
    restart (m, keep)     (32, 31) 0.13, (32, 1) 0.061, (20, 12) 0.20, (2, 1) 0.47
    finish (m, k)         rows: (32, 8) 0.012, (20, 6) 0.018, (20, 1) 0.016, (1, 1) 0.013, random S 0.020; g <= 0.0102
The rows sit at 0.04 - 0.30 eps s_j / beta_j, alpha and beta at 0.05 - 0.48 eps s_j; every exact case is exact."""
import numpy as np
import pytest

import kernel_refs as kr
import lanczos_stage_cases as lc

pytestmark = pytest.mark.gpu


def make():
    from adaptive_matrix_solver_amd import Context
    return Context(0)


def make_sell():
    c = make()
    c.spmm_set_method(1)
    return c


@pytest.mark.parametrize("name", lc.STEP_NAMES)
def test_step_cases(name):
    lc.run_step_case(name, make)


def test_wide_rows_run_the_wave_schedule():
    A = lc.operator("wide", 513)
    with lc.opened(make) as c:
        c.set_matrix_csr(A)
        assert c.matrix_is_sparse() == "wave"
    with lc.opened(make) as c:
        c.set_matrix_csr(lc.operator("tri", 513))
        assert c.matrix_is_sparse() == "rows"


def test_exact_cases():
    lc.run_exact_cases(make)


def test_threshold():
    lc.run_threshold(make)


@pytest.mark.parametrize("ncv,m,keep", lc.RESTARTS)
def test_restart(ncv, m, keep):
    lc.run_restart(make, ncv, m, keep)


@pytest.mark.parametrize("ncv,m,k,kind", lc.FINISHES)
def test_finish(ncv, m, k, kind):
    lc.run_finish(make, ncv, m, k, kind)


def test_finish_with_k_0_drops_everything():
    from adaptive_matrix_solver_amd._cabi import MausHipError
    lc.run_finish_drops(make)
    with lc.opened(make) as c:
        lc._basis(c, 20)
        c.lanczos_finish(np.zeros((20, 0)))
        with pytest.raises(MausHipError, match="no Ritz rows"):
            c.get_ritz_rows()
        with pytest.raises(MausHipError, match="no Lanczos basis"):
            c.lanczos_get_basis(0, 1)


def test_get_basis_refuses_bad_ranges():
    from adaptive_matrix_solver_amd._cabi import MausHipError
    with lc.opened(make) as c:
        c.set_matrix_csr(lc.operator("tri", 33))
        with pytest.raises(MausHipError, match="no Lanczos basis"):
            c.lanczos_get_basis(0, 1)
        c.lanczos_begin(lc.start_vector(33), 4)
        for bad in ((-1, 1), (0, 0), (0, 6), (4, 2), (5, 1)):
            with pytest.raises(MausHipError, match="maus_lanczos_get_basis: need"):
                c.lanczos_get_basis(*bad)
        assert c.lanczos_get_basis(0, 5).shape == (5, 33) and c.lanczos_get_basis(4, 1).shape == (1, 33)


@pytest.mark.parametrize("n,k", lc.MATCH_CASES)
def test_match(n, k):
    lc.run_match_case(make, n, k)


def test_match_crafted_ties_and_nan():
    lc.run_match_crafted(make)


def test_match_with_a_zero_ritz_row():
    lc.run_match_zero_row(make)


def test_match_drops_the_kept_products():
    lc.run_match_stamps(make)


def test_match_second_chunk():
    lc.run_match_chunks(make)


def test_big():
    lc.run_big(make)


def test_sliced_ell_products_give_the_same_bits():
    """The (513, 20) step case and a match case under spmm_set_method(1): bit-equal to method 0."""
    from adaptive_matrix_solver_amd._cabi import SPMM_KERNEL_ROWS, SPMM_KERNEL_SELL
    A, v0, ncv, tol = lc.case_inputs("tri_n513_ncv20")
    out = []
    for mk, kernel in ((make, SPMM_KERNEL_ROWS), (make_sell, SPMM_KERNEL_SELL)):
        with lc.opened(mk) as c:
            B, alpha, beta = lc._sweep(c, A, v0, ncv, tol)
            assert c.spmm_kernel_for(False) == kernel
            out.append((B, alpha, beta))
    for a, b, what in zip(out[0], out[1], ("rows", "alpha", "beta")):
        kr.check_bits(b, a, f"sliced-ELL sweep: {what}")
    lc.run_step_case("tri_n513_ncv20", make_sell)
    n, k = 4097, 6
    rng = np.random.default_rng(31)
    X = rng.standard_normal((9, n)) + 1j * rng.standard_normal((9, n))
    slots = np.arange(9)[::-1]
    out = []
    for mk in (make, make_sell):
        with lc.opened(mk) as c:
            c.set_matrix_csr(lc.operator("tri", n))
            R = lc.unit_ritz_rows(c, n, lc.positions(n, k))
            idx, nrm, rows = lc._match(c, n, X, slots, cap=9)
            num, den = c.matvec_rayleigh(slots)
            lc.check_match(R, X, idx, nrm, rows, "sliced-ELL")
            out.append((np.array(idx, dtype=np.float64), nrm, rows, num, den))
    for a, b, what in zip(out[0], out[1], ("idx", "norms", "rows", "Rayleigh numerators", "Rayleigh denominators")):
        kr.check_bits(b, a, f"sliced-ELL match: {what}")
