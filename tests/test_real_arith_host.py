"""real_arith="on" without a device (csrc/gmres.hip, DESIGN §11 "GMRES in real arithmetic"): the keyword and MAUS_REAL_ARITH,
the flag that decides what counts as real, and the claim the real path rests on, restated in NumPy -- GMRES on a real system
run with float64 vectors (the terms that multiply an exact zero removed) returns the bits, the iteration counts and the exits
of the same text run with complex128 vectors.  That makes the claim a property of the arithmetic, not of one compiler."""
import numpy as np
import pytest
import scipy.sparse as sp

import gmres_cases as gc
import real_cases as rc


# ---- keyword and environment ------------------------------------------------------------------------------------------------
def test_keyword_values_and_environment(monkeypatch):
    from adaptive_matrix_solver_amd import engine
    monkeypatch.delenv("MAUS_REAL_ARITH", raising=False)
    assert engine.REAL_ARITH_MODES == ("auto", "off", "on")
    assert engine.real_arith_mode(None) == "auto"
    for m in engine.REAL_ARITH_MODES:
        assert engine.real_arith_mode(m) == m
    for bad in ("ON", "real", "", "1", True):
        with pytest.raises(ValueError, match="real_arith must be one of"):
            engine.real_arith_mode(bad)
    monkeypatch.setenv("MAUS_REAL_ARITH", "on")
    assert engine.real_arith_mode(None) == "on"
    assert engine.real_arith_mode("off") == "off"                      # the keyword wins
    monkeypatch.setenv("MAUS_REAL_ARITH", "yes")
    with pytest.raises(ValueError, match="real_arith must be one of"):
        engine.real_arith_mode(None)


def test_keyword_reaches_the_solvers(monkeypatch):
    """MAUS_Solver and InverseIterateSolver validate the keyword before they touch a device."""
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver, MAUS_Solver, ProblemType
    monkeypatch.delenv("MAUS_REAL_ARITH", raising=False)
    assert InverseIterateSolver(8, 1e-20, 2, real_arith="on").real_arith == "on"
    assert InverseIterateSolver(8, 1e-20, 2).real_arith == "auto"
    with pytest.raises(ValueError, match="real_arith"):
        InverseIterateSolver(8, 1e-20, 2, real_arith="maybe")
    with pytest.raises(ValueError, match="real_arith"):
        MAUS_Solver(np.eye(4), ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=np.ones(4), real_arith="maybe")


def test_binding_constants():
    from adaptive_matrix_solver_amd import _cabi
    assert (_cabi.REAL_OFF, _cabi.REAL_ON) == (0, 1)
    assert (_cabi.REAL_OK, _cabi.REAL_METHOD_OFF, _cabi.REAL_NOT_CSR, _cabi.REAL_MATRIX_COMPLEX, _cabi.REAL_RHS_ROWS,
            _cabi.REAL_RHS_COMPLEX, _cabi.REAL_SHIFT_COMPLEX) == tuple(range(7))
    assert (_cabi.KC_GMRES_REAL, _cabi.KC_SPMM_REAL) == (19, 20) and _cabi.KC_BAND_SPLIT == 18    # appended behind the others


# ---- the flag ---------------------------------------------------------------------------------------------------------------
def test_flag_on_the_edge_values():
    """-0.0 counts as real; the smallest denormal, NaN, Inf and any number do not; the real part plays no role."""
    from adaptive_matrix_solver_amd._cabi import real_values_flagged as flagged
    z = lambda re, im: np.array([complex(re, im)])
    assert flagged(z(1.5, 0.0)) and flagged(z(1.5, -0.0)) and flagged(z(-0.0, -0.0))
    assert flagged(z(np.nan, 0.0)) and flagged(z(np.inf, -0.0))        # only the imaginary bits are looked at
    assert not flagged(z(1.0, 5e-324)) and not flagged(z(1.0, -5e-324))
    assert not flagged(z(1.0, np.nan)) and not flagged(z(1.0, np.inf)) and not flagged(z(0.0, 1.0))
    assert flagged(np.zeros(0, dtype=np.complex128))
    v = np.arange(1.0, 1001.0) + 0j
    assert flagged(v) and flagged(v.reshape(10, 100))
    for i in (0, 500, 999):
        w = v.copy()
        w[i] = complex(w[i].real, 5e-324)
        assert not flagged(w), i
    assert flagged(np.conj(v))                                         # conj of +0 is -0
    for values in (v, np.conj(v), z(1.0, 5e-324), z(1.0, np.nan)):
        assert flagged(values) == rc.flagged_real(values)
    assert flagged(rc.banded(300).data) and not flagged(gc.banded(300, 1, 1.0).data)


# ---- the claim --------------------------------------------------------------------------------------------------------------
def _diag40(b_value):
    return sp.csr_matrix(np.diag(np.arange(1.0, 41.0)).astype(np.complex128)), gc.unit_vector(40, 3, b_value)


def _small(n):
    return rc.real_csr(sp.csr_matrix(gc.shifted_ginibre(n, 40 + n))), rc.real_vec(60 + n, n)


CLAIM = {
    # name: (A, b, shift, psi, jacobi, kwargs, (info, inner) where known in closed form)
    "cyclic_n8": lambda: (rc.cyclic(8), gc.unit_vector(8, 0), 0.0, 0.0, 0, {}, (0, 8)),
    "cyclic_n20": lambda: (rc.cyclic(20), gc.unit_vector(20, 0), 0.0, 0.0, 0, {}, (0, 20)),
    "cyclic_n21_maxiter4": lambda: (rc.cyclic(21), gc.unit_vector(21, 0), 0.0, 0.0, 0, dict(maxiter=4), (4, 80)),
    "diag40_j0": lambda: _diag40(2.0) + (0.0, 0.0, 0, {}, (0, 1)),
    "diag40_j1": lambda: _diag40(2.0) + (0.0, 0.0, 1, {}, (0, 1)),
    "zero_rhs": lambda: (rc.banded(33), np.zeros(33, dtype=np.complex128), 0.0, 0.0, 0, {}, (0, 0)),
    "band_n255_w0_j0": lambda: (rc.banded(255, 1, 1.0), rc.real_vec(255, 255), 0.0, 0.0, 0, {}, None),
    "band_n257_w1_j1": lambda: (rc.banded(257, 1, 2.2), rc.real_vec(257, 257), 0.0, 0.0, 1, {}, None),
    "band_n1025_w1_j0": lambda: (rc.banded(1025, 1, 2.2), rc.real_vec(1025, 1025), 0.0, 0.0, 0, {}, None),
    "band_n1025_shift_psi_j1": lambda: (rc.banded(1025, 1, 1.0), rc.real_vec(1025, 1025), -0.25, 1e-3, 1, {}, None),
    "band_n300_negzero_shift": lambda: (rc.banded(300), rc.real_vec(7, 300), complex(0.5, -0.0), 1e-19, 0, {}, None),
    "band_n64_restart1": lambda: (rc.banded(64), rc.real_vec(64, 64), 0.0, 0.0, 0, dict(restart=1), None),
    "band_n64_restart5_j1": lambda: (rc.banded(64), rc.real_vec(64, 64), 0.0, 0.0, 1, dict(restart=5), None),
    "band_n64_maxiter1_restart4": lambda: (rc.banded(64), rc.real_vec(64, 64), 0.0, 0.0, 0, dict(restart=4, maxiter=1), (1, 4)),
    "tridiagonal_n513": lambda: (rc.tridiagonal(513), rc.real_vec(5, 513), 0.0, 1e-20, 0, {}, None),
    "five_point_n64": lambda: (rc.five_point(8), rc.real_vec(6, 64), 0.0, 1e-20, 1, {}, None),
    "small_n1": lambda: _small(1) + (0.0, 0.0, 0, {}, None),
    "small_n2_j1": lambda: _small(2) + (0.0, 0.0, 1, {}, None),
    "small_n5": lambda: _small(5) + (0.0, 0.0, 0, {}, None),
    "scale_up": lambda: (rc.banded(64), 1e120 * rc.real_vec(64, 64), 0.0, 0.0, 0, {}, None),
    "scale_down": lambda: (rc.banded(64), 1e-120 * rc.real_vec(64, 64), 0.0, 0.0, 0, {}, None),
}


@pytest.mark.parametrize("name", sorted(CLAIM))
def test_real_vectors_give_the_complex_bits(name):
    A, b, shift, psi, jac, kw, expect = CLAIM[name]()
    assert rc.flagged_real(A.data) and rc.flagged_real(b) and rc.flagged_real(np.array([shift], dtype=np.complex128))
    xc, info_c, inner_c, cycles_c = rc.restated(A, b, shift, psi, jac, np.complex128, **kw)
    xr, info_r, inner_r, cycles_r = rc.restated(A, b, shift, psi, jac, np.float64, **kw)
    assert xc.dtype == np.complex128 and xr.dtype == np.float64
    assert (info_r, inner_r, cycles_r) == (info_c, inner_c, cycles_c), name
    if expect is not None:
        assert (info_c, inner_c) == expect, name
    assert np.all(xc.imag == 0.0), name                                # the imaginary part never leaves zero
    assert np.array_equal(xr, xc.real), name                           # -0.0 == +0.0: the sign of a zero is not claimed
    nz = xr != 0.0
    assert np.array_equal(xr[nz].view(np.uint64), np.ascontiguousarray(xc.real[nz]).view(np.uint64)), name


def test_the_table_reaches_more_than_one_cycle_and_every_exit():
    seen = {"converged": 0, "maxiter": 0, "cycles>1": 0, "inner20": 0}
    for name in sorted(CLAIM):
        A, b, shift, psi, jac, kw, _ = CLAIM[name]()
        _, info, inner, cycles = rc.restated(A, b, shift, psi, jac, np.float64, **kw)
        seen["converged"] += info == 0
        seen["maxiter"] += info != 0
        seen["cycles>1"] += cycles > 1
        seen["inner20"] += inner == 20
    assert all(v > 0 for v in seen.values()), seen


def test_restatement_agrees_with_the_traced_reference():
    """restated() in complex128 is the algorithm of gmres_cases.traced (other summation orders): same exits and counts where no
    decision sits on its threshold, x to rounding."""
    A, b = rc.banded(257, 1, 2.2), rc.real_vec(257, 257)
    H = gc.sparse_h(A, 0.0, 0.0)
    ref = gc.traced(H, b, b, None)
    assert ref[4] >= gc.GUARD
    x, info, inner, cycles = rc.restated(A, b, 0.0, 0.0, 0, np.complex128)
    assert (info, inner, cycles) == (ref[1], ref[2], ref[3])
    assert np.linalg.norm(x - ref[0]) <= 1e-9 * np.linalg.norm(ref[0])


def test_a_real_division_would_not_give_the_complex_bits():
    """Why the one-lane state machine stays complex on the real path: NumPy (and the device's cdiv_np) divide by a complex number
    with imaginary part 0 as a multiplication by 1 / re, which differs from one real division in the last bit for some operands."""
    rng = np.random.default_rng(1)
    a, h = rng.standard_normal(4000), rng.standard_normal(4000) + 2.5
    smith = ((a + 0j) / (h + 0j)).real
    assert np.array_equal(smith, a * (1.0 / h))
    assert np.any(smith != a / h)
