"""real_direct="on" without a device (csrc/band.hip, DESIGN §11 "Band solves in real arithmetic"): the keyword and
MAUS_REAL_DIRECT, the rule's share that needs no device (maus_band_real_kinds: which plans have real kernels), and the claim
the real path rests on, restated in NumPy -- zgbtf2 + zgbtrs on a real band run on float64 (the terms that multiply an exact
zero removed, one division where Smith's algorithm takes three) returns the x, ipiv and info of the same text run on
complex128."""
import numpy as np
import pytest

import band_real_cases as brc


# ---- keyword and environment ------------------------------------------------------------------------------------------------
def test_keyword_values_and_environment(monkeypatch):
    from adaptive_matrix_solver_amd import engine
    monkeypatch.delenv("MAUS_REAL_DIRECT", raising=False)
    assert engine.REAL_DIRECT_MODES == ("auto", "off", "on")
    assert engine.real_direct_mode(None) == "auto"
    for m in engine.REAL_DIRECT_MODES:
        assert engine.real_direct_mode(m) == m
    for bad in ("ON", "real", "", "1", True):
        with pytest.raises(ValueError, match="real_direct must be one of"):
            engine.real_direct_mode(bad)
    monkeypatch.setenv("MAUS_REAL_DIRECT", "on")
    assert engine.real_direct_mode(None) == "on"
    assert engine.real_direct_mode("off") == "off"                     # the keyword wins
    monkeypatch.setenv("MAUS_REAL_ARITH", "off")                       # the two switches do not read each other's variable
    assert engine.real_direct_mode(None) == "on" and engine.real_arith_mode(None) == "off"
    monkeypatch.setenv("MAUS_REAL_DIRECT", "yes")
    with pytest.raises(ValueError, match="real_direct must be one of"):
        engine.real_direct_mode(None)


def test_keyword_reaches_the_solvers(monkeypatch):
    """MAUS_Solver and InverseIterateSolver validate the keyword before they touch a device."""
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver, MAUS_Solver, ProblemType
    monkeypatch.delenv("MAUS_REAL_DIRECT", raising=False)
    s = InverseIterateSolver(8, 1e-20, 2, real_direct="on")
    assert s.real_direct == "on" and s.real_arith == "auto"            # independent of real_arith
    assert InverseIterateSolver(8, 1e-20, 2, real_arith="on").real_direct == "auto"
    with pytest.raises(ValueError, match="real_direct"):
        InverseIterateSolver(8, 1e-20, 2, real_direct="maybe")
    with pytest.raises(ValueError, match="real_direct"):
        MAUS_Solver(np.eye(4), ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=np.ones(4), real_direct="maybe")


def test_binding_constants():
    from adaptive_matrix_solver_amd import _cabi
    assert (_cabi.BAND_REAL_OFF, _cabi.BAND_REAL_ON) == (0, 1)
    assert (_cabi.BAND_REAL_OK, _cabi.BAND_REAL_MODE_OFF, _cabi.BAND_REAL_NOT_CSR, _cabi.BAND_REAL_MATRIX_COMPLEX,
            _cabi.BAND_REAL_RHS_ROWS, _cabi.BAND_REAL_RHS_COMPLEX, _cabi.BAND_REAL_SHIFT_COMPLEX,
            _cabi.BAND_REAL_NO_KERNELS) == tuple(range(8))
    assert _cabi.KC_BAND_REAL == 21 and (_cabi.KC_GMRES_REAL, _cabi.KC_SPMM_REAL) == (19, 20)     # appended behind the others


# ---- which plans have real kernels --------------------------------------------------------------------------------------------
SHAPES = [(0, 0), (15, 16), (16, 1), (15, 17), (0, 32), (100, 5)]


@pytest.mark.parametrize("kl,ku", SHAPES)
def test_band_real_kinds_on_both_sides_of_every_boundary(kl, ku):
    """Real kernels exist for the column kernel and the narrow method, for the band itself or -- where the split takes it --
    for its reduced system.  The expectation is put together from the Python restatement of the plans (band.py)."""
    from adaptive_matrix_solver_amd import _cabi
    from adaptive_matrix_solver_amd import band as bp
    has_real = (_cabi.BAND_COLUMN, _cabi.BAND_NARROW)
    w = kl + ku
    for method in (_cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE, _cabi.BAND_NARROW):
        kind = bp.kernel_for(method, kl, ku)[0]
        assert kind == _cabi.band_plan(method, 5000, kl, ku)[0]
        # the split off: the method's plan alone, at any n
        for n in (1, 70, 5000):
            assert _cabi.band_real_kinds(method, False, 0, n, kl, ku) == (kind in has_real, kind, False)
        # the split on: the rule's partition length, a forced one, and n <= m where the split does not take the band
        for part_len, n in ((0, 5000), (2 * w + 2, 5 * (2 * w + 2) + 3), (2 * w + 2, 2 * w + 3), (2 * w + 2, 2 * w + 2), (64, 64),
                            (64, 65) if 64 >= 2 * w + 2 else (0, 63)):
            takes = bp.runs_split(n, kl, ku, part_len)
            assert takes == _cabi.band_split_plan(method, n, kl, ku, part_len)[0]
            if takes:
                _, _, klr, kur = bp.split_shape(n, kl, ku, part_len)
                rkind = bp.kernel_for(method, klr, kur)[0]
                assert _cabi.band_real_kinds(method, True, part_len, n, kl, ku) == (rkind in has_real, kind, True)
            else:
                assert _cabi.band_real_kinds(method, True, part_len, n, kl, ku) == (kind in has_real, kind, False)


def test_band_real_kinds_verdicts_by_name():
    """The verdicts spelled out where the boundaries lie: kl = 15 / 16 (narrow, blocked), kl + ku = 31 / 32 (narrow, split), and the
    reduced system of a split (15, 16) band, which is 45 wide: real under the column kernel, complex under blocked."""
    from adaptive_matrix_solver_amd import _cabi
    C, B, T, W, N = _cabi.BAND_COLUMN, _cabi.BAND_BLOCKED, _cabi.BAND_TILED, _cabi.BAND_WIDE, _cabi.BAND_NARROW
    k = _cabi.band_real_kinds
    assert k(N, False, 0, 5000, 15, 16) == (True, N, False) and k(N, False, 0, 5000, 15, 17) == (True, C, False)
    assert k(N, False, 0, 5000, 16, 1) == (True, C, False) and k(B, False, 0, 5000, 16, 1) == (False, B, False)
    assert k(B, False, 0, 5000, 15, 16) == (True, C, False) and k(T, False, 0, 5000, 100, 5) == (False, T, False)
    assert k(W, False, 0, 5000, 100, 5) == (False, W, False) and k(W, False, 0, 5000, 16, 1) == (False, T, False)
    assert k(C, True, 0, 5000, 15, 16) == (True, C, True) and k(B, True, 0, 5000, 15, 16) == (False, C, True)
    assert k(N, True, 0, 5000, 1, 1) == (True, N, True) and k(N, True, 0, 5000, 0, 0) == (True, N, False)
    assert k(N, True, 0, 5000, 0, 32) == (True, C, False) and k(B, True, 0, 5000, 0, 32) == (True, C, False)
    for bad in ((3, False, 0, 10, 1, 1), (C, True, 3, 100, 1, 1), (C, False, 0, 10, -1, 1), (C, False, -1, 10, 1, 1)):
        with pytest.raises(_cabi.MausHipError):
            k(*bad)


# ---- the claim, in NumPy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl,ku", [(1, 1), (3, 2), (0, 4), (15, 16)])
@pytest.mark.parametrize("n", [1, 5, 33, 65])
def test_float64_restatement_returns_the_complex_restatements_values(n, kl, ku):
    for zero_cols in ((), (min(3, n - 1),)):                           # one singular column
        _, ab, b = brc.band_case(n, kl, ku, 7 + n + kl, zero_cols)
        assert brc.imag_bits_zero(ab) and brc.imag_bits_zero(b)
        xc, pc, ic, fc = brc.lu_solve(ab, b, kl, ku)
        xr, pr, ir, fr = brc.lu_solve(ab.real.copy(), b.real.copy(), kl, ku)
        assert ir == ic and np.array_equal(pr, pc)
        assert ic == (zero_cols[0] + 1 if zero_cols else 0)
        assert np.array_equal(fr, fc.real) and not np.any(fc.imag)     # the elimination never divides by the zero pivot
        if ic == 0:                                                     # past a zero pivot x is NaN (Smith's 0 / 0) or Inf (1 / 0)
            assert np.all(np.isfinite(xc)) and np.array_equal(xr, xc.real) and not np.any(xc.imag)


def test_float64_restatement_solves_the_system():
    """The model is a solver, not only two texts that agree: against numpy.linalg.solve to the system's condition."""
    A, ab, b = brc.split_case(65, 3, 2, 5)
    x, _, info, _ = brc.lu_solve(ab.real.copy(), b.real.copy(), 3, 2)
    assert info == 0
    xr = np.linalg.solve(A.real, b.real)
    assert np.linalg.norm(x - xr) <= 64 * np.finfo(np.float64).eps * np.linalg.cond(A.real) * np.linalg.norm(xr)


def test_smiths_reciprocal_and_quotient_of_real_operands_are_one_division():
    """crecip / cdiv with an imaginary part of +-0 against 1 / p and a / p: 10^4 random doubles over the whole exponent range,
    subnormals among them, bit for bit in the real part, an exact zero in the imaginary part."""
    rng = np.random.default_rng(2024)
    bits = rng.integers(0, 1 << 63, 10000, dtype=np.uint64) | (rng.integers(0, 2, 10000, dtype=np.uint64) << np.uint64(63))
    p = bits.view(np.float64)
    p = p[np.isfinite(p) & (p != 0)]
    p[:200] = np.float64(5e-324) * rng.integers(1, 1 << 40, 200)       # subnormals
    a = rng.standard_normal(p.size) * np.exp2(rng.integers(-500, 500, p.size))
    assert np.sum(np.abs(p) < np.finfo(np.float64).tiny) >= 200
    with np.errstate(all="ignore"):
        for k in range(p.size):
            for im in (0.0, -0.0):
                r = brc.smith_recip(complex(p[k], im))
                q = brc.smith_div(complex(a[k], im), complex(p[k], -im))
                one, quo = np.float64(1.0) / p[k], a[k] / p[k]
                assert np.array_equal(np.float64(r.real).view(np.uint64), one.view(np.uint64)) and r.imag == 0.0, (k, p[k], r)
                assert np.array_equal(np.float64(q.real).view(np.uint64), np.float64(quo).view(np.uint64)) and q.imag == 0.0, (k, q)
