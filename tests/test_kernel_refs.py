"""CPU tier for tests/kernel_refs.py: the checkers accept correct fp64 evaluations (4M and 3M emulated in NumPy, at the data
where the bound is tightest) and reject each planted error for the reason they are meant to.  The same checkers then run
against tests/fake_ctx.FakeContext where its NumPy arithmetic meets them, so that the test double and the device (the GPU
tier: test_gpu_zgemm_variants.py, test_gpu_vector_kernels.py) are held to one contract."""
import numpy as np
import pytest

import kernel_refs as kr
from fake_ctx import FakeContext


def mm3(A, Bm, conj_a=False, conj_b=False):
    """3M product in fp64 as the device kernels form it: P1 = ArBr, P2 = a_i' b_i', P3 = (Ar + a_i')(Br + b_i')."""
    ar, ai = A.real, (-A.imag if conj_a else A.imag)
    br, bi = Bm.real, (-Bm.imag if conj_b else Bm.imag)
    p1, p2, p3 = ar @ br, ai @ bi, (ar + ai) @ (br + bi)
    return (p1 - p2) + 1j * ((p3 - p1) - p2)


def mm4(A, Bm, conj_a=False, conj_b=False):
    return (A.conj() if conj_a else A) @ (Bm.conj() if conj_b else Bm)


CONJ = [(False, False), (True, False), (False, True), (True, True)]


# ---- exact operands --------------------------------------------------------------------------------------------------
def test_exact_operands_are_what_the_docstring_says():
    A, B = kr.exact_operands(70, 50, 1000, seed=3)
    for v in (A.real, A.imag, B.real, B.imag):
        assert np.array_equal(v, np.round(v)) and np.abs(v).max() <= 2 ** 10
        assert 0.2 < np.mean(v == 0) < 0.3 and (v > 0).any() and (v < 0).any()
    A1, B1 = kr.exact_operands(70, 50, 1000, seed=3, b_layout=1)
    assert B1.shape == (50, 1000) and np.array_equal(B1.T, B) and B1.flags.c_contiguous


@pytest.mark.parametrize("K", [60, 2 ** 14])
@pytest.mark.parametrize("ca,cb", CONJ)
@pytest.mark.parametrize("b_layout", [0, 1])
def test_exact_products_are_exact_in_any_evaluation(K, ca, cb, b_layout):
    """3M and 4M in fp64, BLAS order or reversed K: the same bits as the int64 matmul, at the largest K too."""
    A, B = kr.exact_operands(9, 7, K, seed=K, b_layout=b_layout)
    Bm = kr.as_math_b(B, b_layout)
    kr.check_exact(mm4(A, Bm, ca, cb), A, B, ca, cb, b_layout)
    kr.check_exact(mm3(A, Bm, ca, cb), A, B, ca, cb, b_layout)
    kr.check_exact(mm3(A[:, ::-1], Bm[::-1], ca, cb), A, B, ca, cb, b_layout)
    C0 = kr.exact_matrix(np.random.default_rng(1), 9, 7)
    kr.check_exact(C0 - mm3(A, Bm, ca, cb), A, B, ca, cb, b_layout, alpha=-1.0, C_in=C0)


def test_exact_check_rejects_planted_errors():
    A, B = kr.exact_operands(33, 40, 77, seed=5)
    good = mm4(A, B)
    kr.check_exact(good, A, B)
    with pytest.raises(AssertionError, match="integer reference"):        # K tail dropped
        kr.check_exact(mm4(A[:, :-1], B[:-1]), A, B)
    for ca, cb in CONJ[1:]:                                                # one or both conjugations missing / flipped
        with pytest.raises(AssertionError, match="integer reference"):
            kr.check_exact(good, A, B, ca, cb)
    with pytest.raises(AssertionError, match="integer reference"):        # the sign of P2 = Ai Bi alone (S2 of the DMA kernel)
        kr.check_exact((A.real @ B.real + A.imag @ B.imag) + 1j * good.imag, A, B)
    C0 = kr.exact_matrix(np.random.default_rng(2), 33, 40)
    with pytest.raises(AssertionError, match="integer reference"):        # beta ignored
        kr.check_exact(-good, A, B, alpha=-1.0, C_in=C0)
    with pytest.raises(AssertionError, match="integer reference"):        # alpha ignored
        kr.check_exact(C0 + good, A, B, alpha=-1.0, C_in=C0)
    stray = good.copy(); stray[32, 39] += 1.0                              # one stray write
    with pytest.raises(AssertionError, match=r"1 of 1320 entries.*\(32, 39\)"):
        kr.check_exact(stray, A, B)
    wrong_el = mm4(np.roll(A, 1, axis=1), B)                               # operand elements paired with the wrong k
    with pytest.raises(AssertionError, match="integer reference"):
        kr.check_exact(wrong_el, A, B)


# ---- derived bound ---------------------------------------------------------------------------------------------------
def _gauss(M, N, K, seed):
    return kr.gaussian_operands(M, N, K, seed)


@pytest.mark.parametrize("name,make,K,ceiling", [
    ("gaussian", _gauss, 64, 0.1), ("gaussian", _gauss, 8192, 1e-3),
    ("cancelling", kr.cancelling_operands, 4096, 1e-3),
    ("16 decades", lambda M, N, K, s: tuple(x * 10.0 ** np.random.default_rng(s + i).integers(-8, 9, size=x.shape)
                                            for i, x in enumerate(_gauss(M, N, K, s))), 1024, 0.1)])
def test_bound_accepts_fp64_3m_and_4m(name, make, K, ceiling):
    """A correct fp64 evaluation sits far inside the derived bound (the ceilings are a sanity check that the bound is not
    vacuous the other way: an evaluation that loses digits would have to lose several to reach it)."""
    A, B = make(24, 20, K, 11)
    prods = kr.real_products(A, B)
    for ca, cb in CONJ:
        for mm in (mm3, mm4):
            r = kr.check_within_bound(mm(A, B, ca, cb), A, B, ca, cb, products=prods)
            assert r < ceiling, (name, K, mm.__name__, r)
    C0 = A[:, :20] * 3.0
    kr.check_within_bound(C0 - mm3(A, B), A, B, alpha=-1.0, C_in=C0, products=prods)


def test_bound_rejects_planted_errors():
    A, B = _gauss(40, 30, 200, 7)
    prods = kr.real_products(A, B)
    good = mm3(A, B)
    assert kr.check_within_bound(good, A, B, products=prods) < 0.1
    lo = (A.astype(np.complex64) @ B.astype(np.complex64)).astype(np.complex128)          # fp32 accumulation
    with pytest.raises(AssertionError, match="derived bound") as e:
        kr.check_within_bound(lo, A, B, products=prods)
    assert float(str(e.value).split("=")[1].split()[0]) > 1e3
    with pytest.raises(AssertionError, match=r"1200 of 1200 entries"):                    # K tail dropped: every element
        kr.check_within_bound(mm3(A[:, :-1], B[:-1]), A, B, products=prods)
    with pytest.raises(AssertionError, match="derived bound"):                            # conjugation sign
        kr.check_within_bound(mm3(A, B, True, False), A, B, products=prods)
    with pytest.raises(AssertionError, match="derived bound"):                            # the sign of P2 alone
        kr.check_within_bound((A.real @ B.real + A.imag @ B.imag) + 1j * good.imag, A, B, products=prods)
    C0 = _gauss(40, 30, 1, 8)[0] @ np.ones((1, 30))
    with pytest.raises(AssertionError, match="derived bound"):                            # beta ignored
        kr.check_within_bound(-good, A, B, alpha=-1.0, C_in=C0, products=prods)
    with pytest.raises(AssertionError, match="non-finite"):
        bad = good.copy(); bad[3, 4] = np.nan
        kr.check_within_bound(bad, A, B, products=prods)
    with pytest.raises(AssertionError, match="4e-16"):
        kr.check_statistical(lo, A, B, products=prods)
    assert kr.check_statistical(good, A, B, products=prods) < 1.0


def test_reference_layouts_and_conjugations_agree_with_numpy():
    A, B1 = _gauss(13, 11, 37, 3)
    for bl in (0, 1):
        B = kr.store_b(B1, bl)
        for ca, cb in CONJ:
            re, im = kr.zgemm_reference(A, B, ca, cb, bl)
            ref = mm4(A, B1, ca, cb)
            assert np.allclose(re.astype(float), ref.real, rtol=0, atol=1e-12) and np.allclose(im.astype(float), ref.imag, rtol=0, atol=1e-12)


# ---- vector references -----------------------------------------------------------------------------------------------
def _vec(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def test_per_operation_references_against_python_scalars():
    """The references restate the kernels' operation order; here the same order once more in plain Python floats (IEEE
    double, one rounding per operation), element by element."""
    rng = np.random.default_rng(0)
    x, w, y = _vec(rng, 50), _vec(rng, 50), _vec(rng, 50)
    al, lam, sg = 0.3 - 0.8j, -1.7 + 0.4j, 2.5
    r = kr.relax_ref(x, w, al)
    d1, d3 = kr.eig_diff_ref(x, y, lam), kr.svd_diff_ref(y, x, sg)
    sc = kr.scale_ref(x, 3.7)
    for i in range(50):
        a, b = complex(x[i]), complex(w[i])
        omr, omi = 1.0 - al.real, -al.imag
        t1r, t1i = omr * a.real - omi * a.imag, omr * a.imag + omi * a.real
        t2r, t2i = al.real * b.real - al.imag * b.imag, al.real * b.imag + al.imag * b.real
        assert (r[i].real, r[i].imag) == (t1r + t2r, t1i + t2i)
        tr, ti = lam.real * a.real - lam.imag * a.imag, lam.real * a.imag + lam.imag * a.real
        assert (d1[i].real, d1[i].imag) == (y[i].real - tr, y[i].imag - ti)
        assert (d3[i].real, d3[i].imag) == (y[i].real - sg * a.real, y[i].imag - sg * a.imag)
        inv = 1.0 / 3.7
        assert (sc[i].real, sc[i].imag) == (a.real * inv, a.imag * inv)
    assert kr.same_bits(kr.linear_diff_ref(y, w), y - w)
    # special alphas: alpha = 0 leaves x (up to the sign of zeros), alpha = 1 gives w
    assert np.array_equal(kr.relax_ref(x, w, 0.0), x) and np.array_equal(kr.relax_ref(x, w, 1.0), w)


def test_bit_check_sees_one_ulp_and_signed_zero():
    v = np.array([1.0 + 2.0j, 0.0 + 0.0j, np.nan + 1j])
    kr.check_bits(v.copy(), v)
    w = v.copy(); w[0] = np.nextafter(1.0, 2.0) + 2.0j
    with pytest.raises(AssertionError, match="1 of 6 doubles"):
        kr.check_bits(w, v)
    z = v.copy(); z[1] = complex(-0.0, 0.0)
    with pytest.raises(AssertionError, match="differ in their bits"):
        kr.check_bits(z, v)
    # division instead of multiplication by the rounded reciprocal is a different rounding: the check tells them apart
    rng = np.random.default_rng(1)
    x = _vec(rng, 4096)
    true_div = (x.real / 3.7) + 1j * (x.imag / 3.7)
    assert not kr.same_bits(true_div, kr.scale_ref(x, 3.7))


@pytest.mark.parametrize("n", [1, 2, 257, 16385])
def test_norm_check_accepts_fp64_sums_and_rejects_a_missing_term(n):
    rng = np.random.default_rng(n)
    x = _vec(rng, n)
    f = x.view(np.float64)
    for got in (np.sqrt(np.sum(f * f)), np.linalg.norm(x), np.sqrt(np.sum((f * f)[::-1])), np.sqrt(np.cumsum(f * f)[-1])):
        assert kr.check_norm(got, x) <= 1.0
    # one term missing: the smallest |entry| that still matters at this n (relative weight ~ 1 / n of the sum of squares)
    y = x.copy(); k = n // 2
    y[k] = complex(0.0, y[k].imag) if n > 1 else 0.0
    if abs(x[k].real) ** 2 > 4 * (n + 2) * kr.U * np.linalg.norm(x) ** 2:
        with pytest.raises(AssertionError, match=r"\(n \+ 2\) u"):
            kr.check_norm(np.linalg.norm(y), x)
    with pytest.raises(AssertionError):
        kr.check_norm(np.float32(np.linalg.norm(x)) * (1 + 2.0 ** -20), x)            # single-precision result
    with pytest.raises(AssertionError, match="zero vector"):
        kr.check_norm(1e-300, np.zeros(n, complex))


def test_norm_check_rejects_one_missing_term_of_many():
    """n = 4097 equal entries: leaving out the last one (a loop that stops at a multiple of the block size) moves the norm by
    1 / (2n) relative, 1e11 times the bound."""
    x = np.full(4097, 1.0 + 1.0j)
    kr.check_norm(np.linalg.norm(x), x)
    with pytest.raises(AssertionError, match=r"\(n \+ 2\) u"):
        kr.check_norm(np.linalg.norm(x[:4096]), x)


def test_rayleigh_check():
    rng = np.random.default_rng(4)
    for n in (1, 65, 4097):
        x, y = _vec(rng, n), _vec(rng, n)
        xr, xi, yr, yi = x.real, x.imag, y.real, y.imag
        num = complex(np.sum(xr * yr + xi * yi), np.sum(xr * yi - xi * yr))
        den = complex(np.sum(xr * xr + xi * xi), 0.0)
        assert kr.check_rayleigh(num, den, x, y) <= 1.0
        with pytest.raises(AssertionError, match="not exactly 0.0"):
            kr.check_rayleigh(num, complex(den.real, 1e-300), x, y)
        with pytest.raises(AssertionError, match="not exactly 0.0"):
            kr.check_rayleigh(num, complex(den.real, -0.0), x, y)
        with pytest.raises(AssertionError, match="Rayleigh dots"):          # np.dot instead of np.vdot: no conjugation
            kr.check_rayleigh(np.dot(x, y), den, x, y)
        with pytest.raises(AssertionError, match="Rayleigh dots"):          # last term missing
            kr.check_rayleigh(num - np.conj(x[-1]) * y[-1], den, x, y)
        with pytest.raises(AssertionError, match="Rayleigh dots"):
            kr.check_rayleigh(np.complex64(num), den, x, y) if n > 1 else kr.check_rayleigh(num * (1 + 1e-7), den, x, y)


def test_argmax_check_first_index_and_nan():
    # |3 + 4i| = |-5| = 5: the first maximum is index 1
    s2 = np.array([1 + 0j, 3 + 4j, -5.0 + 0j])
    assert kr.argmax_ref(s2) == 1
    kr.check_argmax(1, s2)
    with pytest.raises(AssertionError, match="np.argmax gives 1"):          # last index of a tie
        kr.check_argmax(2, s2)
    t = np.array([1.0, 9.0, np.nan, 2.0, np.nan + 1j, 100.0], dtype=complex)
    assert kr.argmax_ref(t) == 2
    with pytest.raises(AssertionError, match="np.argmax gives 2"):          # NaN skipped (v > best is false for a NaN)
        kr.check_argmax(5, t)
    with pytest.raises(AssertionError, match="np.argmax gives 2"):          # last NaN
        kr.check_argmax(4, t)
    assert kr.argmax_ref(np.full(7, np.nan, dtype=complex)) == 0


# ---- the test double under the same checkers -------------------------------------------------------------------------
@pytest.fixture
def fake():
    rng = np.random.default_rng(9)
    n, P = 65, 6
    f = FakeContext()
    A = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / 8
    f.set_matrix(A)
    f.pop_reserve(P + 3)
    slots = [7, 0, 4, 2]
    X = np.array([_vec(rng, n) for _ in slots])
    W = np.array([_vec(rng, n) for _ in slots])
    f.pop_put(0, slots, X)
    f.pop_put(2, slots, W)
    return f, A, slots, X, W, rng


def test_fake_context_meets_the_reduction_bounds(fake):
    f, A, slots, X, W, rng = fake
    num, den = f.matvec_rayleigh(slots)
    for k in range(len(slots)):
        # judged on its own product, as the device is on its own Y.  (np.vdot(v, v).imag is not exactly 0.0 with every BLAS:
        # the exact-zero demand is the device kernel's, which never forms that part.)
        kr.check_rayleigh(num[k], complex(den[k].real, 0.0), X[k], A @ X[k])
    lam = np.array([_vec(rng, 1)[0] for _ in slots])
    res, fin = f.residual(1, slots, lam)
    for k in range(len(slots)):
        kr.check_norm(res[k], A @ X[k] - lam[k] * X[k])
    assert fin.all()
    nrm = f.relax_normalise(slots, np.full(len(slots), 0.25 + 0.5j), normalise=False)
    got = f.pop_get(0, slots, A.shape[0])
    for k in range(len(slots)):
        kr.check_norm(nrm[k], got[k])
    # the normalisation multiplies by the rounded reciprocal (NumPy's complex / real), as scale_ref and the kernels do.
    # (NumPy's complex PRODUCT is not held to relax_ref: its SIMD loops may fuse a multiply and an add.)
    f.pop_put(2, slots, got)                                      # w = x: (1 - a) x + a x with a = 1 is x itself
    nrm2 = f.relax_normalise(slots, np.ones(len(slots), complex), normalise=True)
    out = f.pop_get(0, slots, A.shape[0])
    for k in range(len(slots)):
        assert nrm2[k] == nrm[k]
        kr.check_bits(out[k], kr.scale_ref(got[k], nrm2[k]), "normalised x")


def test_fake_context_finite_flags_follow_x_only(fake):
    f, A, slots, X, W, rng = fake
    for bad in (np.nan, np.inf, -np.inf):
        Xb = X.copy(); Xb[2, 64] = bad
        f.pop_put(0, slots, Xb)
        res, fin = f.residual(1, slots, np.ones(len(slots), complex))
        assert list(fin) == list(np.isfinite(Xb).all(axis=1)) == [True, True, False, True]


def test_fake_context_argmax_is_first_index_and_first_nan():
    rng = np.random.default_rng(3)
    n = 40
    V = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    V[:, 31] = V[:, 5] = 50.0 * V[:, 17]                          # three identical columns, far above the rest
    f = FakeContext()
    f.set_matrix(np.eye(n, dtype=complex)); f.set_eigvecs(V); f.pop_reserve(3)
    x = V[:, 17].copy()
    f.pop_put(0, [1], x)
    idx, nrm = f.herm_match([1])
    kr.check_argmax(idx[0], x.conj() @ V)
    assert idx[0] == 5
    kr.check_norm(nrm[0], V[:, 5])
    Vn = V.copy(); Vn[3, 22] = np.nan; Vn[3, 9] = np.nan
    f.set_eigvecs(Vn); f.pop_put(0, [1], x)
    idx, _ = f.herm_match([1])
    kr.check_argmax(idx[0], x.conj() @ Vn)
    assert idx[0] == 9
