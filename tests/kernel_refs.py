"""References and checkers for the kernel-level tests -- TEST INFRASTRUCTURE, pure NumPy (no GPU import).

Three kinds of reference, each with the reason its verdict can be trusted:

  * exact: operands whose parts are small integers.  Every product and partial sum of a 3M or 4M evaluation is an integer below
    2^53, so the result is exact in ANY summation order and the reference is an int64 matmul: a wrong element, sign,
    conjugation, a missing K tail or a stray write is a bit difference.
  * bounded: np.longdouble references with A-PRIORI bounds (derived below, never measured on the code under test).
  * per operation: the element-wise kernels promise one rounding per __dmul_rn / __dadd_rn / __dsub_rn; the references below
    apply one NumPy float64 operation on separate real arrays for each of them (no complex arithmetic of NumPy's, whose
    rounding is NumPy's business), so they ARE the stated rounding and the comparison is bit for bit.

u = 2^-53 throughout.  Every check_* function raises AssertionError and returns the figure it judged (error / bound)."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------------------
# zgemm
# ---------------------------------------------------------------------------------------------------------------------
def as_math_b(B, b_layout):
    """B as the [K][N] matrix of the product, whatever its storage (b_layout 1: stored [N][K], dot-product form)."""
    return B.T if b_layout else B


def store_b(Bm, b_layout):
    """The stored operand for a [K][N] matrix Bm."""
    return np.ascontiguousarray(Bm.T) if b_layout else np.ascontiguousarray(Bm)


def exact_operands(M, N, K, seed, b_layout=0):
    """(A[M][K], B as stored) with integer parts |v| <= 2^10, about a quarter of them zero, mixed signs.  |(Ar+Ai)(Br+Bi)| <=
    2^22 per term, so every partial sum of a 3M or 4M evaluation stays below 2^36 < 2^53 for K <= 2^14."""
    assert K <= 2 ** 14
    rng = np.random.default_rng(seed)

    def part(*shape):
        v = rng.integers(-2 ** 10, 2 ** 10 + 1, size=shape)
        v[rng.random(shape) < 0.25] = 0
        return v.astype(np.float64)

    A = part(M, K) + 1j * part(M, K)
    Bm = part(K, N) + 1j * part(K, N)
    return A, store_b(Bm, b_layout)


def exact_matrix(rng, *shape):
    """Integer-valued complex array for the population-path products (|part| <= 16)."""
    return (rng.integers(-16, 17, size=shape) + 1j * rng.integers(-16, 17, size=shape)).astype(np.complex128)


def _combine(p, conj_a, conj_b):
    """op(A) op(B) from the four real products: conjugation only flips the sign of the operand's imaginary part."""
    sa, sb = (-1 if conj_a else 1), (-1 if conj_b else 1)
    return p["rr"] - (sa * sb) * p["ii"], sb * p["ri"] + sa * p["ir"]


def real_products(A, B, b_layout=0, dtype=LD):
    """ArBr, AiBi, ArBi, AiBr in `dtype`, computed once per operand pair (the long-double matmul is the expensive part)."""
    Bm = as_math_b(B, b_layout)
    ar, ai = np.ascontiguousarray(A.real, dtype=dtype), np.ascontiguousarray(A.imag, dtype=dtype)
    br, bi = np.ascontiguousarray(Bm.real, dtype=dtype), np.ascontiguousarray(Bm.imag, dtype=dtype)
    return {"rr": ar @ br, "ii": ai @ bi, "ri": ar @ bi, "ir": ai @ br}


def exact_reference(A, B, conj_a=False, conj_b=False, b_layout=0):
    """op(A) op(B) of integer-valued operands through int64 matmuls, as complex128 (exact)."""
    re, im = _combine(real_products(A, B, b_layout, dtype=np.int64), conj_a, conj_b)
    assert max(np.abs(re).max(), np.abs(im).max()) < 2 ** 53
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def zgemm_reference(A, B, conj_a=False, conj_b=False, b_layout=0, products=None):
    """(Re, Im) of op(A) op(B) in np.longdouble.  `products`: real_products(A, B, b_layout), to share them between the four
    conjugation combinations."""
    return _combine(products if products is not None else real_products(A, B, b_layout), conj_a, conj_b)


def zgemm_bound(A, B, K, b_layout=0):
    """A-priori bound on |fl(Re) - Re| and on |fl(Im) - Im| of alpha op(A) op(B), alpha = +-1:  2 (K + 8) u S,
    S = (|Ar| + |Ai|) @ (|Br| + |Bi|).

    4M: each part is a sum of 2K products accumulated in any order with one rounding per FMA: gamma_2K times the sum of the
    |products|, which is <= S.  3M: P1 = sum ArBr, P2 = sum AiBi, P3 = sum fl(Ar+Ai) fl(Br+Bi); the operand sums carry
    (1 + d)^2, P3's K-term accumulation gamma_K, and |Ar+Ai| |Br+Bi| summed is <= S, as are sum|ArBr| + sum|AiBi|; the two
    epilogue subtractions add 2u of at most 2S.  Together below (K + 2 + 2 + 4) u S (1 + O(u)) per part; the factor 2 covers
    gamma_k = k u / (1 - k u) and whichever order the MFMA adds its four products in.  Conjugation changes signs only."""
    Bm = as_math_b(B, b_layout)
    S = (np.abs(A.real) + np.abs(A.imag)) @ (np.abs(Bm.real) + np.abs(Bm.imag))
    return 2.0 * (K + 8) * U * S


def check_exact(C, A, B, conj_a=False, conj_b=False, b_layout=0, alpha=1.0, C_in=None):
    """Integer operands (and integer C_in): alpha op(A) op(B) + C_in must come back bit for bit."""
    ref = alpha * exact_reference(A, B, conj_a, conj_b, b_layout)
    if C_in is not None:
        ref = ref + C_in
    ref = ref + 0.0                                           # -0.0 of the reference's sign algebra -> +0.0
    if not np.array_equal(C + 0.0, ref):
        bad = np.argwhere(C + 0.0 != ref)
        i, j = bad[0]
        raise AssertionError(f"{len(bad)} of {C.size} entries differ from the integer reference, first at ({i}, {j}): "
                             f"got {C[i, j]!r}, expected {ref[i, j]!r}")
    return 0.0


def check_within_bound(C, A, B, conj_a=False, conj_b=False, b_layout=0, alpha=1.0, C_in=None, products=None):
    """|C - (alpha op(A) op(B) + C_in)| within zgemm_bound per part (+ u |result| for the rounding of the beta = 1 add).
    Returns the largest error / bound."""
    K = A.shape[1]
    re, im = zgemm_reference(A, B, conj_a, conj_b, b_layout, products)
    re, im = LD(alpha) * re, LD(alpha) * im
    bound = zgemm_bound(A, B, K, b_layout)
    if C_in is not None:
        re, im = re + C_in.real, im + C_in.imag
        bound = bound + U * np.maximum(np.abs(re), np.abs(im)).astype(np.float64)
    err = np.maximum(np.abs(C.real - re), np.abs(C.imag - im)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    if not np.all(np.isfinite(C.view(np.float64))):
        raise AssertionError("non-finite entries in the product of finite operands")
    worst = float(ratio.max())
    if not worst <= 1.0:
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"error / derived bound = {worst:.3g} at ({i}, {j}); {int((ratio > 1).sum())} of {ratio.size} "
                             f"entries exceed the bound 2 (K + 8) u S, K = {K}")
    return worst


def check_statistical(C, A, B, conj_a=False, conj_b=False, b_layout=0, products=None):
    """The form the project's existing tests assert: |C - ref| / (|A| @ |B|) < 4e-16 max(4, sqrt(K)).  Returns measured /
    allowed."""
    K = A.shape[1]
    re, im = zgemm_reference(A, B, conj_a, conj_b, b_layout, products)
    err = np.hypot((C.real - re).astype(np.float64), (C.imag - im).astype(np.float64))
    scale = np.abs(A) @ np.abs(as_math_b(B, b_layout))
    worst = float(np.max(err / scale)) / (4e-16 * max(4.0, np.sqrt(K)))
    if not worst < 1.0:
        raise AssertionError(f"|C - ref| / (|A| @ |B|) is {worst:.3g} times 4e-16 max(4, sqrt(K)), K = {K}")
    return worst


def gaussian_operands(M, N, K, seed, b_layout=0):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) + 1j * rng.standard_normal((M, K))
    Bm = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    return A, store_b(Bm, b_layout)


def cancelling_operands(M, N, K, seed, b_layout=0):
    """Ar = -Ai and Br = -Bi up to 1e-9: the 3M operand sums Ar + Ai, Br + Bi cancel to nine digits."""
    rng = np.random.default_rng(seed)
    ar, br = rng.standard_normal((M, K)), rng.standard_normal((K, N))
    A = ar + 1j * (-ar + 1e-9 * rng.standard_normal((M, K)))
    Bm = br + 1j * (-br + 1e-9 * rng.standard_normal((K, N)))
    return A, store_b(Bm, b_layout)


# ---------------------------------------------------------------------------------------------------------------------
# per-candidate vector kernels: per-operation references (float64, one NumPy operation per rounding of the kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _parts(v):
    v = np.asarray(v, dtype=np.complex128)
    return np.ascontiguousarray(v.real), np.ascontiguousarray(v.imag)


def _cplx(re, im):
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def _cmul(pr, pi, ar, ai):
    """(pr + i pi)(ar + i ai): each real product rounded, then the difference / sum."""
    return pr * ar - pi * ai, pr * ai + pi * ar


def relax_ref(x, w, alpha):
    """fl((1 - alpha) x) + fl(alpha w) as relax_normalise_kernel rounds it."""
    xr, xi = _parts(x)
    wr, wi = _parts(w)
    al = np.complex128(alpha)
    omr, omi = np.float64(1.0) - al.real, -al.imag
    t1r, t1i = _cmul(omr, omi, xr, xi)
    t2r, t2i = _cmul(al.real, al.imag, wr, wi)
    return _cplx(t1r + t2r, t1i + t2i)


def scale_ref(v, nrm):
    """v * fl(1 / nrm): the kernels multiply by the rounded reciprocal."""
    vr, vi = _parts(v)
    inv = np.float64(1.0) / np.float64(nrm)
    return _cplx(vr * inv, vi * inv)


def eig_diff_ref(x, y, lam):
    """y - fl(lam x), residual_kernel kind 1."""
    xr, xi = _parts(x)
    yr, yi = _parts(y)
    l = np.complex128(lam)
    tr, ti = _cmul(l.real, l.imag, xr, xi)
    return _cplx(yr - tr, yi - ti)


def linear_diff_ref(y, b):
    yr, yi = _parts(y)
    br, bi = _parts(b)
    return _cplx(yr - br, yi - bi)


def svd_diff_ref(y, u, sigma):
    """y - fl(sigma u) with the real sigma of svd_resid_kernel."""
    yr, yi = _parts(y)
    ur, ui = _parts(u)
    s = np.float64(sigma)
    return _cplx(yr - s * ur, yi - s * ui)


def same_bits(a, b):
    """Bit equality of two complex / real arrays (NaNs compare by payload-free value: NaN == NaN here, -0.0 != 0.0)."""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    fa, fb = a.view(np.float64), b.view(np.float64)
    nan = np.isnan(fa) & np.isnan(fb)
    return bool(np.all((fa.view(np.int64) == fb.view(np.int64)) | nan))


def check_bits(got, ref, what="values"):
    if not same_bits(got, ref):
        if np.shape(got) != np.shape(ref):
            raise AssertionError(f"{what}: shape {np.shape(got)} against {np.shape(ref)}")
        g = np.ascontiguousarray(got).view(np.float64).ravel()
        r = np.ascontiguousarray(ref).view(np.float64).ravel()
        bad = np.flatnonzero((g.view(np.int64) != r.view(np.int64)) & ~(np.isnan(g) & np.isnan(r)))
        k = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} doubles differ in their bits from the per-operation reference, "
                             f"first at {k}: got {g[k]!r}, expected {r[k]!r}")
    return 0.0


# ---- reductions: long-double references and a-priori bounds (any summation order) -----------------------------------
def norm_ref(v):
    vr, vi = _parts(v)
    vr, vi = vr.astype(LD), vi.astype(LD)
    return np.sqrt(np.sum(vr * vr + vi * vi))


def check_norm(got, v, what="norm"):
    """|got - ||v||| <= (n + 2) u ||v||: the sum of 2n squares by FMAs in any order has relative error gamma_2n (all terms
    are >= 0, so there is no cancellation), the square root halves it and adds one rounding.  Returns error / bound."""
    n = np.size(v)
    ref = norm_ref(v)
    got = np.float64(got)
    if ref == 0:
        if got != 0.0:
            raise AssertionError(f"{what}: {got!r} for a zero vector")
        return 0.0
    ratio = float(abs(LD(got) - ref) / ((n + 2) * U * ref))
    if not ratio <= 1.0:
        raise AssertionError(f"{what}: got {got!r}, long-double reference {float(ref)!r}: error is {ratio:.3g} times (n + 2) u, n = {n}")
    return ratio


def rayleigh_ref(x, y):
    """(num, den) = (sum conj(x) y, sum conj(x) x) as (re, im) pairs of long doubles."""
    xr, xi = (p.astype(LD) for p in _parts(x))
    yr, yi = (p.astype(LD) for p in _parts(y))
    return (np.sum(xr * yr + xi * yi), np.sum(xr * yi - xi * yr)), (np.sum(xr * xr + xi * xi), LD(0))


def rayleigh_bound(x, y):
    """(2n + 2) u sum (|xr| + |xi|)(|yr| + |yi|) per part: 2n FMA roundings in any order (gamma_2n) on terms whose absolute
    values sum to at most that, plus the block reduction's adds counted in the + 2."""
    xr, xi = _parts(x)
    yr, yi = _parts(y)
    return (2 * np.size(x) + 2) * U * float(np.sum((np.abs(xr) + np.abs(xi)).astype(LD) * (np.abs(yr) + np.abs(yi))))


def check_rayleigh(num, den, x, y):
    """num, den of matvec_rayleigh against the bounds; den.imag must be exactly 0.0.  Returns the largest error / bound."""
    (nr, ni), (dr, _) = rayleigh_ref(x, y)
    bn, bd = rayleigh_bound(x, y), rayleigh_bound(x, x)
    num, den = np.complex128(num), np.complex128(den)
    if not (den.imag == 0.0 and not np.signbit(den.imag)):
        raise AssertionError(f"den.imag is {den.imag!r}, not exactly 0.0")
    errs = [abs(LD(num.real) - nr) / bn if bn else abs(LD(num.real) - nr), abs(LD(num.imag) - ni) / bn if bn else abs(LD(num.imag) - ni),
            abs(LD(den.real) - dr) / bd if bd else abs(LD(den.real) - dr)]
    worst = float(max(errs))
    if not worst <= 1.0:
        raise AssertionError(f"Rayleigh dots: error / bound = {[float(e) for e in errs]} (num.re, num.im, den), n = {np.size(x)}")
    return worst


def argmax_ref(scores):
    """np.argmax(np.abs(scores)): the first maximum, and the first NaN as soon as one score is NaN (AMS:169)."""
    return int(np.argmax(np.abs(np.asarray(scores, dtype=np.complex128))))


def check_argmax(idx, scores):
    want = argmax_ref(scores)
    if int(idx) != want:
        a = np.abs(np.asarray(scores, dtype=np.complex128))
        raise AssertionError(f"arg-max {int(idx)} (|score| {a[int(idx)]!r}), np.argmax gives {want} (|score| {a[want]!r})")
    return 0.0
