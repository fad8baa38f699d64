"""Inputs and the NumPy model of the band solves in real arithmetic (real_direct="on", maus_band_set_real; csrc/band.hip, DESIGN
§11 "Band solves in real arithmetic"), shared by tests/test_band_real_host.py on the CPU and tests/test_gpu_band_real.py on
the device.

The inputs are the real parts of tests/test_gpu_band.py's _band_case and tests/split_cases.py's band_case -- the same draws,
the same zero_cols -- as complex128 with imaginary bits +0.0.

The model restates zgbtf2 + zgbtrs once over the dtype with the device's operations: the pivot is the first maximum of
|re| + |im| (float64: |v|) with a NaN never winning, the reciprocal of the pivot is Smith's algorithm spelled out for complex128
and 1 / p for float64, the quotient of the back substitution likewise, and every element is changed by one multiply-subtract.
NumPy has no fused multiply-add, so the model rounds the product where the device does not, for both dtypes alike: it holds
the structure of the argument (the float64 text is the complex text without the terms that multiply an exact zero), not the
device's bits."""
import numpy as np

import split_cases as sc


def as_real(z):
    """Re z as complex128 with imaginary bits +0.0."""
    out = np.zeros(np.shape(z), dtype=np.complex128)
    out.real = np.asarray(z).real
    return out


def band_case(n, kl, ku, seed, zero_cols=()):
    """tests/test_gpu_band.py's _band_case, real parts: (A dense, ab in zgbtrf's layout, b)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    for d in range(-ku, kl + 1):
        m = n - abs(d)
        if m <= 0:
            continue
        v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        A += np.diag(v, -d)
    for j in zero_cols:
        A[:, j] = 0
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    A = as_real(A)
    return A, sc.to_band(A, kl, ku), as_real(b)


def split_case(n, kl, ku, seed, zero_cols=()):
    """tests/split_cases.py's band_case, real parts."""
    A, _, b = sc.band_case(n, kl, ku, seed, zero_cols)
    A = as_real(A)
    return A, sc.to_band(A, kl, ku), as_real(b)


def imag_bits_zero(x):
    """Every imaginary part has the bits of +0.0."""
    return not np.any(np.ascontiguousarray(np.asarray(x, dtype=np.complex128).imag).view(np.uint64))


# ---- the device's scalar operations, per dtype --------------------------------------------------------------------------------
def smith_recip(z):
    """1 / z as csrc/common.h's crecip on a complex128 scalar."""
    x, y = np.float64(z.real), np.float64(z.imag)
    if abs(x) >= abs(y):
        t = y / x
        d = x + y * t
        return complex(np.float64(1.0) / d, -t / d)
    t = x / y
    d = x * t + y
    return complex(t / d, np.float64(-1.0) / d)


def smith_div(a, b):
    """a / b as csrc/common.h's cdiv on complex128 scalars."""
    ax, ay, bx, by = (np.float64(v) for v in (a.real, a.imag, b.real, b.imag))
    if abs(bx) >= abs(by):
        t = by / bx
        d = bx + by * t
        return complex((ax + ay * t) / d, (ay - ax * t) / d)
    t = bx / by
    d = bx * t + by
    return complex((ax * t + ay) / d, (ay * t - ax) / d)


def _abs1(v):
    return np.abs(v.real) + np.abs(v.imag) if np.iscomplexobj(v) else np.abs(v)


def _recip(p):
    return smith_recip(complex(p)) if isinstance(p, (complex, np.complexfloating)) else np.float64(1.0) / np.float64(p)


def _div(a, b):
    return smith_div(complex(a), complex(b)) if isinstance(b, (complex, np.complexfloating)) else np.float64(a) / np.float64(b)


def _mul(a, b):
    """The device's cmul on an array a and a scalar b, component by component."""
    if np.iscomplexobj(a):
        b = complex(b)
        out = np.empty(a.shape, dtype=np.complex128)
        out.real = a.real * b.real - a.imag * b.imag
        out.imag = a.real * b.imag + a.imag * b.real
        return out
    return a * b


def _fms(a, l, u):
    """a - l u per element in the order of the device's cfms (products rounded: NumPy has no fma)."""
    if np.iscomplexobj(a):
        out = np.empty(np.broadcast(a, l, u).shape, dtype=np.complex128)
        out.real = (a.real - l.real * u.real) + l.imag * u.imag
        out.imag = (a.imag - l.real * u.imag) - l.imag * u.real
        return out
    return a - l * u


def lu_solve(ab, b, kl, ku):
    """zgbtf2 + zgbtrs as csrc/band.hip's column kernel runs them, on ab[2 kl + ku + 1, n] and b[n] of one dtype (complex128 or
    float64): (x, ipiv 0-based, info, the factored band)."""
    ab = np.array(ab)
    x = np.array(b)
    assert ab.dtype == x.dtype and ab.dtype in (np.complex128, np.float64)
    n, kv = ab.shape[1], kl + ku
    ipiv = np.zeros(n, dtype=np.int64)
    for j in range(ku + 1, min(kv, n)):
        ab[kv - j:kl, j] = 0
    ju = info = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            if j + kv < n:
                ab[:kl, j + kv] = 0
            km = min(kl, n - 1 - j)
            v = _abs1(ab[kv:kv + km + 1, j])
            jp = int(np.argmax(np.where(np.isnan(v), -1.0, v)))             # the first maximum; a NaN never wins
            piv = ab[kv + jp, j]
            ipiv[j] = j + jp
            if piv == 0:
                info = info or j + 1
                continue
            ju = max(ju, min(j + ku + jp, n - 1))
            if jp:
                for c in range(j, ju + 1):
                    r0, r1 = kv + j - c, kv + jp + j - c
                    ab[r0, c], ab[r1, c] = ab[r1, c], ab[r0, c]
                x[j], x[j + jp] = x[j + jp], x[j]
            if km > 0:
                l = _mul(ab[kv + 1:kv + km + 1, j], _recip(piv))
                ab[kv + 1:kv + km + 1, j] = l
                x[j + 1:j + km + 1] = _fms(x[j + 1:j + km + 1], l, x[j])
                for c in range(1, ju - j + 1):
                    ab[kv + 1 - c:kv + km + 1 - c, j + c] = _fms(ab[kv + 1 - c:kv + km + 1 - c, j + c], l, ab[kv - c, j + c])
        for j in range(n - 1, -1, -1):
            xj = x[j]
            if xj != 0:
                xj = _div(xj, ab[kv, j])
                lo = max(0, j - kv)
                x[lo:j] = _fms(x[lo:j], np.asarray(xj, dtype=x.dtype), ab[kv + lo - j:kv, j])
            x[j] = xj
    return x, ipiv, info, ab
