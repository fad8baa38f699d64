"""Cases, references and checks for the stages of the Hermitian reduction (csrc/herm.hip: maus_herm_tridiag and the Q that
maus_herm_backtransform(I) returns), importable without a GPU.  A "reducer" is any callable A, chunk -> (d, e, Q) with
A_L = Q T Q^H for the Hermitian matrix A_L of A's lower triangle and real diagonal, T = tridiag(e, d, e), LAPACK's zhetrd('L')
conventions.  tests/test_herm_cases_host.py runs the table through LAPACK and through the NumPy restatement below (which
must fail the checks under seven planted faults); tests/test_gpu_herm_reduction.py runs it through the device.

Check A (extended precision, O(k n^2)): with k = 8 complex Gaussian probe columns X in np.clongdouble,
    r = ||A_L X - Q (T (Q^H X))||_F / (||A||_2 ||X||_F),        u = ||Q (Q^H X) - X||_F / ||X||_F,
each at most 8 x max(LAPACK's value on the same matrix and probes, eps): both are backward-stable Householder reductions that
differ in the order of summation, eps is the rounding of storing Q and T, and one wrong entry of A moves r by ~1 / n^1.5.
Check B (conventions): Q e_1 = e_1 and e_1^T Q = e_1^T exactly, d[0] = Re A[0, 0] exactly, e[0] = -copysign(||A[1:, 0]||, Re A[1, 0])
within 4 ulps, e real and finite."""
import functools
import math

import numpy as np
from scipy.linalg import lapack

import scenarios

EPS = float(np.finfo(np.float64).eps)
NPROBE = 8
BOUND = 8.0                                   # check A: times max(LAPACK's value, eps)
TILE = 64                                     # tile edge of the device's matvec = panel width = reflectors per block
LD, CLD = np.longdouble, np.clongdouble

# LAPACK's own check-A values on random Hermitian matrices (scenarios.hermitian(n, n), probe seed 1), in units of eps:
# n -> (r / eps, u / eps).  test_herm_cases_host.py recomputes them and holds them within a factor of two.
LAPACK_RECORDED = {65: (2.7, 3.4), 200: (3.4, 4.3), 600: (4.5, 5.1), 1100: (5.6, 5.9), 2100: (7.5, 7.2)}

RANDOM_SIZES = (1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 191, 193, 257, 321, 1089)
# the smallest orders at which a block row of the tile grid has two chunks: (tiles per workgroup, n)
FORCED = ((8, 600), (8, 577), (16, 1100), (16, 1089))
SCALES = (2.0 ** -300, 2.0 ** 300, 2.0 ** -560, 2.0 ** 560)


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def lower_hermitian(A):
    """What zhetrd('L') sees: the lower triangle, its mirror image, the real part of the diagonal."""
    L = np.tril(A, -1)
    return L + L.conj().T + np.diag(A.diagonal().real).astype(np.complex128)


def _block_diag(sizes, seed):
    n = sum(sizes)
    A = np.zeros((n, n), dtype=np.complex128)
    o = 0
    for k, s in enumerate(sizes):
        A[o:o + s, o:o + s] = scenarios.hermitian(s, seed + k)
        o += s
    return A


def _complex_tridiagonal(n, seed):
    rng = np.random.default_rng(seed)
    dd = rng.standard_normal(n)
    ee = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    return np.diag(dd).astype(np.complex128) + np.diag(ee, -1) + np.diag(ee.conj(), 1)


def _arrowhead(n, seed):
    rng = np.random.default_rng(seed)
    A = np.diag(rng.standard_normal(n)).astype(np.complex128)
    c = rng.standard_normal(n - 1) + 1j * rng.standard_normal(n - 1)
    A[1:, 0] = c
    A[0, 1:] = c.conj()
    return A


def _real_symmetric(n, seed):
    B = np.random.default_rng(seed).standard_normal((n, n))
    return ((B + B.T) / 2.0).astype(np.complex128)


def dirty_upper(A):
    """A with everything zhetrd('L') must not read set to NaN: the strict upper triangle and the imaginary diagonal."""
    B = A.copy()
    B[np.triu_indices(A.shape[0], 1)] = complex(np.nan, np.nan)
    dg = A.diagonal().copy()
    dg.imag = np.nan
    B[np.diag_indices(A.shape[0])] = dg
    return B


# name -> (kind, builder, extra).  Structured cases span more than one 64-column panel.
CASES = {}
for _n in RANDOM_SIZES:
    CASES[f"random_n{_n}"] = ("random", functools.partial(scenarios.hermitian, _n, _n), None)
for _h, _n in FORCED:
    CASES[f"chunk{_h}_n{_n}"] = ("random", functools.partial(scenarios.hermitian, _n, _n), _h)
CASES["block_diag_mid"] = ("block_diag", functools.partial(_block_diag, (70, 60, 70), 300), (70, 130))
CASES["block_diag_edge"] = ("block_diag", functools.partial(_block_diag, (64, 64, 72), 310), (64, 128))
CASES["complex_tridiagonal"] = ("complex_tridiagonal", functools.partial(_complex_tridiagonal, 200, 4), None)
CASES["arrowhead"] = ("arrowhead", functools.partial(_arrowhead, 200, 5), None)
CASES["real_symmetric"] = ("real_symmetric", functools.partial(_real_symmetric, 200, 6), None)
CASES["lower_only"] = ("lower_only", functools.partial(scenarios.hermitian, 200, 77), None)
CASES["scaled"] = ("scaled", functools.partial(scenarios.hermitian, 130, 91), None)
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = CASES[name][1]()
    A.setflags(write=False)
    return A


# ---- the reference: LAPACK on the host -------------------------------------------------------------------------------------------
def lapack_reduce(A, chunk=0):
    """zhetrd(lower) and Q = H(0) .. H(n-2) from zungqr on the reflector block."""
    n = A.shape[0]
    c, d, e, tau, info = lapack.zhetrd(np.array(A, dtype=np.complex128, order="F"), lower=1)
    assert info == 0
    Q = np.eye(n, dtype=np.complex128)
    if n > 1:
        q, _, info = lapack.zungqr(np.asfortranarray(c[1:, : n - 1]), tau)
        assert info == 0
        Q[1:, 1:] = q
    return d, e, Q


# ---- check A ----------------------------------------------------------------------------------------------------------------------
def _fro(M):
    M = np.asarray(M, dtype=CLD)
    return float(np.sqrt(np.sum(M.real.astype(LD) ** 2 + M.imag.astype(LD) ** 2)))


class Probe:
    """The matrix-only half of check A: the probes, A_L X in extended precision, ||A||_2."""

    def __init__(self, A, seed=1):
        n = A.shape[0]
        rng = np.random.default_rng(seed)
        self.X = (rng.standard_normal((n, NPROBE)) + 1j * rng.standard_normal((n, NPROBE))).astype(CLD)
        AL = lower_hermitian(A)
        self.AX = AL.astype(CLD) @ self.X
        self.anorm = float(np.abs(np.linalg.eigvalsh(AL)).max())
        self.xnorm = _fro(self.X)

    def values(self, d, e, Q):
        """(r, u) of a decomposition."""
        Ql = np.asarray(Q).astype(CLD)
        Y = Ql.conj().T @ self.X
        TY = np.asarray(d, dtype=LD)[:, None] * Y
        if len(d) > 1:
            el = np.asarray(e, dtype=LD)[:, None]
            TY[1:] += el * Y[:-1]
            TY[:-1] += el * Y[1:]
        r = _fro(self.AX - Ql @ TY) / (max(self.anorm, np.finfo(np.float64).tiny) * self.xnorm)
        u = _fro(Ql @ Y - self.X) / self.xnorm
        return r, u


@functools.lru_cache(maxsize=None)
def probe_and_lapack(name):
    """(Probe, LAPACK's (r, u)) of a case's matrix: computed once, shared by every test on that matrix."""
    A = matrix(name)
    p = Probe(A)
    return p, p.values(*lapack_reduce(A))


def check_a(name, d, e, Q):
    """Asserts check A; returns (r / eps, u / eps, r / LAPACK's r, u / LAPACK's u) for the record."""
    p, (r0, u0) = probe_and_lapack(name)
    r, u = p.values(d, e, Q)
    rec = (r / EPS, u / EPS, r / max(r0, EPS), u / max(u0, EPS))
    print(f"CHECK_A {name}: r = {rec[0]:.2f} eps ({rec[2]:.2f} x LAPACK's {r0 / EPS:.2f}), u = {rec[1]:.2f} eps ({rec[3]:.2f} x LAPACK's {u0 / EPS:.2f})")
    assert np.isfinite(r) and r <= BOUND * max(r0, EPS), f"{name}: r = {r / EPS:.3g} eps, LAPACK {r0 / EPS:.3g} eps"
    assert np.isfinite(u) and u <= BOUND * max(u0, EPS), f"{name}: u = {u / EPS:.3g} eps, LAPACK {u0 / EPS:.3g} eps"
    return rec


# ---- check B ----------------------------------------------------------------------------------------------------------------------
def within_ulps(x, ref, k):
    ref = np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(np.asarray(x, dtype=np.float64) - ref) <= k * np.spacing(np.abs(ref))))


def check_b(A, d, e, Q):
    n = A.shape[0]
    assert d.shape == (n,) and e.shape == (max(n - 1, 0),) and Q.shape == (n, n)
    e1 = np.zeros(n, dtype=np.complex128)
    e1[0] = 1.0
    assert np.array_equal(Q[0, :], e1), "first row of Q is not e_1^T"
    assert np.array_equal(Q[:, 0], e1), "Q e_1 is not e_1"
    assert d[0] == A[0, 0].real
    assert np.isrealobj(e) and np.isfinite(e).all() and np.isfinite(d).all()
    if n > 1:
        alpha, x = A[1, 0], A[2:, 0]
        if not x.any() and alpha.imag == 0.0:                   # zlarfg: H = I, beta = alpha
            assert e[0] == alpha.real
        else:
            c = A[1:, 0].astype(CLD)
            nrm = float(np.sqrt(np.sum(c.real ** 2 + c.imag ** 2)))
            assert within_ulps(e[0], -math.copysign(nrm, alpha.real), 4), (e[0], -math.copysign(nrm, alpha.real))


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---- one case against one reducer ---------------------------------------------------------------------------------------------------
def run_case(name, reduce, records=None):
    """Every assertion of the case table for `name`, on reduce(A, chunk) -> (d, e, Q)."""
    kind, _, extra = CASES[name]
    A = matrix(name)
    n = A.shape[0]
    chunk = extra if kind == "random" and extra else 0
    d, e, Q = reduce(A, chunk)
    if kind == "scaled":
        check_b(A, d, e, Q)
        check_a(name, d, e, Q)
        for s in SCALES:
            ds, es, Qs = reduce(A * s, 0)
            assert np.array_equal(ds, d * s) and np.array_equal(es, e * s), f"d, e of {s:g} A are not {s:g} times those of A"
            assert bits(Qs) == bits(Q), f"Q of {s:g} A differs from Q of A"
        return
    check_b(A, d, e, Q)
    rec = check_a(name, d, e, Q)
    if records is not None:
        records[name] = rec
    if kind == "block_diag":
        anorm = probe_and_lapack(name)[0].anorm
        lo = 0
        for hi in tuple(extra) + (n,):
            if hi < n:
                assert e[hi - 1] == 0.0, f"e[{hi - 1}] = {e[hi - 1]!r} at the split"
            from scipy.linalg import eigvalsh_tridiagonal
            wt = eigvalsh_tridiagonal(d[lo:hi], e[lo:hi - 1]) if hi - lo > 1 else d[lo:hi]
            wa = np.linalg.eigvalsh(A[lo:hi, lo:hi])
            assert np.abs(wt - wa).max() <= 40 * n * EPS * anorm
            lo = hi
    elif kind == "complex_tridiagonal":
        assert within_ulps(np.abs(e), np.abs(A.diagonal(-1)), 4)
    elif kind == "real_symmetric":
        assert not Q.imag.any(), "Q of a real symmetric matrix has imaginary parts"
    elif kind == "lower_only":
        d2, e2, Q2 = reduce(dirty_upper(A), 0)
        assert bits(d2, e2, Q2) == bits(d, e, Q), "the strict upper triangle or the imaginary diagonal was read"


# ---- a plain restatement of the unblocked reduction (zhetd2 with zlarfg, lower triangle), with planted faults --------------------------
SAFE_LO, SAFE_HI = -400, 400                  # herm.hip: the matrix is scaled when max |a| lies outside [2^-400, 2^400)
FAULTS = ("skip_tile", "upper_tile", "diag_imag", "drop_chunk", "beta_sign", "tau_conj", "unscaled")


def numpy_reduce(A, chunk=0, fault=None):
    """zhetd2('L') in NumPy as the device organises it: a power-of-two scaling of the whole matrix when its largest entry is
    far from 1, an unscaled sum of squares inside zlarfg, the matvec on the lower triangle.  `fault` plants one of FAULTS."""
    assert fault is None or fault in FAULTS
    A = np.asarray(A, dtype=np.complex128)
    n = A.shape[0]
    nbk = (n + TILE - 1) // TILE
    f = 1.0
    if fault != "unscaled":
        low = np.tril(A)
        m = max(float(np.fmax.reduce(np.abs(low.real), axis=None)), float(np.fmax.reduce(np.abs(np.tril(A, -1).imag), axis=None)))
        if 0.0 < m < np.inf:
            ex = math.frexp(m)[1] - 1
            if ex < SAFE_LO or ex >= SAFE_HI:
                f = 2.0 ** max(-1000, min(1000, -ex))
    L = np.tril(A, -1) * f
    if fault == "upper_tile":                                   # tile (1, 0) taken from its mirror image in the upper triangle
        L[TILE:2 * TILE, 0:TILE] = (A[0:TILE, TILE:2 * TILE] * f).conj().T
    dg = (A.diagonal() if fault == "diag_imag" else A.diagonal().real.astype(np.complex128)) * f
    M = L + L.conj().T + np.diag(dg)
    d, e = np.zeros(n), np.zeros(max(n - 1, 0))
    taus, vs = [], []
    for i in range(n - 1):
        d[i] = M[i, i].real
        alpha, x = M[i + 1, i], M[i + 2:, i]
        xnorm = math.sqrt(float(np.sum(x.real * x.real + x.imag * x.imag)))
        v = np.zeros(n - i - 1, dtype=np.complex128)
        v[0] = 1.0
        if xnorm == 0.0 and alpha.imag == 0.0:
            tau, beta = 0.0j, alpha.real
        else:
            nrm = math.hypot(alpha.real, alpha.imag, xnorm)                # dlapy3
            beta = math.copysign(nrm, alpha.real) if fault == "beta_sign" else -math.copysign(nrm, alpha.real)
            tau = complex((beta - alpha.real) / beta, -alpha.imag / beta)
            with np.errstate(invalid="ignore"):                                # (a NaN planted by a fault travels on)
                v[1:] = x * (1.0 / (alpha - beta))
        e[i] = beta
        taus.append(tau)
        vs.append(v)
        if tau != 0.0:
            M22 = M[i + 1:, i + 1:]
            y = np.zeros(n, dtype=np.complex128)
            y[i + 1:] = M22 @ v
            vf = np.zeros(n, dtype=np.complex128)
            vf[i + 1:] = v
            if fault == "skip_tile" and nbk >= 3:               # tile (2, 1) of the grid never enters the matvec
                R, C = slice(2 * TILE, min(3 * TILE, n)), slice(TILE, 2 * TILE)
                y[R] -= M[R, C] @ vf[C]
                y[C] -= M[R, C].conj().T @ vf[R]
            if fault == "drop_chunk":                           # hch = 8: the row sums of the second chunk of a block row are lost
                b0 = (i + 1) // TILE
                for bi in range(b0 + 8, nbk):
                    R = slice(bi * TILE, min((bi + 1) * TILE, n))
                    for bj in range(b0 + 8, bi + 1):
                        C = slice(bj * TILE, min((bj + 1) * TILE, n))
                        y[R] -= (M[R, C] if bj < bi else np.tril(M[R, C])) @ vf[C]
            wv = tau * y[i + 1:]
            wv += (-0.5 * tau * np.vdot(wv, v)) * v
            M22 -= np.outer(v, wv.conj()) + np.outer(wv, v.conj())
    if n:
        d[n - 1] = M[n - 1, n - 1].real
    Q = np.eye(n, dtype=np.complex128)
    for i in range(n - 2, -1, -1):
        tau = taus[i].conjugate() if fault == "tau_conj" else taus[i]
        if tau != 0.0:
            v = vs[i]
            Q[i + 1:, i + 1:] -= tau * np.outer(v, v.conj() @ Q[i + 1:, i + 1:])
    g = 1.0 / f
    return d * g, e * g, Q
