"""Real operators and the NumPy restatement behind real_arith="on" (maus_real_set_method, csrc/gmres.hip; DESIGN §11 "GMRES in
real arithmetic"), shared by tests/test_real_arith_host.py and tests/test_gpu_real_arith.py.  Pure NumPy / SciPy.

The operators are the real parts of the operators of tests/gmres_cases.py and tests/sell_cases.py (stored zeros stay stored:
the 0.3j super-diagonal of banded() becomes a diagonal of explicit 0.0), the right-hand sides the real parts of theirs.

restated() is SciPy's restarted GMRES as tests/gmres_cases.py::traced states it, written once over the dtype of the VECTORS:
complex128, or float64 "with the zero terms removed" -- |v|^2 is re^2 where the complex text has re^2 + im^2, and a product is
one multiplication.  Every sum runs on one fixed tree of element-wise additions (tree_sum), and the operator is applied entry
by entry of a padded row (EllOp), so that no library routine chooses an order of its own for one dtype and another for the
other.  The scalars -- Hessenberg column, rotations, the pseudo-solve -- are complex in both, as on the device: NumPy divides
a complex y by a complex h with imaginary part 0 as y.re * (1 / h.re), which one real division does not reproduce, so the
real path keeps the complex one-lane state machine and takes the real parts of its y."""
import numpy as np
import scipy.sparse as sp

import gmres_cases as gc
import sell_cases as sc
from oracle import maus_oracle as orc

EPS = np.finfo(np.float64).eps


# ---- operators -------------------------------------------------------------------------------------------------------------
def real_csr(M):
    """The real part of M, entry for entry of its CSR pattern, as complex128 with imaginary parts +0.0."""
    M = sp.csr_matrix(M)
    M.sort_indices()
    return sp.csr_matrix((M.data.real.astype(np.complex128), M.indices.copy(), M.indptr.copy()), shape=M.shape)


def real_vec(seed, n):
    return gc.crand(seed, n).real + 0j


def banded(n, s=1, weight=1.0):
    return real_csr(gc.banded(n, s, weight))


def tridiagonal(n, off=0.3):
    """From the real part T of sell_cases.tridiagonal(n): diagonal 1.5 + |diag T|, off-diagonals `off` times T's (N(0, 1)), so
    that almost every row is diagonally dominant and GMRES converges within a few cycles at any n."""
    T = real_csr(sc.tridiagonal(n))
    d = T.diagonal().real
    return real_csr(sp.diags(1.5 + np.abs(d)) + off * (T - sp.diags(d)))


def five_point(m):
    """2-D 5-point operator on an m x m grid plus 2 I (the operator of tools/gmres_rates.py with real values)."""
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    L = sp.kron(sp.identity(m), T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(m))
    return real_csr((L + 2.0 * sp.identity(m * m)).tocsr())


def rows_of_33(n=64):
    """n x n, every row 33 entries at columns i, i + 1, .. (mod n): nnz = 33 n > 32 n, the wave-per-row schedule, and a row
    gives lanes 0 .. 32 one entry each."""
    rng = np.random.default_rng(33)
    rows = np.repeat(np.arange(n), 33)
    cols = (rows + np.tile(np.arange(33), n)) % n
    return real_csr(sp.csr_matrix((rng.standard_normal(33 * n), (rows, cols)), shape=(n, n)))


def cyclic(n):
    return real_csr(sp.csr_matrix(gc.cyclic(n, 1.0)))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def tree_sum(a):
    """Sum of a 1-D array on one fixed binary tree of element-wise additions (zero-padded to a power of two)."""
    a = np.asarray(a)
    m = 1
    while m < a.shape[0]:
        m *= 2
    t = np.zeros(m, dtype=a.dtype)
    t[: a.shape[0]] = a
    while t.shape[0] > 1:
        t = t[0::2] + t[1::2]
    return t[0]


def abs2(v):
    """|v|^2 entry by entry: re^2 + im^2, or re^2 for real vectors (the zero term removed)."""
    return v.real * v.real + v.imag * v.imag if np.iscomplexobj(v) else v * v


def norm(v):
    return float(np.sqrt(tree_sum(abs2(v))))


class EllOp:
    """y = H x with H = A - shift I + psi I, row i summed entry by entry in CSR order: acc += val[i, p] * x[idx[i, p]] for
    p ascending, element-wise over the rows, then + (psi - shift) x."""

    def __init__(self, A, shift, psi, dtype):
        A = sp.csr_matrix(A)
        A.sort_indices()
        n = A.shape[0]
        lens = np.diff(A.indptr)
        w = int(lens.max()) if n else 0
        self.idx = np.zeros((n, w), dtype=np.int64)
        self.val = np.zeros((n, w), dtype=dtype)
        for i in range(n):
            p0, p1 = A.indptr[i], A.indptr[i + 1]
            self.idx[i, : p1 - p0] = A.indices[p0:p1]
            self.val[i, : p1 - p0] = A.data[p0:p1] if dtype == np.complex128 else A.data[p0:p1].real
        self.live = np.arange(w)[None, :] < lens[:, None]
        sh = np.complex128(psi) - np.complex128(shift)
        self.sh = sh if dtype == np.complex128 else np.float64(sh.real)
        self.diag = np.asarray(A.diagonal(), dtype=dtype if dtype == np.complex128 else np.complex128)
        self.dtype = dtype

    def __call__(self, x):
        acc = np.zeros(x.shape[0], dtype=self.dtype)
        for p in range(self.idx.shape[1]):
            acc = np.where(self.live[:, p], acc + self.val[:, p] * x[self.idx[:, p]], acc)
        return acc + self.sh * x


def restated(A, b, shift, psi, jacobi, dtype, rtol=1e-8, maxiter=50, restart=20):
    """GMRES from x0 = b on ((A - shift I) + psi I) x = b with vectors of `dtype` -> (x, info, inner, cycles)."""
    cplx = dtype == np.complex128
    n = b.shape[0]
    b = np.asarray(b, dtype=np.complex128)
    b = b.copy() if cplx else b.real.copy()
    H = EllOp(A, shift, psi, dtype)
    inv = None
    if jacobi:
        d = (np.asarray(sp.csr_matrix(A).diagonal(), dtype=np.complex128) - np.complex128(shift)) + np.complex128(psi)
        inv = 1.0 / d if cplx else 1.0 / d.real

    def psolve(v):
        return v.copy() if inv is None else inv * v

    def scalar(t):                                    # a vector-side scalar on the Hessenberg side: complex, imaginary part +0
        return np.complex128(t)

    def vec(t):                                       # and back: the complex scalar itself, or its real part
        return t if cplx else np.float64(np.complex128(t).real)

    x = b.copy()
    bnrm2 = norm(b)
    atol = max(0.0, rtol * bnrm2)
    if bnrm2 == 0:
        return x, 0, 0, 0
    restart = min(restart, n)
    ptol_max_factor = 1.0
    ptol = norm(psolve(b)) * min(ptol_max_factor, atol / bnrm2)
    presid = 0.0
    V = np.empty((restart + 1, n), dtype=dtype)
    Hh = np.zeros((restart, restart + 1), dtype=np.complex128)
    giv = np.zeros((restart, 2), dtype=np.complex128)
    inner = cycles = 0
    rnorm = np.inf
    for cycle in range(maxiter):
        if cycle == 0:
            r = b - H(x)
            if norm(r) < atol:
                return x, 0, inner, cycles
        cycles += 1
        V[0] = psolve(r)
        tmp = norm(V[0])
        V[0] = V[0] * (1 / tmp)
        S = np.zeros(restart + 1, dtype=np.complex128)
        S[0] = tmp
        breakdown = False
        col = 0
        for col in range(restart):
            w = psolve(H(V[col]))
            h0 = norm(w)
            for k in range(col + 1):
                t = tree_sum(np.conj(V[k]) * w)
                Hh[col, k] = scalar(t)
                w = w - t * V[k]
            h1 = norm(w)
            Hh[col, col + 1] = h1
            V[col + 1] = w
            if h1 <= EPS * h0:
                Hh[col, col + 1] = 0
                breakdown = True
            else:
                V[col + 1] = V[col + 1] * (1 / h1)
            for k in range(col):
                c, s = giv[k, 0], giv[k, 1]
                n0, n1 = Hh[col, k], Hh[col, k + 1]
                Hh[col, k], Hh[col, k + 1] = c * n0 + s * n1, -np.conj(s) * n0 + c * n1
            c, s, mag = orc.zlartg(Hh[col, col], Hh[col, col + 1])
            giv[col] = (c, s)
            Hh[col, col], Hh[col, col + 1] = mag, 0
            t = -np.conjugate(s) * S[col]
            S[col], S[col + 1] = c * S[col], t
            presid = np.abs(t)
            inner += 1
            if presid <= ptol or breakdown:
                break
        if Hh[col, col] == 0:
            S[col] = 0
        y = np.array(S[: col + 1], dtype=np.complex128)
        for k in range(col, 0, -1):
            if y[k] != 0:
                y[k] /= Hh[k, k]
                t = y[k]
                y[:k] -= t * Hh[k, :k]
        if y[0] != 0:
            y[0] /= Hh[0, 0]
        for j in range(col + 1):                      # x += y @ V[:col + 1], one column after the other
            x = x + vec(y[j]) * V[j]
        r = b - H(x)
        rnorm = norm(r)
        if rnorm <= atol:
            break
        elif breakdown:
            break
        elif presid <= ptol:
            ptol_max_factor = max(EPS, 0.25 * ptol_max_factor)
        else:
            ptol_max_factor = min(1.0, 1.5 * ptol_max_factor)
        ptol = presid * min(ptol_max_factor, atol / rnorm)
    info = 0 if rnorm <= atol else maxiter
    return x, info, inner, cycles


def flagged_real(values):
    """The library's flag (maus_real_plan reports it): every imaginary part has the bits of +0.0 or -0.0."""
    v = np.ascontiguousarray(values, dtype=np.complex128).view(np.uint64).reshape(-1, 2)[:, 1]
    return bool(np.all((v << np.uint64(1)) == 0))
