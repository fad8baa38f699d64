"""Matrices and the NumPy restatement of the sliced-ELL layout shared by tests/test_spmm_plan_host.py and
tests/test_gpu_spmm_sell.py (csrc/spmm.hip, DESIGN §10 "SpMM on a sliced-ELL copy").  Pure NumPy / SciPy."""
import numpy as np
import scipy.sparse as sp

SLICE = 64                    # rows per slice: one wave
FILL_CAP = 200                # the documented default of maus_spmm_set_method's fill_cap_percent (what 0 means)
FORCE = 1000000               # the largest cap: sliced ELL for every lane-per-row operand that stores anything


def csr(A):
    A = sp.csr_matrix(A, dtype=np.complex128)
    A.sum_duplicates()
    A.sort_indices()
    return A


def adjoint(A):
    return csr(A.conj().T)


def random_pattern(n, per_row, seed=1):
    """tests/test_gpu_sparse.py::_random_pattern: per_row random columns per row (duplicates summed) plus 30 I"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, n * per_row)
    vals = rng.standard_normal(n * per_row) + 1j * rng.standard_normal(n * per_row)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    return csr(A + sp.identity(n, format="csr") * 30.0)


def tridiagonal(n, seed=2):
    """complex tridiagonal (1 x 1: a single entry)"""
    rng = np.random.default_rng(seed)
    d = [rng.standard_normal(n - abs(o)) + 1j * rng.standard_normal(n - abs(o)) for o in (-1, 0, 1)]
    if n == 1:
        return csr(sp.csr_matrix(np.array([[d[1][0] + 3.0]])))
    return csr(sp.diags(d, [-1, 0, 1], shape=(n, n)) + sp.identity(n) * 3.0)


def empty_slice_200():
    """200 x 200, 5 random entries per row plus the diagonal, rows 64..127 emptied: a whole empty slice, zero-length lanes"""
    A = random_pattern(200, 5).tolil()
    for r in range(64, 128):
        A.rows[r], A.data[r] = [], []
    return csr(A)


def ragged_256():
    """256 x 256 identity plus two rows of 64 entries spread over the full width: the second slice is as wide as those two
    rows and every other lane of it holds one entry and padding"""
    rng = np.random.default_rng(5)
    A = sp.identity(256, format="lil", dtype=np.complex128)
    for r in (70, 125):
        cols = np.sort(rng.choice(256, 64, replace=False))
        A[r, cols] = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    return csr(A)


def rect(m, n, seed):
    """m x n at 8 % density"""
    A = sp.random(m, n, density=0.08, random_state=np.random.RandomState(seed), format="csr", dtype=np.float64)
    return csr(A * (1.0 + 0.5j) + 1j * sp.random(m, n, density=0.01, random_state=np.random.RandomState(seed + 1), format="csr"))


def sell_layout(A):
    """(off[slices + 1], len[rows], padded) of the CSR matrix A: slice s holds rows 64 s .. 64 s + 63 and is as wide as its
    longest row; rows past the end are empty."""
    A = csr(A)
    ln = np.diff(A.indptr).astype(np.int64)
    ns = -(-A.shape[0] // SLICE)
    full = np.zeros(ns * SLICE, dtype=np.int64)
    full[: A.shape[0]] = ln
    width = full.reshape(ns, SLICE).max(axis=1)
    off = np.concatenate([[0], np.cumsum(SLICE * width)])
    return off, ln, int(off[-1])


def sell_arrays(A):
    """(val, idx) of the layout: entry p of row r at off[r // 64] + 64 p + (r % 64), padding (0, 0)"""
    A = csr(A)
    off, ln, padded = sell_layout(A)
    val, idx = np.zeros(padded, dtype=np.complex128), np.zeros(padded, dtype=np.int32)
    for r in range(A.shape[0]):
        p = np.arange(ln[r])
        pos = off[r // SLICE] + SLICE * p + (r % SLICE)
        val[pos] = A.data[A.indptr[r]: A.indptr[r + 1]]
        idx[pos] = A.indices[A.indptr[r]: A.indptr[r + 1]]
    return val, idx


def fill(A):
    return sell_layout(A)[2] / max(1, csr(A).nnz)


def wide_10x1000():
    """10 x 1000 with about 500 entries: nnz > 32 rows, so the MATRIX has the wave-per-row schedule and A^H (1000 rows, about
    one entry in every second) runs under it too -- no operand takes the copy, whatever the cap"""
    return rect_entries(10, 1000, 500, 7)


def tall_1000x10():
    """1000 x 10 with about 500 entries: a lane-per-row matrix whose A^H has 10 rows of about 50 entries"""
    return rect_entries(1000, 10, 500, 8)


def rect_entries(m, n, k, seed):
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, m, k), rng.integers(0, n, k)
    return csr(sp.coo_matrix((rng.standard_normal(k) + 1j * rng.standard_normal(k), (r, c)), shape=(m, n)))


def expected_kind(M, method, cap, matrix_rows=None):
    """The documented rule, restated, for the operand M (A or A^H) of a matrix with `matrix_rows` rows (default: M is A).  The
    schedule belongs to the matrix: 2 where nnz > 32 rows of A, for both operands; else 3 under method 1 when nnz > 0 and
    100 padded <= cap nnz; else 1."""
    M = csr(M)
    if M.nnz > 32 * (M.shape[0] if matrix_rows is None else matrix_rows):
        return 2
    padded = sell_layout(M)[2]
    return 3 if method == 1 and M.nnz > 0 and 100 * padded <= (cap or FILL_CAP) * M.nnz else 1
