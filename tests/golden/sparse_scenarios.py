"""Seeded sparse inputs shared by the sparse golden generator (make_sparse_goldens.py, which drives the *reference*) and by
the tests (tests/test_sparse_host.py, tests/test_gpu_sparse.py).  Pure NumPy / SciPy; like scenarios.py, every matrix
comes from np.random.default_rng(seed), never from the legacy global streams the harness seeds afterwards."""
import numpy as np
import scipy.sparse as sp


def banded_complex(n, seed, far=3):
    """complex tridiagonal (diagonal 4 + N(0,1) + i N(0,1), off-diagonals -1 + 0.3i N(0,1)) plus `far` entries far from
    the band, as a dense ndarray (about 3/n dense: the reference converts it to CSC, AMS:357-358)"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    A[i, i] = 4.0 + rng.standard_normal(n) + 1j * rng.standard_normal(n)
    A[i[:-1], i[:-1] + 1] = -1.0 + 0.3j * rng.standard_normal(n - 1)
    A[i[1:], i[1:] - 1] = -1.0 + 0.3j * rng.standard_normal(n - 1)
    for _ in range(far):
        r, c = rng.integers(0, n, 2)
        A[r, c] += 0.5 + 0.5j
    return A


def hermitian_sparse(n, seed, real=False, per_row=3):
    """Hermitian (real symmetric for real=True) CSR matrix with about per_row random off-diagonal entries per row"""
    rng = np.random.default_rng(seed)
    m = n * per_row // 2
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    v = rng.standard_normal(m) + (0.0 if real else 1j) * rng.standard_normal(m)
    B = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    A = (B + B.conj().T) * 0.5 + sp.diags(rng.standard_normal(n) * 2.0)
    A = sp.csr_matrix(A, dtype=np.float64 if real else np.complex128)
    A.sum_duplicates()
    A.sort_indices()
    return A


def sparse_rect(m, n, seed, density=0.15):
    rng = np.random.default_rng(seed)
    k = int(m * n * density)
    r, c = rng.integers(0, m, k), rng.integers(0, n, k)
    v = rng.standard_normal(k) + 1j * rng.standard_normal(k)
    A = sp.coo_matrix((v, (r, c)), shape=(m, n)).tocsr() + sp.eye(m, n, dtype=np.complex128)
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


# name -> spec; "modes": the gmres_compat modes a fixture is captured for ('rtol' runs the reference through the tol->rtol
# shim of make_goldens.py, 'scipy-legacy' unshimmed: TypeError swallowed -> spsolve); "arpack": the reference's eigsh runs,
# which the product replaces by one eigh per matrix, so the fixture keeps the first body's rows for a tolerance check)
SPARSE_TRAJECTORIES = {
    "sp_lin48": dict(kind="lin", n=48, seed=101, P=24, tol=1e-8, iters=6, modes=("rtol", "scipy-legacy")),
    "sp_eig40": dict(kind="eig", n=40, seed=102, P=32, tol=1e-8, iters=4, modes=("rtol", "scipy-legacy")),
    "sp_herm40": dict(kind="eig", n=40, seed=103, P=16, tol=1e-8, iters=3, modes=("rtol",), arpack=True),
    "sp_herm6": dict(kind="eig", n=6, seed=104, P=8, tol=1e-8, iters=5, modes=("rtol", "scipy-legacy")),
    "sp_real_herm24": dict(kind="eig", n=24, seed=105, P=12, tol=1e-8, iters=3, modes=("rtol",), arpack=True),
    "sp_svd40x32": dict(kind="svd", n=40, m=32, seed=106, P=12, tol=1e-6, iters=4, modes=("rtol",)),
    "demo1": dict(kind="lin", n=5, seed=107, P=15, tol=1e-7, iters=10, modes=("rtol", "scipy-legacy")),
}


def build(name):
    """(A, b) of a sparse scenario: A as the reference receives it (ndarray, csc_matrix or csr_matrix)"""
    spec = SPARSE_TRAJECTORIES[name]
    n = spec["n"]
    b = None
    if name == "sp_lin48":
        A = banded_complex(n, spec["seed"])
        rng = np.random.default_rng(spec["seed"] + 1000)
        b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    elif name == "sp_eig40":
        A = sp.csc_matrix(banded_complex(n, spec["seed"]))
    elif name in ("sp_herm40", "sp_herm6"):
        A = hermitian_sparse(n, spec["seed"])
    elif name == "sp_real_herm24":
        A = hermitian_sparse(n, spec["seed"], real=True)
    elif name == "sp_svd40x32":
        A = sparse_rect(n, spec["m"], spec["seed"])
    elif name == "demo1":
        A, b = np.eye(5), np.ones(5)                      # AMS:644
    else:
        raise KeyError(name)
    return A, b
