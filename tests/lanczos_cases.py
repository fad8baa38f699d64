"""Test operators of the device Lanczos (tests/test_gpu_lanczos.py, tools/lanczos_rates.py)."""
import numpy as np
import scipy.sparse as sp


def lattice(nx, ny, c=4.0, real=False, seed=3):
    """Hermitian 2-D operator on an nx x ny grid (site (i, j) -> i ny + j): links to the lower and to the right neighbour with
    value -exp(2 pi i u) (-1 for the real case) and its conjugate, diagonal c + 4 (u - 0.5); all draws from default_rng(seed)
    in that order (links down, links right, diagonal).  Random link phases and a random diagonal leave no symmetry-induced
    multiple eigenvalues."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(nx, ny)
    rows, cols, vals = [], [], []
    for a, b in ((idx[:-1, :].ravel(), idx[1:, :].ravel()), (idx[:, :-1].ravel(), idx[:, 1:].ravel())):
        u = rng.random(a.size)
        v = -np.ones(a.size) if real else -np.exp(2j * np.pi * u)
        rows += [a, b]
        cols += [b, a]
        vals += [v, v.conj()]
    d = c + 4.0 * (rng.random(n) - 0.5)
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(d)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n),
                      dtype=np.float64 if real else np.complex128)
    A.sort_indices()
    return A


def tridiagonal(n, seed=7):
    """Hermitian tridiagonal matrix: diagonal 4 + N(0, 1), off-diagonal -1 + 0.3i N(0, 1), from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    d = 4.0 + rng.standard_normal(n)
    e = -1.0 + 0.3j * rng.standard_normal(n - 1)
    return sp.csr_matrix(sp.diags([e.conj(), d.astype(np.complex128), e], [-1, 0, 1], format="csr"))


def start_vector(n):
    return np.random.default_rng(1).standard_normal(n)


# (name, nx, ny, c, real)
LATTICES = [("c64x50", 64, 50, 4.0, False), ("c256x250", 256, 250, 4.0, False), ("r256x250", 256, 250, 4.0, True),
            ("split256x250", 256, 250, 0.0, False), ("c1024x1000", 1024, 1000, 4.0, False)]
