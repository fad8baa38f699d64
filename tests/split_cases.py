"""Inputs and the NumPy model of the split band solve (sparse_split="on", maus_band_set_split; csrc/band.hip, DESIGN §11 "The
split method"), shared by tests/test_band_split_host.py on the CPU and tests/test_gpu_band_split.py on the device.

The model runs the device's elimination order with the device's pivot rule on a dense copy: the interior columns of every
partition in ascending order, pivoting among the partition's rows not yet used (first maximum of |re| + |im| in row order, a
NaN never wins, a zero pivot records the column, the zero candidate nearest the diagonal leaves and the step goes on
without an update); then the leftover rows, in row order,
partition after partition, as a system in the separator columns, factored as zgbtf2 factors it; then the back substitution."""
import numpy as np

# tridiagonal, pentadiagonal, one-sided, kl != ku, kl + ku = 31 three ways, kl = ku = 15
SHAPES = [(1, 1), (2, 2), (0, 4), (4, 0), (3, 2), (7, 24), (15, 15), (15, 16), (1, 30)]
EPS = float(np.finfo(np.float64).eps)


def band_case(n, kl, ku, seed, zero_cols=()):
    """tests/test_gpu_band.py's _band_case (the same draws) with 0.75 (kl + ku + 1) added to the diagonal: the raw random
    bands are singular to working precision where the band is one-sided.  Returns (A dense, ab in zgbtrf's layout, b)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    for d in range(-ku, kl + 1):
        m = n - abs(d)
        if m <= 0:
            continue
        v = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        A += np.diag(v, -d)
    A += 0.75 * (kl + ku + 1) * np.eye(n)
    for j in zero_cols:
        A[:, j] = 0
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, to_band(A, kl, ku), b


def to_band(A, kl, ku):
    n = A.shape[0]
    ab = np.zeros((2 * kl + ku + 1, n), dtype=np.complex128)
    for d in range(-ku, kl + 1):
        m = n - abs(d)
        if m > 0:
            j = np.arange(max(0, -d), max(0, -d) + m)
            ab[kl + ku + d, j] = A[j + d, j]
    return ab


def from_band(ab, kl, ku):
    n = ab.shape[1]
    A = np.zeros((n, n), dtype=np.complex128)
    for d in range(-ku, kl + 1):
        m = n - abs(d)
        if m > 0:
            j = np.arange(max(0, -d), max(0, -d) + m)
            A[j + d, j] = ab[kl + ku + d, j]
    return A


def toeplitz_shifted(n, kd, rel=1e-9, seed=5):
    """A non-Hermitian Toeplitz band operator (kl = ku = kd) shifted onto one of its eigenvalues to `rel` relative."""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    for d in range(-kd, kd + 1):
        A += np.diag(np.full(n - abs(d), rng.standard_normal() + 1j * rng.standard_normal()), d)
    ev = np.linalg.eigvals(A)
    lam = ev[np.argmin(np.abs(ev - ev.mean()))]
    A -= lam * (1.0 + rel) * np.eye(n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return A, to_band(A, kd, kd), b


def partitions(n, kl, ku, m):
    """[(a, b, r0, r1, s0, s1)] per partition: interior columns a .. b, rows [r0, r1), separator columns [s0, s1)."""
    w = kl + ku
    p = (n + m - 1) // m
    out = []
    for i in range(p):
        a = i * m
        last = i == p - 1
        b = n - 1 if last else a + m - w - 1
        out.append((a, b, max(a - ku, 0), n if last else a + m - ku, b + 1, b + 1 if last else a + m))
    return out


def column_order(n, kl, ku, m):
    """Q: every interior, partition after partition, then every separator."""
    parts = partitions(n, kl, ku, m)
    return np.array([c for a, b, *_ in parts for c in range(a, b + 1)] + [c for *_, s0, s1 in parts for c in range(s0, s1)],
                    dtype=np.int64)


def omega(H, x, b):
    """Normwise backward error |b - H x|_inf / (|H|_inf |x|_inf + |b|_inf)."""
    return float(np.abs(b - H @ x).max() / (np.abs(H).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))


def model_omega(H, b, kl, ku, m):
    """omega of LAPACK's solve of the column-reordered system H[:, Q] y = b, x[Q] = y: the reference for this ordering."""
    import scipy.linalg as sla
    Q = column_order(H.shape[0], kl, ku, m)
    x = np.empty(H.shape[0], dtype=np.complex128)
    x[Q] = sla.solve(H[:, Q], b)
    return omega(H, x, b)


def _first_max(v, gap_rel):
    """(index of the first maximum with NaN never winning, whether the runner-up is within gap_rel of it)."""
    vv = np.where(np.isnan(v), -1.0, v)
    k = int(np.argmax(vv))
    rest = np.delete(vv, k)
    close = rest.size > 0 and vv[k] > 0 and rest.max() >= vv[k] * (1.0 - gap_rel)
    return k, bool(close)


def split_reference(ab, b, kl, ku, m, gap_rel=1e-6):
    """(x, status, piv, sure): the model's solution; status 0 or 1 + the smallest column with a zero pivot; piv[c] the 0-based
    pivot row of column c -- a row of H for an interior column, a row of the reduced system (zgbtrf's ipiv of it) for a
    separator column -- and sure[c] False where the best and the second candidate were within gap_rel of each other."""
    n = ab.shape[1]
    w = kl + ku
    assert m >= 2 * w + 2 and n > m and w >= 1
    M = np.concatenate([from_band(ab, kl, ku), np.asarray(b, dtype=np.complex128)[:, None]], axis=1)
    parts = partitions(n, kl, ku, m)
    used = np.zeros(n, dtype=bool)
    piv = np.full(n, -1, dtype=np.int64)
    sure = np.ones(n, dtype=bool)
    info = 0
    a1 = lambda z: np.abs(z.real) + np.abs(z.imag)
    left = []
    for a, bb, r0, r1, s0, s1 in parts:
        for c in range(a, bb + 1):
            rows = np.array([r for r in range(r0, min(c + kl, r1 - 1) + 1) if not used[r]])
            v = a1(M[rows, c])
            k, close = _first_max(v, gap_rel)
            if not v[k] > 0:                                             # no pivot: the zero candidate nearest the diagonal leaves
                ok = np.flatnonzero(v == 0) if (v == 0).any() else np.arange(rows.size)
                k = int(ok[np.argmin(np.abs(rows[ok] - c))])
            pr = rows[k]
            piv[c], sure[c] = pr, not close
            used[pr] = True
            if M[pr, c] == 0:
                info = info or c + 1
                M[np.delete(rows, k), c] = 0
                continue
            others = np.delete(rows, k)
            lo, hi = max(a - w, 0), min(c + w, n - 1) + 1
            l = M[others, c] / M[pr, c]
            M[others, lo:hi] -= l[:, None] * M[pr, lo:hi][None, :]
            M[others, n] -= l * M[pr, n]
            M[others, c] = 0
        left += [r for r in range(r0, r1) if not used[r]]
    sep = np.array([c for *_, s0, s1 in parts for c in range(s0, s1)], dtype=np.int64)
    nr = sep.size
    assert len(left) == nr
    R = M[np.ix_(left, np.append(sep, n))]
    klr = min(kl + w - 1, nr - 1)
    for q in range(nr):                                                  # zgbtf2 on the reduced system, the rhs with it
        hi = min(q + klr, nr - 1) + 1
        k, close = _first_max(a1(R[q:hi, q]), gap_rel)
        piv[sep[q]], sure[sep[q]] = q + k, not close
        if R[q + k, q] == 0:
            cq = int(sep[q]) + 1
            info = min(info, cq) if info else cq
            continue
        if k:
            R[[q, q + k]] = R[[q + k, q]]
        l = R[q + 1:hi, q] / R[q, q]
        R[q + 1:hi, q + 1:] -= l[:, None] * R[q, q + 1:][None, :]
        R[q + 1:hi, q] = 0
    x = np.zeros(n, dtype=np.complex128)
    with np.errstate(all="ignore"):
        for q in range(nr - 1, -1, -1):
            x[sep[q]] = (R[q, nr] - R[q, q + 1:nr] @ x[sep[q + 1:]]) / R[q, q]
        for a, bb, r0, r1, s0, s1 in parts:
            for c in range(bb, a - 1, -1):
                pr = piv[c]
                lo, hi = max(a - w, 0), min(c + w, n - 1) + 1
                row = M[pr, lo:hi].copy()
                row[c - lo] = 0
                x[c] = (M[pr, n] - row @ x[lo:hi]) / M[pr, c]
    return x, info, piv, sure
