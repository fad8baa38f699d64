"""Ordering and band shape of a sparse problem matrix for the band solves of csrc/band.hip.

`band_order(A)` picks, once per matrix, the symmetric permutation the band LU works in: reverse Cuthill-McKee on the pattern
of |A| + |A|^T + I, or the identity when that is no wider.  Width is the band storage a solve needs, 2 kl + ku + 1 rows
(zgbtrf's ldab).  The result depends on the matrix alone."""
from __future__ import annotations

import numpy as np


def band_widths(A, perm) -> tuple[int, int]:
    """(kl, ku): the lower and upper half-bandwidths of A[perm][:, perm] over its stored pattern."""
    import scipy.sparse as sp
    C = sp.coo_matrix(A)
    n = C.shape[0]
    iperm = np.empty(n, dtype=np.int64)
    iperm[np.asarray(perm, dtype=np.int64)] = np.arange(n, dtype=np.int64)
    if C.nnz == 0:
        return 0, 0
    d = iperm[C.row] - iperm[C.col]
    return max(int(d.max()), 0), max(int(-d.min()), 0)


def band_order(A) -> tuple[np.ndarray, int, int]:
    """(perm, kl, ku) for a square scipy.sparse matrix A: perm[i] = the row of A that becomes row i."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    M = sp.csr_matrix(A)
    n = M.shape[0]
    if M.shape[0] != M.shape[1]:
        raise ValueError("band_order: square matrix required")
    C = M.tocoo()
    P = sp.csr_matrix((np.ones(C.nnz), (C.row, C.col)), shape=M.shape)
    P = (P + P.T + sp.identity(n, format="csr")).tocsr()         # the pattern of |A| + |A|^T + I (no cancellation)
    P.sort_indices()
    rcm = np.asarray(reverse_cuthill_mckee(P, symmetric_mode=True), dtype=np.int64)
    ident = np.arange(n, dtype=np.int64)
    kl_i, ku_i = band_widths(M, ident)
    kl_r, ku_r = band_widths(M, rcm)
    if 2 * kl_i + ku_i + 1 <= 2 * kl_r + ku_r + 1:
        return ident, kl_i, ku_i
    return rcm, kl_r, ku_r


# The rule of csrc/band.hip's band_plan, restated for sizing before a context exists; tests/test_band_plan_host.py compares the
# two over every boundary (maus_band_plan needs no device).
# sparse_direct -> maus_band_set_method, in the order the keyword lists its modes
DIRECT_METHOD = {"band": 0, "blocked": 1, "tiled": 2, "narrow": 8, "wide": 4}

BLOCKED_NB = 16                 # block width of the blocked method (8 where kl + 16 > 1024)
BLOCKED_MIN_KL = 16             # narrower bands run the column kernel under sparse_direct='blocked' too ...
BLOCKED_MAX_KL = 1024           # ... and so do bands too tall for its one-workgroup panel


def runs_blocked(kl: int, ku: int) -> bool:
    """Whether the blocked method takes a (kl, ku) band when it is selected (pinned by tests/test_band_plan_host.py)."""
    return BLOCKED_MIN_KL <= kl <= BLOCKED_MAX_KL


TILED_MIN_KL = 16               # the tiled method's range under sparse_direct='tiled': the column kernel outside it ...
TILED_MAX_KL = 4096             # ... which is where its register panel ends (above kl = 1024: nb = 16 to 1520, 8 to 3064, then 4)


def runs_tiled(kl: int, ku: int) -> bool:
    """Whether the tiled method takes a (kl, ku) band when it is selected (pinned by tests/test_band_plan_host.py)."""
    return TILED_MIN_KL <= kl <= TILED_MAX_KL


WIDE_MIN_KL = 64                # the wide method's range under sparse_direct='wide': below it the outer block is wider than
WIDE_MAX_KL = 4096              # the band's reach (the tiled method runs from kl = 16), above it the inner panel ends
WIDE_NBO = 64                   # columns of the outer block


def runs_wide(kl: int, ku: int) -> bool:
    """Whether the wide method takes a (kl, ku) band when it is selected (pinned by tests/test_band_plan_host.py)."""
    return WIDE_MIN_KL <= kl <= WIDE_MAX_KL


NARROW_MAX_KL = 15              # the narrow method's range under sparse_direct='narrow': the bands whose live columns
NARROW_MAX_KV = 31              # (kl + ku + 1 of them) fit its LDS ring; the column kernel outside it


def runs_narrow(kl: int, ku: int) -> bool:
    """Whether the narrow method takes a (kl, ku) band when it is selected (pinned by tests/test_band_plan_host.py)."""
    return 0 <= kl <= NARROW_MAX_KL and kl + ku <= NARROW_MAX_KV


def kernel_for(method: int, kl: int, ku: int) -> tuple[int, int]:
    """(kind, nb) that a (kl, ku) band runs under `method`, as maus_band_kernel_for: kind one of DIRECT_METHOD's values (0
    where the method does not take the band; under 4 the tiled kernels for 16 <= kl < 64), nb the (inner) block width."""
    nb = BLOCKED_NB if kl + BLOCKED_NB <= 1024 else 8                   # while two rows per thread of the panel hold kl + nb
    if method == 1 and runs_blocked(kl, ku):
        return 1, nb
    if method in (2, 4) and runs_tiled(kl, ku):
        if kl > BLOCKED_MAX_KL:                                          # the widest block whose panel stays in registers
            nb = 16 if kl + 16 <= 1536 else (8 if kl + 8 <= 3072 else 4)
        return (4 if method == 4 and runs_wide(kl, ku) else 2), nb
    if method == 8 and runs_narrow(kl, ku):
        return 8, 1
    return 0, 1


def band_bytes_per_solve(n: int, kl: int, ku: int, blocked: bool = False, tiled: bool = False, wide: bool = False,
                         narrow: bool = False, method: int | None = None) -> int:
    """Device memory of one band solve: the band storage, the right-hand side and the pivots; with `blocked` (`tiled`), and
    a band the blocked (tiled) method takes, its panel of L and its reach as well; with `wide` the tiled method's where that
    runs, and the L of the outer block ((kl + 64) x 64) where the wide method does.  `narrow` adds nothing: the narrow method
    works in the column kernel's workspace.  `method` (a value of DIRECT_METHOD) stands for the flag of that method."""
    if method is not None:
        blocked, tiled, wide = method == 1, method == 2, method == 4
    per = 16 * ((2 * kl + ku + 1) * n + n) + 4 * n
    if (blocked and runs_blocked(kl, ku)) or ((tiled or wide) and runs_tiled(kl, ku)):
        per += 16 * (kl + BLOCKED_NB) * BLOCKED_NB + 4
    if wide and runs_wide(kl, ku):
        per += 16 * (kl + WIDE_NBO) * WIDE_NBO
    return per


# The split beside the method (sparse_split='on', maus_band_set_split; DESIGN §11 "The split method"), restated from
# csrc/band.hip's split_plan; tests/test_band_split_host.py compares the two over every boundary.
SPLIT_MAX_KL = NARROW_MAX_KL    # the narrow range without the diagonal case ...
SPLIT_MAX_W = NARROW_MAX_KV     # ... and n above one partition length


def split_len(n: int, kl: int, ku: int) -> int:
    """The rule's partition length: 64 ceil(sqrt(n w) / 64) with w = kl + ku, at least 2 w + 2."""
    import math
    w = kl + ku
    s = math.isqrt(n * w)
    if s * s < n * w:
        s += 1
    return max((s + 63) // 64 * 64, 2 * w + 2)


def _split_m(n: int, kl: int, ku: int, part_len: int) -> int:
    if part_len and part_len < 2 * (kl + ku) + 2:
        raise ValueError(f"the partition length must be at least 2 (kl + ku) + 2 = {2 * (kl + ku) + 2}, not {part_len}")
    return part_len or split_len(n, kl, ku)


def runs_split(n: int, kl: int, ku: int, part_len: int = 0) -> bool:
    """Whether the split takes an (n, kl, ku) band when it is on: 1 <= kl + ku <= 31, kl <= 15 and at least two partitions."""
    w = kl + ku
    if w < 1 or kl > SPLIT_MAX_KL or w > SPLIT_MAX_W or n < 1:
        return False
    return n > _split_m(n, kl, ku, part_len)


def split_shape(n: int, kl: int, ku: int, part_len: int = 0) -> tuple[int, int, int, int]:
    """(p, n_red, kl_red, ku_red) of a band the split takes: partitions, and the order and half-bandwidths of the reduced
    system in the separator unknowns."""
    w = kl + ku
    m = _split_m(n, kl, ku, part_len)
    p = (n + m - 1) // m
    n_red = (p - 1) * w
    return p, n_red, min(kl + w - 1, n_red - 1), min(ku + w - 1, n_red - 1)


def split_bytes_per_solve(n: int, kl: int, ku: int, part_len: int = 0, method: int = 0) -> int:
    """Device memory the split adds to band_bytes_per_solve for a band it takes (0 for any other): the pivot rows
    n (2 w + 2), the reduced system's own workspace under `method`, its solution, and three status words."""
    if not runs_split(n, kl, ku, part_len):
        return 0
    w = kl + ku
    _, n_red, klr, kur = split_shape(n, kl, ku, part_len)
    return 16 * n * (2 * w + 2) + band_bytes_per_solve(n_red, klr, kur, method=method) + 16 * n_red + 12
