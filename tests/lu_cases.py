"""Planted-factor systems for the dense LU (csrc/lu.hip), the bound that makes them exact, the case table of
tests/test_lu_cases_host.py (CPU) and tests/test_gpu_lu_exact.py (device), and a restatement of the host-side dispatch.

planted() builds P A = L U from factors whose arithmetic is exact in fp64 in any summation order: the strictly lower entries
of L are 0, +-1/2, +-i/2, U is a Gaussian-integer matrix with parts in -2..2 and a diagonal of (unit) * 2^k, k = 3..5, x is a
Gaussian-integer vector and b = A x.  Every multiplier a / u is then an exact division (crecip of unit * 2^k is exact), every
Schur complement, every inverted 16 x 16 unit-lower block, every product with it and every back-substitution partial sum is
a dyadic number that budget_bits() bounds; tests/test_lu_cases_host.py demands <= 45 bits for every case, which leaves 8 for
the operand sums of the 3M complex product and for any accumulation order.  LAPACK and the device must then both return the
planted ipiv and x bit for bit, whatever the condition number.

The pivot of a column is unique under LAPACK's rule (max |re| + |im|, first index wins) by construction:
    ordinary columns   every multiplier has |re| + |im| = 1/2
    tie columns        a few rows carry multipliers with |re| + |im| = 1 (+-1, +-i, (+-1 +- i)/2): as large as the pivot, and
                       the planted pivot is the identity swap, i.e. the FIRST of the tied rows
    rule columns       u_jj = (1 + i) * 8 and the multiplier 0.75 - 0.75i in three rows: candidates of value 12 and modulus 12
                       against a pivot of value 16 and modulus 11.3 -- a modulus rule takes the candidate
    zero columns       u_jj = 0 and nothing below it: the Schur column is exactly zero, info = j + 1, identity swap
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sp

UNITS = np.array([1, -1, 1j, -1j], dtype=np.complex128)
HALVES = np.array([0, 0.5, -0.5, 0.5j, -0.5j], dtype=np.complex128)
TIES = np.array([1, -1, 1j, -1j, 0.5 + 0.5j, 0.5 - 0.5j, -0.5 + 0.5j, -0.5 - 0.5j], dtype=np.complex128)
RULE_MULT = 0.75 - 0.75j
RULE_DIAG = (1 + 1j) * 8
BLK = 16                      # MAUS_NBP: base panel width = side of the inverted diagonal blocks
SPARSE_ROW_NNZ = 32           # off-block nonzeros per row of a sparse L (at most)


def cabs1(z):
    return np.abs(np.real(z)) + np.abs(np.imag(z))


def pivot_sequence(n, kind, rng, fixed=()):
    """LAPACK-style 0-based ipiv: row j is interchanged with row ipiv[j] >= j.  Columns in `fixed` get the identity swap."""
    j = np.arange(n)
    if kind == "identity":
        piv = j.copy()
    elif kind == "last":
        piv = np.full(n, n - 1)
    elif kind == "reverse":
        piv = np.where(j < n // 2, n - 1 - j, j)
    elif kind == "random":
        piv = j + (rng.random(n) * (n - j)).astype(np.int64)
    else:
        raise ValueError(kind)
    piv = np.minimum(piv, n - 1)
    for c in fixed:
        piv[c] = c
    return piv.astype(np.int32)


def final_order(ipiv):
    """p with (P A)[i] = A[p[i]] for the interchange sequence ipiv."""
    p = np.arange(len(ipiv))
    for j, q in enumerate(ipiv):
        if q != j:
            p[j], p[q] = p[q], p[j]
    return p


def tie_rows(j, n, rng):
    """Rows below j that tie with the pivot row of column j.  With r = row - (j - j % 16) the panel-local row, the panel
    kernels give row r to thread r % NT, slot r / NT (NT = 128, 256, 512), or to workgroup r / 512 (r / 1024), so a distance
    of 128, 256, 512 or 1024 is the same lane in another slot (or another workgroup), less than 64 - j % 16 another lane of
    the wave, a multiple of 64 plus a little another wave, and beyond 1024 another workgroup of the multi-workgroup panel."""
    a = j % BLK
    want = [j + d for d in (128, 256, 512, 1024, 2048) if j + d < n][-2:]             # same lane, other slot / workgroup
    if j + 1 < n:
        want.append(j + 1 + int(rng.integers(0, max(1, min(63 - a, n - j - 1)))))     # same wave, other lane
    if j + 70 < n:
        want.append(j + 64 * int(rng.integers(1, (n - j - 6) // 64 + 1)) + int(rng.integers(0, 6)))   # another wave
    if j + 1100 < n:
        want.append(int(rng.integers(j + 1030, n)))                                  # another workgroup
    return sorted(set(r for r in want if j < r < n))


def _rows_times(Ls, U, threads=8):
    """Ls @ U for a CSR Ls, row slices on a few threads (the sparse product runs outside the interpreter lock)."""
    n = Ls.shape[0]
    out = np.empty((n, U.shape[1]), dtype=np.complex128)
    edges = np.linspace(0, n, 4 * threads + 1).astype(np.int64)

    def work(k):
        out[edges[k]:edges[k + 1]] = Ls[edges[k]:edges[k + 1]] @ U

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(4 * threads)))
    return out


def planted(n, seed, *, pivots="random", tie_cols=(), rule_cols=(), zero_cols=(), sparse_L=False):
    """A, b, x, ipiv, L, U with P A = L U exactly (see the module docstring).  L is unit lower triangular, a dense array or,
    with sparse_L, a CSR matrix with at most SPARSE_ROW_NNZ nonzeros per row outside its dense 16-column diagonal blocks."""
    rng = np.random.default_rng(seed)
    tie_cols, rule_cols, zero_cols = (sorted(set(int(c) for c in cs)) for cs in (tie_cols, rule_cols, zero_cols))
    assert not (set(tie_cols) & set(rule_cols)) and not (set(tie_cols) & set(zero_cols)) and not (set(rule_cols) & set(zero_cols))
    ipiv = pivot_sequence(n, pivots, rng, fixed=tie_cols + zero_cols)

    U = np.empty((n, n), dtype=np.complex128)
    U.real = rng.integers(-2, 3, (n, n), dtype=np.int8)
    U.imag = rng.integers(-2, 3, (n, n), dtype=np.int8)
    for i0 in range(0, n, 256):                                   # strictly lower part <- 0, block row by block row
        i1 = min(n, i0 + 256)
        U[i0:i1, :i0] = 0
        U[i0:i1, i0:i1] = np.triu(U[i0:i1, i0:i1])
    diag = UNITS[rng.integers(0, 4, n)] * 2.0 ** rng.integers(3, 6, n)
    diag[rule_cols] = RULE_DIAG
    diag[zero_cols] = 0
    U[np.arange(n), np.arange(n)] = diag

    special = {}                                                  # (row, col) -> multiplier
    for j in tie_cols:
        for r in tie_rows(j, n, rng):
            special[(r, j)] = TIES[rng.integers(0, len(TIES))]
    for j in rule_cols:
        if j + 1 < n:
            for r in rng.choice(np.arange(j + 1, n), size=min(3, n - j - 1), replace=False):
                special[(int(r), j)] = RULE_MULT
    srow = np.array([k[0] for k in special], dtype=np.int64)
    scol = np.array([k[1] for k in special], dtype=np.int64)
    sval = np.array(list(special.values()), dtype=np.complex128)

    if not sparse_L:
        L = HALVES[rng.integers(0, len(HALVES), (n, n))]
        L = np.tril(L, -1)
        L[:, zero_cols] = 0
        L[srow, scol] = sval
        L[np.arange(n), np.arange(n)] = 1
        LU = L @ U
    else:
        i = np.arange(n)
        b0 = i - i % BLK                                          # first column of row i's diagonal block
        # dense diagonal blocks
        rr = np.repeat(i, BLK)
        cc = np.repeat(b0, BLK) + np.tile(np.arange(BLK), n)
        keep = cc < rr
        rr, cc = rr[keep], cc[keep]
        # off-block entries: SPARSE_ROW_NNZ draws per row in [0, b0), duplicates dropped
        r2 = np.repeat(i[BLK:], SPARSE_ROW_NNZ)
        c2 = (rng.random(r2.shape[0]) * np.repeat(b0[BLK:], SPARSE_ROW_NNZ)).astype(np.int64)
        key = np.unique(r2 * n + c2)
        rr = np.concatenate([rr, key // n])
        cc = np.concatenate([cc, key % n])
        vv = HALVES[rng.integers(1, len(HALVES), rr.shape[0])]    # every stored entry is +-1/2 or +-i/2
        drop = np.isin(cc, zero_cols) | np.isin(rr * n + cc, srow * n + scol)
        rr, cc, vv = rr[~drop], cc[~drop], vv[~drop]
        rr = np.concatenate([rr, srow, i])
        cc = np.concatenate([cc, scol, i])
        vv = np.concatenate([vv, sval, np.ones(n, dtype=np.complex128)])
        L = sp.csr_matrix((vv, (rr, cc)), shape=(n, n))
        L.sort_indices()
        LU = None

    p = final_order(ipiv)                                         # (P A)[i] = A[p[i]]  =>  A[p] = L U
    if LU is None:
        inv = np.empty(n, dtype=np.int64)
        inv[p] = np.arange(n)
        A = _rows_times(L[inv], U)                                # rows of L go to their original places before the product
    else:
        A = np.empty_like(LU)
        A[p] = LU
    x = (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)
    b = A @ x
    return A, b, x, ipiv, L, U


def gaussian(n, seed, count=1):
    """The Gaussian complement: complex Gaussian systems of the same shapes (rounding is visible here, pivots are generic)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((count, n, n)) + 1j * rng.standard_normal((count, n, n))
    b = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    return A, b


def backward_errors(A, xs, b, threads=8):
    """Normwise backward errors ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) of several x for one system, in
    np.longdouble throughout (row blocks of A on a few threads: the long-double products run outside the interpreter lock)."""
    ld = np.longdouble
    n = A.shape[0]
    X = np.stack(xs, axis=1)
    Xr, Xi = X.real.astype(ld), X.imag.astype(ld)
    br, bi = b.real.astype(ld), b.imag.astype(ld)
    edges = np.linspace(0, n, max(1, min(4 * threads, n // 64)) + 1).astype(np.int64)
    res = np.zeros((len(edges) - 1, X.shape[1]), dtype=ld)
    nrm = np.zeros(len(edges) - 1, dtype=ld)

    def work(k):
        lo, hi = edges[k], edges[k + 1]
        Ar, Ai = A[lo:hi].real.astype(ld), A[lo:hi].imag.astype(ld)
        rr = br[lo:hi, None] - (Ar @ Xr - Ai @ Xi)
        ri = bi[lo:hi, None] - (Ar @ Xi + Ai @ Xr)
        res[k] = np.max(np.hypot(rr, ri), axis=0)
        nrm[k] = np.max(np.sum(np.hypot(Ar, Ai), axis=1))

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(len(edges) - 1)))
    nA, nb = nrm.max(), np.max(np.hypot(br, bi))
    nx = np.max(np.hypot(Xr, Xi), axis=0)
    return [float(v) for v in res.max(axis=0) / (nA * nx + nb)]


def backward_error(A, x, b):
    return backward_errors(A, [x], b)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the exactness bound
# ---------------------------------------------------------------------------------------------------------------------------
def _frac_bits(a):
    """Smallest f with a * 2^f integer in both parts (a: dyadic numbers)."""
    parts = np.concatenate([np.real(a).ravel(), np.imag(a).ravel()])
    for f in range(0, 80):
        s = parts * 2.0 ** f
        if np.array_equal(s, np.rint(s)):
            return f
    raise AssertionError("not dyadic")


def diag_block_inverses(L):
    """Inverses of the unit lower 16 x 16 diagonal blocks of L, by forward substitution (exact: asserted by the caller through
    budget_bits).  Shape (blocks, 16, 16); a last block short of 16 rows is padded with the identity."""
    n = L.shape[0]
    nb = (n + BLK - 1) // BLK
    D = np.zeros((nb, BLK, BLK), dtype=np.complex128)
    D[:, np.arange(BLK), np.arange(BLK)] = 1
    for k in range(nb):
        lo, hi = k * BLK, min(n, (k + 1) * BLK)
        blk = L[lo:hi, lo:hi]
        D[k, :hi - lo, :hi - lo] = blk.toarray() if sp.issparse(blk) else blk
    X = np.zeros_like(D)
    X[:, np.arange(BLK), np.arange(BLK)] = 1
    for i in range(1, BLK):                                       # row i of the inverse: x_i = e_i - sum_{k<i} L[i][k] x_k
        X[:, i, :i] = -np.einsum("bk,bkc->bc", D[:, i, :i], X[:, :i, :i])
    return X


def budget_bits(L, U, x=None):
    """Upper bound on the significand bits any intermediate of the factorisation and the two substitutions needs, in any
    summation order: log2 of a bound on its magnitude (|re| + |im|, which also bounds an operand sum re + im of the 3M
    product) plus the number of fraction bits of its unit.
        Schur partial sums     a_ij - sum_k l_ik u_kj over any subset of k: at most T = max_i sum_k |l_ik| |u_kj| <=
                               4 * (row sum of |L| off the diagonal) + 32 (|u| <= 4 off the diagonal, <= 32 on it); unit that of L
        forward substitution   the same sums against y = U x (the augmented column): T_y = max row sum of |L| * max |y|
        inverted blocks        Dinv by exact forward substitution; partial sums of sum_k l_ik x_k, unit that of Dinv
        Dinv * T               max row sum of |Dinv| * max(T, T_y), unit = unit(Dinv) * unit(L)
        back substitution      sum_j |u_ij| |x_j|, integers
    """
    n = L.shape[0]
    if sp.issparse(L):
        Lo = L - sp.identity(n, dtype=np.complex128, format="csr")
        l1 = sp.csr_matrix((cabs1(Lo.data), Lo.indices, Lo.indptr), shape=L.shape)
        rowL = np.asarray(l1.sum(axis=1)).ravel()
        fL = _frac_bits(Lo.data)
    else:
        rowL = cabs1(L).sum(axis=1) - 1
        fL = _frac_bits(L)
    udiag = cabs1(np.diagonal(U))
    T = 4 * rowL.max() + max(32.0, udiag.max())
    bits = [np.log2(T) + fL]
    if x is not None:
        y = U @ x
        Ty = (rowL.max() + 1) * cabs1(y).max()
        bits.append(np.log2(Ty) + fL)
        bits.append(np.log2((4 * n + 32) * cabs1(x).max()))       # back substitution, integers
        T = max(T, Ty)
    X = diag_block_inverses(L)
    fD = _frac_bits(X)
    rowD = cabs1(X).sum(axis=2).max()
    bits.append(np.log2(rowD) + fD)                               # the substitution that forms Dinv
    bits.append(np.log2(rowD * T) + fD + fL)                      # Dinv * T in the triangular solves
    return float(max(bits))


# ---------------------------------------------------------------------------------------------------------------------------
# restatement of the dispatch: lu_panel, lu_recurse / lu_trsm / maus_lu_factor, maus_lu_backsolve (csrc/lu.hip)
# ---------------------------------------------------------------------------------------------------------------------------
PT = 512
MW_MAXW = 8
ALL_VARIANTS = frozenset(
    ["rs<2,128>", "rs<2,256>", "rs<2,512>", "mw<1>", "mw<2>", "ip<4,8>", "ip<8,4>", "ip<16,2>", "ip<32,1>"]
    + [f"trsm<{k}>" for k in range(1, 9)] + ["backsolve:whole", "backsolve:blocked", "backsolve:blocked+short_top"])
# lu_panel_ip_kernel<1,8> and <2,8> serve m <= 1024, which lu_panel gives to lu_panel_rs_kernel before it gets there
UNREACHABLE = frozenset(["ip<1,8>", "ip<2,8>"])


def round_up(n, g=32):
    return (n + g - 1) // g * g


def _p2floor(x):
    p = 1
    while 2 * p <= x:
        p *= 2
    return p


def _p2ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def panel_variant(m, G, ncu, mw_allowed, npad):
    """The kernel lu_panel launches for a panel of m rows."""
    if m <= 2 * PT:
        return "rs<2,128>" if m <= 256 else "rs<2,256>" if m <= 512 else "rs<2,512>"
    if mw_allowed and m > 1024 and npad <= 8192:
        wmin = _p2ceil((m + 2 * PT - 1) // (2 * PT))
        wmax = min(_p2floor(max(1, ncu // max(1, G))), MW_MAXW)
        W = max(wmin, min(wmax, _p2floor(m // 256)))
        if 2 <= W <= wmax:
            return "mw<1>" if (m + W * PT - 1) // (W * PT) <= 1 else "mw<2>"
    rpt = (m + PT - 1) // PT
    for r, w in ((1, 8), (2, 8), (4, 8), (8, 4), (16, 2)):
        if rpt <= r:
            return f"ip<{r},{w}>"
    return "ip<32,1>"


def factor_plan(npad, nbo=512):
    """(panel row counts, trsm block counts k / 16, zgemm shapes (M, N, K)) of maus_lu_factor, in launch order."""
    panels, trsms, gemms = [], [], []
    ncols = npad + 32

    def gemm(r0, r1, c0, c1, k0, k1):
        if r1 - r0 > 0 and c1 - c0 > 0 and k1 - k0 > 0:
            gemms.append((r1 - r0, c1 - c0, k1 - k0))

    def trsm(j, k, c_lo, c_hi):
        if c_hi <= c_lo:
            return
        if k <= 128:
            trsms.append(k // 16)
            return
        h = (k // 32) * 16
        trsm(j, h, c_lo, c_hi)
        gemm(j + h, j + k, c_lo, c_hi, j, j + h)
        trsm(j + h, k - h, c_lo, c_hi)

    def recurse(j0, wd):
        if wd <= BLK:
            panels.append(npad - j0)
            return
        h = (wd // (2 * BLK)) * BLK
        recurse(j0, h)
        trsm(j0, h, j0 + h, j0 + wd)
        gemm(j0 + h, npad, j0 + h, j0 + wd, j0, j0 + h)
        recurse(j0 + h, wd - h)

    nbo = max(32, nbo) // 32 * 32
    for J in range(0, npad, nbo):
        wd = min(nbo, npad - J)
        recurse(J, wd)
        trsm(J, wd, J + wd, ncols)
        gemm(J + wd, npad, J + wd, ncols, J, J + wd)
    return panels, trsms, gemms


def trsm_blocks(npad, nbo=512):
    return set(f"trsm<{k}>" for k in factor_plan(npad, nbo)[1])


def panel_variants(npad, G, ncu, mw_allowed, nbo=512):
    return set(panel_variant(m, G, ncu, mw_allowed, npad) for m in factor_plan(npad, nbo)[0])


def backsolve_form(npad, G):
    blocked = True if npad > 8192 else (G <= 64 and npad >= 2048 and npad % 256 == 0)
    if not blocked:
        return {"backsolve:whole"}
    return {"backsolve:blocked"} | ({"backsolve:blocked+short_top"} if npad % 256 else set())


def backsolve_lds_bytes(npad, G):
    """Largest dynamic LDS request of backsolve_kernel (x, a 32 x 33 block, 2 x 32 partial sums of complex doubles)."""
    rows = npad if backsolve_form(npad, G) == {"backsolve:whole"} else min(npad, 256)
    return 16 * (rows + 32 * 33 + 64)


def variants(n, G, ncu, shared, nbo=512):
    npad = round_up(n)
    return panel_variants(npad, G, ncu, not shared, nbo) | trsm_blocks(npad, nbo) | backsolve_form(npad, G)


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
def every(n, step, first, avoid=()):
    """About every step-th column from `first`, moved right past anything in `avoid`."""
    out, used = [], set(avoid)
    for c in range(first, n, step):
        while c in used and c < n - 1:
            c += 1
        if c < n and c not in used:
            out.append(c)
            used.add(c)
    return out


def _case(name, n, G, contexts, reaches, seed, sparse=False, nbo=None, **kw):
    return dict(name=name, n=n, G=G, contexts=contexts, reaches=frozenset(reaches), seed=seed, sparse=sparse, nbo=nbo, kw=kw)


def _table():
    T = []
    for n in (1, 2, 15, 16, 17, 31, 32, 33):
        T.append(_case(f"n{n}", n, 3, ("default",), ["rs<2,128>"] + (["trsm<1>"] if n > 16 else []), 100 + n))
    for n, nb in ((96, 3), (160, 5), (192, 6), (224, 7)):
        T.append(_case(f"n{n}", n, 2, ("default",), [f"trsm<{nb}>"], 200 + n))
    for nbo in (32, 96, 512):
        T.append(_case(f"n224_nbo{nbo}", 224, 2, ("default",), ["trsm<7>"] if nbo == 512 else ["trsm<1>"], 424, nbo=nbo))
    for n in (993, 1024):
        T.append(_case(f"n{n}", n, 2, ("default",), ["rs<2,128>", "rs<2,256>", "rs<2,512>", "trsm<8>", "trsm<4>", "trsm<2>"], 300 + n))
    for n in (1025, 1056):
        T.append(_case(f"n{n}", n, 3, ("default", "shared"), ["mw<1>", "ip<4,8>", "backsolve:whole"], 400 + n))
    T.append(_case("n2048", 2048, 2, ("default",), ["backsolve:blocked"], 2048))
    T.append(_case("n2080", 2080, 1, ("default", "shared"), ["mw<1>", "ip<8,4>", "backsolve:whole"], 2080))
    T.append(_case("n4128", 4128, 1, ("default", "shared"), ["mw<2>", "ip<16,2>"], 4128, sparse=True))
    T.append(_case("n8160", 8160, 1, ("default",), ["backsolve:whole"], 8160, sparse=True))
    T.append(_case("n8224", 8224, 1, ("default",), ["ip<32,1>", "backsolve:blocked+short_top"], 8224, sparse=True))
    return T


TABLE = _table()


def _family(n):
    """The pivot and edge families of one size: name -> keyword arguments of planted() (one matrix each) or a list of them
    (a batch)."""
    ties = every(n, 37, 5)
    rules = every(n, 101, 50, avoid=ties)
    second = 512 + 40 if n > 600 else 100                         # a column of the second outer block (n = 224: under ZERO_NBO)
    F = {}
    for piv in ("identity", "last", "reverse", "random"):
        F[f"piv_{piv}"] = dict(pivots=piv)
        F[f"ties_{piv}"] = dict(pivots=piv, tie_cols=ties)
    F["rules_random"] = dict(pivots="random", rule_cols=rules)
    F["rules_identity"] = dict(pivots="identity", rule_cols=rules)
    F["ties_rules_random"] = dict(pivots="random", tie_cols=ties, rule_cols=rules)
    for c in sorted(set([0, 15, 16, n - 1, second])):
        F[f"zero_{c}"] = dict(pivots="random", zero_cols=[c])
    F["zero_two"] = dict(pivots="random", zero_cols=[n // 3, n // 3 + 21])
    return F


FAMILY_SIZES = (224, 1056)
FAMILIES = {n: _family(n) for n in FAMILY_SIZES}
# n = 224 has one outer block at the default width; its second-outer-block zero column is run under MAUS_LU_NBO = 96
ZERO_NBO = {224: 96, 1056: None}


@functools.lru_cache(maxsize=4)
def _planted_cached(n, seed, sparse, kw):
    return planted(n, seed, sparse_L=sparse, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in kw})


def system(n, seed, sparse=False, **kw):
    """planted(), cached (the default and the shared context of a case solve the same system)."""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
    return _planted_cached(n, seed, sparse, key)


def case_kwargs(case, g):
    """planted() arguments of matrix g of a table case: a pivot family per matrix, tie and rule columns where there is room."""
    n = case["n"]
    kw = dict(pivots=("random", "last", "reverse")[g % 3])
    if n >= 96:
        kw["tie_cols"] = every(n, 37, 5 + g)
        kw["rule_cols"] = every(n, 101, 50 + g, avoid=kw["tie_cols"])
    return kw


def case_batch(case):
    """(A [G, n, n], b [G, n], x, ipiv) of a table case: G planted systems with their own seeds."""
    got = [system(case["n"], case["seed"] + 1000 * g, case["sparse"], **case_kwargs(case, g))[:4] for g in range(case["G"])]
    if case["G"] == 1:
        return tuple(a[None] for a in got[0])
    return tuple(np.stack([t[k] for t in got]) for k in range(4))


def promised(case, context):
    """The instantiations a case promises in one of its contexts: of a case run in both, the multi-workgroup panels belong to
    the default context and the one-workgroup panels to the shared one."""
    both = len(case["contexts"]) == 2
    return {v for v in case["reaches"]
            if not both or not v.startswith(("mw", "ip")) or v.startswith("mw") == (context == "default")}


def family_seed(n, name):
    return 7000 + n + sum(ord(ch) for ch in name)


# ---------------------------------------------------------------------------------------------------------------------------
# unblocked reference LU with a choice of (wrong) pivot rules: the sensitivity checks of the CPU tier
# ---------------------------------------------------------------------------------------------------------------------------
def numpy_lu(A, rule="lapack"):
    """Unblocked right-looking LU.  rule: "lapack" (max |re| + |im|, first index), "last" (last index on ties), "modulus"
    (max |z|, first index), "pad" (the search runs one row past the matrix, where a kernel without its row guard would
    compare whatever its registers hold: modelled as a row of 2^40).  Returns (ipiv, LU)."""
    n = A.shape[0]
    M = np.array(A, dtype=np.complex128)
    if rule == "pad":
        M = np.vstack([M, np.full((1, n), 2.0 ** 40)])
    ipiv = np.zeros(n, dtype=np.int32)
    for j in range(n):
        col = M[j:, j]
        v = np.abs(col) if rule == "modulus" else cabs1(col)
        if rule == "last":
            p = j + len(v) - 1 - int(np.argmax(v[::-1]))
        else:
            p = j + int(np.argmax(v))
        ipiv[j] = p
        if p != j:
            M[[j, p]] = M[[p, j]]
        if M[j, j] != 0:
            M[j + 1:, j] /= M[j, j]
        M[j + 1:, j + 1:] -= np.outer(M[j + 1:, j], M[j, j + 1:])
    return ipiv, M[:n]
