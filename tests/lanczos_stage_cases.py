"""Cases, references and checks for the stages of the device Lanczos (csrc/lanczos.hip: maus_lanczos_begin / _inject / _extend /
_restart / _finish, maus_herm_match_rows), importable without a GPU.  A "stepper" is any object with the Lanczos methods of
_cabi.Context (set_matrix_csr, lanczos_begin / _inject / _extend / _restart / _finish / _get_basis, get_ritz_rows, pop_reserve /
pop_put / pop_get, herm_match_rows, matvec_rayleigh); every run_* function takes `make`, a callable that returns a fresh one.
tests/test_lanczos_stage_host.py runs the table through FakeLanczosContext and through the NumPy restatement below (which must
fail a named check under each of the planted faults); tests/test_gpu_lanczos_stages.py runs it through the device.

u = 2^-53, eps = 2 u, gamma_k = k u / (1 - k u).  A sum whose every term passes through at most k rounded operations, in whatever
tree, has error at most gamma_k sum |terms| (Higham, Accuracy and Stability, section 4.2); a complex multiply-add is two real
FMAs per part with |a_r b_r| + |a_i b_i| <= |a| |b|, so a per-part bound gamma_k sum |a| |b| is sqrt(2) times that in modulus.

Check S (one step, local).  After begin and extend(0, ncv, tol) the rows 0 .. ncv are read back.  For each j the step is recomputed
in np.clongdouble FROM THE DEVICE'S OWN ROWS 0 .. j (Krylov sequences diverge from a one-ulp difference; a local comparison does
not): w = A v_j, two classical Gram-Schmidt passes h_p = V^H w, w -= V^T h_p, alpha_j = Re(h_1[j] + h_2[j]), beta_j = ||w||,
row j + 1 = w / beta_j.  The bound is a running one: beside every reference quantity walks a bound on how far the device's can be
from it, each stage adding its own rounding to what it inherits.  With e = |A| |v_j| (componentwise), s_j = ||e||_2, V the rows
0 .. j (cnt = j + 1 of them), c = ceil(nblk / 256) and nblk = ceil(n / 512):
    product   E_w = sqrt(2) gamma_{2 L + 2} e                  L = the longest row: 2 L FMAs per part in any order (the wave
                                                               schedule splits a row over lanes and joins them in a tree)
    dots      E_h[i] = sqrt(2) gamma_D |v_i| . (|w| + E_w) + |v_i| . E_w
                  D = 4 + 6 + 3 + c + 8: two entries of two FMAs per part in a thread, six DPP levels, the workgroup's four waves
                  added in index order, c strided adds of the partial sums, and the tree of lz_block_sum (6 + 2) once more
    update    E_w <- E_w + |V|^T E_h + sqrt(2) gamma_{2 cnt + 1} (|w| + E_w + |V|^T (|h| + E_h))       a chain of cnt complex FMAs
    alpha     E_a = E_h1[j] + E_h2[j] + u (|alpha| + E_h1[j] + E_h2[j])
    beta      E_b = ||E_w||_2 + (N / 2 + 2) u (beta + ||E_w||_2),   N = 4 + 8 + c + 8: the sum of squares by the same tree has
                  relative error gamma_N (no cancellation), the root halves it and rounds once
    row       E_r = (E_w + |w| E_b / beta + 2.5 u (|w| + E_w)) / (beta - E_b)      the reciprocal and the product round once each
Every term is linear in e, so E_a and E_b scale with s_j and E_r with s_j / beta_j; they are kept termwise (componentwise for the
row) instead of being collapsed into one constant times s_j, and each record prints error / (eps s_j) beside error / bound.  The
assertion is error <= 2 E: the factor 2 covers the reference's own rounding (np.sum adds pairwise: about 30 x 2^-64 relative to
sum |terms|, a hundredth of u) and what is of second order in u.  Where E = 0 (a zero row behind a breakdown: every operand is an
exact zero) the device's value must be the reference's exactly.  A step whose reported beta is not above tol must leave a zero
row, any other a non-zero one; where beta - E_b <= 0 (a breakdown the threshold did not cut) the row has no bound and is only
required to be finite.  Row 0 is v0 / ||v0|| within (n + 5) u componentwise: kernel_refs.check_norm's (n + 2) u for the norm, one
rounding each for the reciprocal and the product, one to spare.
A float64 NumPy restatement (class Restatement) sits at 0.05 - 0.25 eps s_j / beta_j in the worst entry of a row and below 0.6 eps s_j
for alpha and beta on these operators, which is below one hundredth of the derived bounds: they are correct, not tight, and a
lost entry, stretch or partial sum still misses them by orders of magnitude (the host test shows it).  They are a priori: nothing in them was
measured on a device.

Check O (whole sweep).  g = max |B B^H - I| over the non-zero rows 0 .. ncv and f = ||A V_m - V_m T - beta_m v_{m+1} e_m^T||_F /
||A||_1 (m = ncv, T from the reported alpha and beta), both in np.clongdouble, each at most 8 x max(the restatement's value on the
same case, ncv eps): herm_cases.BOUND's factor and reasoning -- two backward-stable computations that differ in the order of
summation, ncv eps the rounding of storing ncv + 1 rows.  The same rule holds |R R^H - I| of the Ritz rows after finish.
The restatement's values (g / eps, f / eps), recomputed and held within a factor of two by the host test:
RECORDED_O below.  With one Gram-Schmidt pass instead of two the shifted lattice (lattice(23, 23) + 2^20 I: beta / ||A v|| is about
2e-6) gives g above 1e-8 instead of 1.6 eps: that is the case which shows the second pass (check S sees it there too, at row 2).

Restart: rows 0 .. keep - 1 against S^T B[:m] in np.clongdouble, real and imaginary parts separately within
gamma_{m + 1} sum_r |S[r, i]| |B[r, x]| (a chain of m FMAs per part), row keep bit-equal to the old row m, rows keep + 1 .. ncv
bit-equal to what they were.  Finish: row q against the np.clongdouble recombination, then the same running bound through the two
Gram-Schmidt passes against the device's own rows 0 .. q - 1.  Match: the Ritz rows are unit vectors (injected, then selected by a
permutation S), so every score has one non-zero term and is exact; idx is np.argmax of the np.longdouble |scores| wherever the two
leading ones differ by more than 2 sqrt(2) kernel_refs.rayleigh_bound (everywhere, for these inputs: asserted), the norm is held by
kernel_refs.check_norm and the written row is kernel_refs.scale_ref(R[idx], norm) bit for bit."""
import contextlib
import functools
import math

import numpy as np
import scipy.sparse as sp

import kernel_refs as kr
import lanczos_cases

U = 2.0 ** -53
EPS = 2.0 * U
LD, CLD = np.longdouble, np.clongdouble
SQ2 = math.sqrt(2.0)
SPAN = 512                                    # entries of n per workgroup of a step (LZ_SPAN)
JOIN = 256                                    # partial sums a join adds per trip (LZ_BT)
MSPAN = 4096                                  # entries of n per workgroup of the match (LZ_MSPAN)
MAXV, MAXK = 32, 8                            # LZ_MAXV, LZ_MAXK
CHUNK = 32768                                 # candidates per launch of the match
O_FACTOR = 8.0                                # check O: times max(the restatement's value, ncv eps)
SLACK = 2.0                                   # check S: error <= SLACK * running bound

# the restatement's check-O values per step case, in units of eps: (g / eps, f / eps)
RECORDED_O = {
    "tri_n1_ncv1": (0.20, 0.0), "tri_n2_ncv2": (0.84, 0.36), "tri_n33_ncv32": (1.43, 1.94),
    "tri_n255_ncv20": (1.05, 1.58), "tri_n256_ncv20": (1.36, 1.64), "tri_n257_ncv20": (0.96, 1.50),
    "tri_n511_ncv20": (1.60, 1.63), "tri_n512_ncv20": (1.65, 1.64), "tri_n513_ncv20": (1.44, 1.67),
    "tri_n1023_ncv20": (1.46, 1.92), "tri_n1025_ncv20": (1.06, 2.11),
    "lattice32x33_ncv32": (1.91, 2.30), "shifted23x23_ncv20": (1.59, 2.60), "wide513_ncv20": (1.37, 0.96),
    "tri_n131072_ncv4": (1.32, 0.46), "tri_n131073_ncv4": (1.43, 0.47), "big": (2.10, 0.30),
}


def gam(k):
    return k * U / (1.0 - k * U)


# ---- operators ------------------------------------------------------------------------------------------------------------------
def _csr(A):
    A = sp.csr_matrix(A, dtype=np.complex128)
    A.sum_duplicates()
    A.sort_indices()
    return A


def shifted_lattice():
    return _csr(lanczos_cases.lattice(23, 23) + 2.0 ** 20 * sp.identity(23 * 23, dtype=np.complex128, format="csr"))


def wide_rows(n=513, half=20, seed=11):
    """Random Hermitian pattern, about 2 half = 40 entries per row, and a real diagonal: the SpMM's wave schedule."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), half)
    c = rng.integers(0, n, size=r.size)
    v = rng.standard_normal(r.size) + 1j * rng.standard_normal(r.size)
    off = r != c
    B = sp.csr_matrix((v[off], (r[off], c[off])), shape=(n, n))
    A = _csr(B + B.conj().T + sp.diags(4.0 + rng.standard_normal(n)).astype(np.complex128))
    assert A.nnz > 32 * n and abs(A - A.conj().T).max() == 0.0
    return A


def pair_swap(n):
    """The permutation A e_{2i} = e_{2i+1}, A e_{2i+1} = e_{2i} (n even): every quantity of a step from a unit vector is exact."""
    assert n % 2 == 0
    i = np.arange(n)
    return _csr(sp.csr_matrix((np.ones(n), (i, i ^ 1)), shape=(n, n)))


# name -> (kind, n, ncv)
STEP_CASES = {"tri_n1_ncv1": ("tri", 1, 1), "tri_n2_ncv2": ("tri", 2, 2), "tri_n33_ncv32": ("tri", 33, 32)}
for _n in (255, 256, 257, 511, 512, 513, 1023, 1025):
    STEP_CASES[f"tri_n{_n}_ncv20"] = ("tri", _n, 20)
STEP_CASES["lattice32x33_ncv32"] = ("lattice", 32 * 33, 32)
STEP_CASES["shifted23x23_ncv20"] = ("shifted", 23 * 23, 20)
STEP_CASES["wide513_ncv20"] = ("wide", 513, 20)
STEP_CASES["tri_n131072_ncv4"] = ("tri", 131072, 4)
STEP_CASES["tri_n131073_ncv4"] = ("tri", 131073, 4)
STEP_NAMES = list(STEP_CASES)
BIG_N = (1 << 20) + 1                         # nblk = 257 in the match, 2049 in a step
BIG_CASE = ("tri", BIG_N, 2)


@functools.lru_cache(maxsize=4)
def operator(kind, n):
    if kind == "tri":
        return _csr(lanczos_cases.tridiagonal(n)) if n > 1 else _csr(sp.csr_matrix(np.array([[4.25 + 0j]])))
    if kind == "lattice":
        assert n == 32 * 33
        return _csr(lanczos_cases.lattice(32, 33))
    if kind == "shifted":
        return shifted_lattice()
    if kind == "wide":
        return wide_rows(n)
    if kind == "swap":
        return pair_swap(n)
    raise KeyError(kind)


def start_vector(n):
    rng = np.random.default_rng(1)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def anorm1(A):
    return float(abs(A).sum(axis=0).max())


def unit(n, p, phase=1.0):
    v = np.zeros(n, dtype=np.complex128)
    v[p] = phase
    return v


@contextlib.contextmanager
def opened(make):
    st = make()
    try:
        yield st
    finally:
        close = getattr(st, "close", None)
        if close is not None:
            close()


# ---- extended-precision pieces -----------------------------------------------------------------------------------------------------
def _mod(z):
    """|z| of a (long double) complex array as float64, rounded up by a hair."""
    return (np.hypot(z.real, z.imag) * LD(1.0 + 4 * U)).astype(np.float64)


class Csr:
    """A in extended precision: A @ v and |A| @ |v| by segmented pairwise sums over the stored rows."""

    def __init__(self, A):
        self.n = A.shape[0]
        self.indices = A.indices
        counts = np.diff(A.indptr)
        self.rows = np.flatnonzero(counts > 0)
        self.starts = A.indptr[:-1][self.rows]
        self.data = A.data.astype(CLD)
        self.adata = np.abs(A.data).astype(LD)
        self.longest = int(counts.max()) if self.n else 0
        self.anorm1 = anorm1(A)

    def _seg(self, terms):
        out = np.zeros(self.n, dtype=terms.dtype)
        if len(self.starts):
            out[self.rows] = np.add.reduceat(terms, self.starts)
        return out

    def dot(self, v):
        return self._seg(self.data * v[self.indices])

    def absdot(self, av):
        return self._seg(self.adata * av[self.indices])


def _sumsq(w):
    return np.sum(w.real * w.real + w.imag * w.imag)


def _joins(n):
    nblk = (n + SPAN - 1) // SPAN
    return max(1, (nblk + JOIN - 1) // JOIN)


def gs_reference(V, w, Ew, n):
    """Two classical Gram-Schmidt passes of w (np.clongdouble, exact input) against the rows V (cnt x n, the device's own), the
    norm and the scaled row, with the running bounds of the module docstring; Ew bounds |device's w - w| on entry."""
    cnt = V.shape[0]
    c = _joins(n)
    gd, gu, nn = gam(4 + 6 + 3 + c + 8), gam(2 * cnt + 1), 4 + 8 + c + 8
    aV = _mod(V) if cnt else None
    hs, Ehs = [], []
    for _ in range(2):
        if cnt:
            aw = _mod(w) + Ew
            h = np.sum(V.conj() * w[None, :], axis=1)
            Eh = SQ2 * gd * (aV @ aw) + aV @ Ew
            ah = _mod(h) + Eh
            Ew = Ew + aV.T @ Eh + SQ2 * gu * (aw + aV.T @ ah)
            for i in range(cnt):
                w = w - h[i] * V[i]
        else:
            h, Eh = np.zeros(0, dtype=CLD), np.zeros(0)
        hs.append(h)
        Ehs.append(Eh)
    beta = float(np.sqrt(_sumsq(w)))
    nEw = float(np.linalg.norm(Ew)) * (1.0 + 8 * U)
    Eb = nEw + (nn / 2.0 + 2.0) * U * (beta + nEw)
    aw = _mod(w)
    if beta - Eb > 0.0:
        row = w / LD(np.sqrt(_sumsq(w)))
        Er = (Ew + aw * (Eb / beta) + 2.5 * U * (aw + Ew)) / (beta - Eb)
    else:
        row, Er = None, None
    return {"h": hs, "Eh": Ehs, "w": w, "Ew": Ew, "beta": beta, "Eb": Eb, "row": row, "Er": Er}


def _ratio(err, bound):
    """max error / bound, an error where the bound is zero counting as infinite"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


def _nonzero(row):
    return bool(np.any(row.view(np.float64) != 0.0))


# ---- check S --------------------------------------------------------------------------------------------------------------------
def check_row0(B0, v0):
    ref = v0.astype(CLD) / LD(kr.norm_ref(v0))
    n = v0.size
    r = _ratio(_mod(B0.astype(CLD) - ref), (n + 5) * U * _mod(ref))
    assert r <= 1.0, f"check S: row 0 is {r:.3g} times (n + 5) u |v0| / ||v0|| away from v0 / ||v0||"
    return r


def check_s(A, B, alpha, beta, tol, j0=0, tag=""):
    """Steps j0 .. j0 + len(alpha) - 1 against the local extended-precision recomputation.  Returns the worst error / (2 E) of
    alpha, beta and the rows, and the worst errors in units of eps s_j (eps s_j / beta_j for the rows)."""
    X = Csr(A)
    n = X.n
    assert np.all(np.isfinite(B.view(np.float64))) and np.all(np.isfinite(alpha)) and np.all(np.isfinite(beta)), \
        f"check S: {tag}: non-finite output"
    Bl = B.astype(CLD)
    rec = {"alpha": 0.0, "beta": 0.0, "row": 0.0, "alpha_eps_s": 0.0, "beta_eps_s": 0.0, "row_eps_s_beta": 0.0}
    for k in range(len(alpha)):
        j = j0 + k
        v = Bl[j]
        av = _mod(v)
        e = X.absdot(av.astype(LD)).astype(np.float64)
        s = float(np.linalg.norm(e))
        g = gs_reference(Bl[:j + 1], X.dot(v), SQ2 * gam(2 * X.longest + 2) * e, n)
        a_ref = float((g["h"][0][j] + g["h"][1][j]).real)
        Ea = g["Eh"][0][j] + g["Eh"][1][j]
        Ea = Ea + U * (abs(a_ref) + Ea)
        ea = abs(float(LD(alpha[k]) - (g["h"][0][j] + g["h"][1][j]).real))
        eb = abs(float(LD(beta[k]) - LD(g["beta"])))
        ra, rb = _ratio(ea, SLACK * Ea), _ratio(eb, SLACK * g["Eb"])
        assert ra <= 1.0, f"check S: {tag}: alpha[{j}] = {alpha[k]!r}, reference {a_ref!r}: error / bound = {ra:.3g}"
        assert rb <= 1.0, f"check S: {tag}: beta[{j}] = {beta[k]!r}, reference {g['beta']!r}: error / bound = {rb:.3g}"
        rec["alpha"], rec["beta"] = max(rec["alpha"], ra), max(rec["beta"], rb)
        if s > 0.0:
            rec["alpha_eps_s"], rec["beta_eps_s"] = max(rec["alpha_eps_s"], ea / (EPS * s)), max(rec["beta_eps_s"], eb / (EPS * s))
        new = B[j + 1]
        if not beta[k] > tol:
            assert not _nonzero(new), f"check S: {tag}: beta[{j}] = {beta[k]!r} is not above tol = {tol!r}, yet row {j + 1} is not zero"
            continue
        assert _nonzero(new), f"check S: {tag}: beta[{j}] = {beta[k]!r} is above tol = {tol!r}, yet row {j + 1} is zero"
        if g["row"] is None:
            continue
        er = _mod(Bl[j + 1] - g["row"])
        rr = _ratio(er, SLACK * g["Er"])
        assert rr <= 1.0, f"check S: {tag}: row {j + 1}: error / bound = {rr:.3g} at entry {int(np.argmax(er / np.maximum(g['Er'], 1e-300)))}"
        rec["row"] = max(rec["row"], rr)
        if s > 0.0:
            rec["row_eps_s_beta"] = max(rec["row_eps_s_beta"], float(er.max()) * g["beta"] / (EPS * s))
    return rec


# ---- check O --------------------------------------------------------------------------------------------------------------------
def gram_defect(B):
    """max |B B^H - I| over the non-zero rows, in extended precision (pairwise sums)."""
    Bl = [B[i].astype(CLD) for i in range(B.shape[0]) if _nonzero(B[i])]
    worst = 0.0
    for i in range(len(Bl)):
        for j in range(i, len(Bl)):
            d = np.sum(Bl[i].conj() * Bl[j]) - (1.0 if i == j else 0.0)
            worst = max(worst, float(np.hypot(d.real, d.imag)))
    return worst


def sweep_values(A, B, alpha, beta):
    """(g, f) of check O for the rows 0 .. m of a sweep from row 0 (m = len(alpha))."""
    X = Csr(A)
    m = len(alpha)
    Bl = B.astype(CLD)
    ss = LD(0.0)
    for j in range(m):
        r = X.dot(Bl[j]) - LD(alpha[j]) * Bl[j] - LD(beta[j]) * Bl[j + 1]
        if j:
            r = r - LD(beta[j - 1]) * Bl[j - 1]
        ss += _sumsq(r)
    return gram_defect(B[:m + 1]), float(np.sqrt(ss)) / X.anorm1


def o_rule(value, own, ncv):
    return np.isfinite(value) and value <= O_FACTOR * max(own, ncv * EPS)


def _sweep(st, A, v0, ncv, tol):
    st.set_matrix_csr(A)
    st.lanczos_begin(v0, ncv)
    alpha, beta = st.lanczos_extend(0, ncv, tol)
    return st.lanczos_get_basis(0, ncv + 1), np.array(alpha), np.array(beta)


def case_inputs(name):
    kind, n, ncv = BIG_CASE if name == "big" else STEP_CASES[name]
    A = operator(kind, n)
    return A, start_vector(n), ncv, EPS * anorm1(A)


@functools.lru_cache(maxsize=None)
def restatement_o(name):
    """(g, f) of the float64 restatement on a step case: check O's yardstick, computed once."""
    A, v0, ncv, tol = case_inputs(name)
    return sweep_values(A, *_sweep(Restatement(), A, v0, ncv, tol))


def check_o(name, A, B, alpha, beta):
    g0, f0 = restatement_o(name)
    ncv = len(alpha)
    g, f = sweep_values(A, B, alpha, beta)
    assert o_rule(g, g0, ncv), f"check O: {name}: max |B B^H - I| = {g / EPS:.3g} eps, the restatement's {g0 / EPS:.3g} eps"
    assert o_rule(f, f0, ncv), f"check O: {name}: Lanczos relation {f / EPS:.3g} eps ||A||_1, the restatement's {f0 / EPS:.3g} eps"
    return {"g_eps": g / EPS, "f_eps": f / EPS, "g": g / (O_FACTOR * max(g0, ncv * EPS)), "f": f / (O_FACTOR * max(f0, ncv * EPS))}


def _show(name, rec):
    print(f"STAGE {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in rec.items()))


def run_step_case(name, make, records=None):
    """begin, one sweep, checks S and O.  Returns the worst ratios."""
    A, v0, ncv, tol = case_inputs(name)
    with opened(make) as st:
        B, alpha, beta = _sweep(st, A, v0, ncv, tol)
    rec = {"row0": check_row0(B[0], v0)}
    rec.update(check_s(A, B, alpha, beta, tol, tag=name))
    rec.update(check_o(name, A, B, alpha, beta))
    _show(name, rec)
    if records is not None:
        records[name] = rec
    return rec


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def _bits(got, ref, what):
    kr.check_bits(np.ascontiguousarray(got) + 0.0, np.ascontiguousarray(ref) + 0.0, what)


def run_exact_cases(make):
    """The pair-swap operator and unit vectors: every row, alpha and beta is exactly representable."""
    n, ncv = 514, 32
    A = operator("swap", n)
    with opened(make) as st:
        st.set_matrix_csr(A)
        st.lanczos_begin(unit(n, 0), ncv)
        alpha, beta = st.lanczos_extend(0, 1, 0.0)
        assert alpha[0] == 0.0 and beta[0] == 1.0, f"exact: first step gives alpha {alpha[0]!r}, beta {beta[0]!r}"
        _bits(st.lanczos_get_basis(0, 2), np.array([unit(n, 0), unit(n, 1)]), "exact: rows 0, 1 after one step")
        alpha, beta = st.lanczos_extend(1, 4, 0.0)            # A e_1 = e_0: the Krylov space is exhausted
        assert np.array_equal(alpha, np.zeros(3)) and np.array_equal(beta, np.zeros(3)), f"exact: breakdown gives {alpha!r}, {beta!r}"
        want = np.zeros((ncv + 1, n), dtype=np.complex128)
        want[0, 0] = want[1, 1] = 1.0
        _bits(st.lanczos_get_basis(0, 5), want[:5], "exact: rows 0 .. 4 after the breakdown")
        for j in range(2, ncv + 1):
            st.lanczos_inject(j, unit(n, 2 * j, 1j))
            want[j, 2 * j] = 1j
            if j in (2, 3, ncv - 1, ncv):
                _bits(st.lanczos_get_basis(0, ncv + 1)[:j + 1], want[:j + 1], f"exact: rows 0 .. {j} after inject({j}, i e_{2 * j})")
        _bits(st.lanczos_get_basis(ncv, 1), want[ncv:], "exact: row 32 alone")
        _bits(st.lanczos_get_basis(7, 3), want[7:10], "exact: rows 7 .. 9")
        for bad in ((-1, 1), (0, ncv + 2), (ncv, 2), (ncv + 1, 1)):
            try:
                st.lanczos_get_basis(*bad)
            except Exception:
                continue
            raise AssertionError(f"exact: get_basis{bad} did not refuse")


# ---- threshold ------------------------------------------------------------------------------------------------------------------
def run_threshold(make, name="tri_n513_ncv20", j=3):
    A, v0, ncv, _tol = case_inputs(name)
    with opened(make) as st:
        st.set_matrix_csr(A)

        def upto(tol_last):
            st.lanczos_begin(v0, ncv)
            if j:
                st.lanczos_extend(0, j, 0.0)
            a, b = st.lanczos_extend(j, j + 1, tol_last)
            return float(a[0]), float(b[0]), st.lanczos_get_basis(0, j + 2)

        a0, b0, B0 = upto(0.0)
        assert b0 > 0.0 and _nonzero(B0[j + 1])
        a1, b1, B1 = upto(b0)
        assert (a1, b1) == (a0, b0), f"threshold: alpha, beta changed with tol_abs: {(a1, b1)!r} against {(a0, b0)!r}"
        assert not _nonzero(B1[j + 1]), "threshold: beta == tol_abs must leave a zero row (beta > tol_abs is strict)"
        kr.check_bits(B1[:j + 1], B0[:j + 1], "threshold: the rows before the step")
        a2, b2, B2 = upto(float(np.nextafter(b0, 0.0)))
        assert (a2, b2) == (a0, b0)
        kr.check_bits(B2, B0, "threshold: tol_abs one ulp below beta must give the first run's rows")
        st.lanczos_begin(v0, ncv)
        a, b = st.lanczos_extend(0, j + 1, float("inf"))
        B3 = st.lanczos_get_basis(0, j + 2)
        st.lanczos_begin(v0, ncv)
        af, bf = st.lanczos_extend(0, 1, 0.0)
        assert a[0] == af[0] and b[0] == bf[0] and b[0] > 0.0, "threshold: tol_abs = inf must still report the first beta"
        assert not np.any(a[1:]) and not np.any(b[1:]), "threshold: steps from a zero row report alpha = beta = 0"
        assert not np.any(B3[1:].view(np.float64)), "threshold: tol_abs = inf must leave every new row zero"
        kr.check_bits(B3[0], B0[0], "threshold: row 0")


# ---- restart and finish ---------------------------------------------------------------------------------------------------------
RESTARTS = ((32, 32, 31), (32, 32, 1), (20, 20, 12), (20, 2, 1))            # (ncv, m, keep)
FINISHES = ((32, 32, 8, "eigh"), (20, 20, 6, "eigh"), (20, 20, 1, "eigh"), (20, 1, 1, "eigh"), (20, 20, 6, "random"))  # (ncv, m, k, S)
BASIS_N = 513


def _tridiag(alpha, beta, m):
    T = np.diag(np.asarray(alpha[:m], dtype=np.float64))
    if m > 1:
        T += np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    return T


def random_s(m, k, seed=5):
    S = np.random.default_rng(seed).standard_normal((m, k))
    assert np.linalg.cond(S) <= 10.0
    return S


def _s_matrix(alpha, beta, m, cols, kind):
    if kind == "random":
        return random_s(m, cols)
    _w, Z = np.linalg.eigh(_tridiag(alpha, beta, m))
    return np.ascontiguousarray(Z[:, m - cols:])


def _basis(st, ncv):
    A = operator("tri", BASIS_N)
    B, alpha, beta = _sweep(st, A, start_vector(BASIS_N), ncv, EPS * anorm1(A))
    return A, B, alpha, beta


def combine_reference(S, B):
    """(S^T B in np.clongdouble, the per-part bounds on the real and on the imaginary parts)."""
    m = S.shape[0]
    Sl = S.astype(LD)
    re = np.zeros((S.shape[1], B.shape[1]), dtype=LD)
    im = np.zeros_like(re)
    for r in range(m):
        re += Sl[r][:, None] * B[r].real.astype(LD)[None, :]
        im += Sl[r][:, None] * B[r].imag.astype(LD)[None, :]
    aS = np.abs(S).T
    g = gam(m + 1)
    return re, im, g * (aS @ np.abs(B[:m].real)), g * (aS @ np.abs(B[:m].imag))


def run_restart(make, ncv, m, keep, records=None):
    with opened(make) as st:
        _A, B, alpha, beta = _basis(st, ncv)
        S = _s_matrix(alpha, beta, m, keep, "eigh")
        st.lanczos_restart(S)
        N = st.lanczos_get_basis(0, ncv + 1)
    re, im, bre, bim = combine_reference(S, B[:m])
    r = max(_ratio(np.abs((N[:keep].real - re).astype(np.float64)), bre), _ratio(np.abs((N[:keep].imag - im).astype(np.float64)), bim))
    assert np.all(np.isfinite(N.view(np.float64))) and r <= 1.0, \
        f"restart ({m}, {keep}): rows 0 .. {keep - 1} are {r:.3g} times gamma_(m+1) sum |S| |B| away from S^T B"
    kr.check_bits(N[keep], B[m], f"restart ({m}, {keep}): row keep against the old row m")
    kr.check_bits(N[keep + 1:], B[keep + 1:], f"restart ({m}, {keep}): rows behind keep")
    rec = {"combine": r}
    _show(f"restart_ncv{ncv}_m{m}_keep{keep}", rec)
    if records is not None:
        records[f"restart_{m}_{keep}"] = rec
    return rec


@functools.lru_cache(maxsize=None)
def restatement_ritz_defect(ncv, m, k, kind):
    st = Restatement()
    _A, _B, alpha, beta = _basis(st, ncv)
    st.lanczos_finish(_s_matrix(alpha, beta, m, k, kind))
    return gram_defect(st.get_ritz_rows())


def _refuses(call, what):
    try:
        call()
    except Exception:
        return
    raise AssertionError(f"{what} did not refuse")


def run_finish(make, ncv, m, k, kind, records=None):
    with opened(make) as st:
        _A, B, alpha, beta = _basis(st, ncv)
        S = _s_matrix(alpha, beta, m, k, kind)
        st.lanczos_finish(S)
        R = st.get_ritz_rows()
        _refuses(lambda: st.lanczos_get_basis(0, 1), "finish: get_basis after finish (the basis is freed)")
    assert R.shape == (k, BASIS_N) and np.all(np.isfinite(R.view(np.float64)))
    re, im, bre, bim = combine_reference(S, B[:m])
    C = np.empty(re.shape, dtype=CLD)
    C.real, C.imag = re, im
    Rl = R.astype(CLD)
    worst = 0.0
    for q in range(k):
        g = gs_reference(Rl[:q], C[q], np.hypot(bre[q], bim[q]) * (1.0 + 4 * U), BASIS_N)
        assert g["row"] is not None
        r = _ratio(_mod(Rl[q] - g["row"]), SLACK * g["Er"])
        assert r <= 1.0, f"finish ({m}, {k}, {kind}): Ritz row {q}: error / bound = {r:.3g}"
        worst = max(worst, r)
    d, d0 = gram_defect(R), restatement_ritz_defect(ncv, m, k, kind)
    assert o_rule(d, d0, ncv), f"finish ({m}, {k}, {kind}): check O: max |R R^H - I| = {d / EPS:.3g} eps, the restatement's {d0 / EPS:.3g} eps"
    rec = {"row": worst, "g_eps": d / EPS, "g": d / (O_FACTOR * max(d0, ncv * EPS))}
    _show(f"finish_ncv{ncv}_m{m}_k{k}_{kind}", rec)
    if records is not None:
        records[f"finish_{m}_{k}_{kind}"] = rec
    return rec


def run_finish_drops(make):
    with opened(make) as st:
        _basis(st, 20)
        st.lanczos_finish(np.zeros((20, 0)))
        _refuses(st.get_ritz_rows, "finish with k = 0: get_ritz_rows")
        _refuses(lambda: st.lanczos_get_basis(0, 1), "finish with k = 0: get_basis")


# ---- match ----------------------------------------------------------------------------------------------------------------------
PHASES = (complex(1.0, 0.0), complex(0.0, 1.0), complex(-1.0, 0.0), complex(0.0, -1.0))      # no negative zeros
MATCH_CASES = [(n, k) for n in (4095, 4096, 4097) for k in (1, 6, 8)]
MATCH_COUNTS = (1, 3, 9)


def positions(n, k):
    out = []
    for p in (n - 1, 0, 4095, 4096, 255, 256, 511, 512, 2048, 1, 2, 3):
        if 0 <= p < n and p not in out:
            out.append(p)
    assert len(out) >= k
    return out[:k]


def unit_ritz_rows(st, n, pos):
    """Ritz rows that are exact: unit vectors injected one by one, finished with the reversing permutation.  Returns them."""
    k = len(pos)
    st.lanczos_begin(unit(n, pos[0], PHASES[0]), k)
    for j in range(1, k):
        st.lanczos_inject(j, unit(n, pos[j], PHASES[j % 4]))
    st.lanczos_finish(np.ascontiguousarray(np.eye(k)[:, ::-1]))
    want = np.array([unit(n, pos[j], PHASES[j % 4]) for j in range(k)])[::-1]
    _bits(st.get_ritz_rows(), want, "match: the unit Ritz rows")
    return np.ascontiguousarray(want)


def score_reference(R, x):
    """vdot(x, R[j]) as (re, im) in np.longdouble, by the device's own real formulas (so inf and NaN travel as they do there)."""
    xr, xi = x.real.astype(LD), x.imag.astype(LD)
    rr, ri = R.real.astype(LD), R.imag.astype(LD)
    with np.errstate(invalid="ignore"):
        return np.sum(rr * xr + ri * xi, axis=1), np.sum(ri * xr - rr * xi, axis=1)


def undecided(R, X):
    """Candidates whose two leading |scores| lie within twice the dot-product bound of each other."""
    out = 0
    for x in X:
        if R.shape[0] < 2 or not np.all(np.isfinite(x.view(np.float64))):
            continue
        re, im = score_reference(R, x)
        a = np.sort(np.hypot(re, im).astype(np.float64))
        bound = max(kr.rayleigh_bound(x, R[j]) for j in range(R.shape[0]))
        out += int(a[-1] - a[-2] <= 2.0 * SQ2 * bound)
    return out


def check_match(R, X, idx, nrm, rows, tag):
    assert undecided(R, X) == 0, f"match: {tag}: the inputs leave candidates undecided"
    worst = 0.0
    for g, x in enumerate(X):
        re, im = score_reference(R, x)
        with np.errstate(invalid="ignore"):
            want = int(np.argmax(np.hypot(re, im)))
        assert int(idx[g]) == want, f"match: {tag}: idx[{g}] = {int(idx[g])}, np.argmax of the reference scores gives {want}"
        try:
            worst = max(worst, kr.check_norm(nrm[g], R[want], "norm_out"))
        except AssertionError as e:
            raise AssertionError(f"match: {tag}: norm of candidate {g}: {e}") from None
        kr.check_bits(rows[g], kr.scale_ref(R[want], nrm[g]), f"match: {tag}: the row written for candidate {g}")
    return worst


def _match(st, n, X, slots, cap=None):
    st.pop_reserve(cap if cap is not None else int(max(slots)) + 1)
    st.pop_put(0, slots, X)
    idx, nrm = st.herm_match_rows(slots)
    return idx, nrm, st.pop_get(0, slots, n)


def run_match_case(make, n, k):
    A = operator("tri", n)
    with opened(make) as st:
        st.set_matrix_csr(A)
        R = unit_ritz_rows(st, n, positions(n, k))
        for count in MATCH_COUNTS:
            rng = np.random.default_rng([n, k, count])
            X = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
            slots = rng.permutation(count + 3)[:count]
            idx, nrm, rows = _match(st, n, X, slots, cap=12)
            check_match(R, X, idx, nrm, rows, f"n = {n}, k = {k}, {count} candidates")


def crafted_candidates(n, pos):
    """(X, expected idx) for Ritz rows R[i] = phase e_{pos[k - 1 - i]}, k = 6: a tie, two infinities, all NaN."""
    k = len(pos)
    at = lambda i: pos[k - 1 - i]                                   # the position where Ritz row i is not zero
    rng = np.random.default_rng(77)
    X = 0.1 * (rng.random((4, n)) + 1j * rng.random((4, n)))
    X[0, at(1)], X[0, at(4)] = 5.0, -5.0                            # |score| 5 exactly for rows 1 and 4: the first wins
    X[1, at(0)] = np.inf                                            # row 0 scores (inf, NaN) -> |.| = inf; every other row NaN
    X[2, at(2)] = np.inf                                            # rows 0 and 1 score NaN already
    X[3, :] = complex(np.nan, np.nan)
    return X, [1, 1, 0, 0]


def run_match_crafted(make, n=4097, k=6):
    A = operator("tri", n)
    pos = positions(n, k)
    with opened(make) as st:
        st.set_matrix_csr(A)
        R = unit_ritz_rows(st, n, pos)
        X, want = crafted_candidates(n, pos)
        slots = np.array([2, 0, 5, 3])
        idx, nrm, rows = _match(st, n, X, slots, cap=8)
    for g in range(len(want)):
        re, im = score_reference(R, X[g])
        with np.errstate(invalid="ignore"):
            assert int(np.argmax(np.hypot(re, im))) == want[g]              # the reference agrees with the stated order
        assert int(idx[g]) == want[g], f"match: crafted candidate {g}: idx = {int(idx[g])}, np.argmax's order gives {want[g]}"
        kr.check_norm(nrm[g], R[want[g]], f"match: crafted candidate {g}: norm_out")
        kr.check_bits(rows[g], kr.scale_ref(R[want[g]], nrm[g]), f"match: crafted candidate {g}: the row written")


def run_match_zero_row(make, n=514):
    """Ritz rows (0, e_0, e_1) from the pair-swap breakdown: the norms of the rows differ, so the norm of the wrong row shows."""
    A = operator("swap", n)
    with opened(make) as st:
        st.set_matrix_csr(A)
        st.lanczos_begin(unit(n, 0), 3)
        st.lanczos_extend(0, 2, 0.0)
        st.lanczos_finish(np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]))
        R = np.array([np.zeros(n), unit(n, 0), unit(n, 1)], dtype=np.complex128)
        _bits(st.get_ritz_rows(), R, "match: Ritz rows with a zero row")
        rng = np.random.default_rng(9)
        X = rng.standard_normal((5, n)) + 1j * rng.standard_normal((5, n))
        slots = np.array([4, 1, 0, 6, 2])
        idx, nrm, rows = _match(st, n, X, slots, cap=7)
    check_match(R, X, idx, nrm, rows, "zero Ritz row")
    assert set(int(i) for i in idx) <= {1, 2}


def run_match_stamps(make, n=4097, k=6):
    """matvec_rayleigh of a replaced slot after a match against a fresh stepper holding the same row: a product kept from
    before the match must not be served."""
    A = operator("tri", n)
    rng = np.random.default_rng(21)
    X = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    slots = np.array([1, 3, 0])
    with opened(make) as st:
        st.set_matrix_csr(A)
        st.pop_reserve(4)
        st.pop_put(0, slots, X)
        before = st.matvec_rayleigh(slots)
        unit_ritz_rows(st, n, positions(n, k))
        st.herm_match_rows(slots[:2])
        rows = st.pop_get(0, slots, n)
        num, den = st.matvec_rayleigh(slots)
    with opened(make) as fresh:
        fresh.set_matrix_csr(A)
        fresh.pop_reserve(4)
        fresh.pop_put(0, slots, rows)
        num0, den0 = fresh.matvec_rayleigh(slots)
    kr.check_bits(rows[2], X[2], "match: stamps: the slot that was not matched")
    kr.check_bits(np.array(num), np.array(num0), "match: stamps: Rayleigh numerators after the match")
    kr.check_bits(np.array(den), np.array(den0), "match: stamps: Rayleigh denominators after the match")
    kr.check_bits(np.array(num[2:]), np.array(before[0][2:]), "match: stamps: the untouched slot's numerator")


def run_match_chunks(make, n=64, count=CHUNK + 1):
    """32769 candidates in distinct slots: the second launch of the chunk loop, with its offsets into slots, idx and norms."""
    A = operator("tri", n)
    rng = np.random.default_rng(13)
    X = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    slots = rng.permutation(count)
    with opened(make) as st:
        st.set_matrix_csr(A)
        R = unit_ritz_rows(st, n, [n - 1, 0])
        idx, nrm, rows = _match(st, n, X, slots, cap=count)
    # vectorised check_match: one non-zero per Ritz row, so a score is one product
    a = np.abs(np.stack([X[:, 0], X[:, n - 1]], axis=1))           # R[0] = i e_0, R[1] = e_{n-1}
    assert np.all(np.abs(a[:, 0] - a[:, 1]) > 1e-9), "match: chunks: the inputs leave candidates undecided"
    want = np.argmax(a, axis=1)
    bad = np.flatnonzero(np.asarray(idx) != want)
    assert bad.size == 0, f"match: chunks: {bad.size} wrong idx, first at candidate {bad[0]} (slot {slots[bad[0]]})"
    assert np.array_equal(np.asarray(nrm), np.ones(count)), "match: chunks: norm_out"
    kr.check_bits(rows, R[want], "match: chunks: the rows written")


def run_big(make, records=None):
    """n = 2^20 + 1: a sweep of two steps (2049 partial sums per dot: nine trips of the strided join) under checks S and O, then
    unit Ritz rows in the first and in the last workgroup of the match (257 partial sums: its second trip) and three candidates."""
    A, v0, ncv, tol = case_inputs("big")
    n = BIG_N
    with opened(make) as st:
        B, alpha, beta = _sweep(st, A, v0, ncv, tol)
        R = unit_ritz_rows(st, n, [n - 1, 5])
        rng = np.random.default_rng(3)
        X = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        X[0, n - 1], X[1, n - 1], X[2, n - 1] = 3.0, 0.25j, -2.0              # the last entry decides: it lies in block 256
        X[0, 5], X[1, 5], X[2, 5] = 1.0, 1.0, 1.0
        slots = np.array([2, 0, 1])
        idx, nrm, rows = _match(st, n, X, slots, cap=3)
    rec = {"row0": check_row0(B[0], v0)}
    rec.update(check_s(A, B, alpha, beta, tol, tag="big"))
    rec.update(check_o("big", A, B, alpha, beta))
    check_match(R, X, idx, nrm, rows, "n = 2^20 + 1")
    assert [int(i) for i in idx] == [1, 0, 1]                       # R[1] = e_{n-1}, R[0] = i e_5
    _show("big", rec)
    if records is not None:
        records["big"] = rec
    return rec


# ---- a plain float64 restatement of the steps, with planted faults --------------------------------------------------------------------
FAULTS = ("dot_tail", "norm_stretch", "join_blocks", "join_blocks_match", "one_pass", "no_conj", "alpha_prev", "threshold_ge", "s_transposed",
          "restart_in_place", "keep_row_first", "tie_last", "nan_ignored", "wrong_norm")


class Restatement:
    """The device's steps in float64 NumPy, in NumPy's own order of summation.  `fault` plants one of FAULTS:
    dot_tail          the last entry of n is left out of the dots
    norm_stretch      the second 512-stretch is left out of the norm
    join_blocks       the partial sums beyond the 256th are left out of the joins of a step (entries from 256 x 512 on)
    join_blocks_match the same in the match (entries from 256 x 4096 on)
    one_pass          the second Gram-Schmidt pass is skipped
    no_conj           the dots do not conjugate
    alpha_prev        alpha is taken from h[j - 1]
    threshold_ge      beta >= tol_abs instead of beta > tol_abs
    s_transposed      S is read transposed
    restart_in_place  the restart recombines row by row in place, reading rows it has already replaced
    keep_row_first    row keep receives row m before the recombination has read it
    tie_last          a tie of |scores| goes to the last index
    nan_ignored       NaN scores are ignored
    wrong_norm        the norm of row 0 is reported, and used, whatever row was picked"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault
        self.A = None
        self.rows = self.cols = 0
        self.B = self.R = None
        self.X = None

    def close(self):
        pass

    # -- data
    def set_matrix_csr(self, A):
        A = _csr(A)
        if A.shape != (self.rows, self.cols):
            self.X = None
        self.A = A
        self.rows, self.cols = A.shape
        self.B = self.R = None

    def matrix_is_sparse(self):
        return "wave" if self.A.nnz > 32 * self.rows else "rows"

    def pop_reserve(self, cap):
        if self.X is None or self.X.shape[0] < cap:
            new = np.zeros((cap, self.rows), dtype=np.complex128)
            if self.X is not None:
                new[:self.X.shape[0]] = self.X
            self.X = new

    def pop_put(self, which, slots, vecs):
        assert which == 0
        self.X[np.asarray(slots)] = np.asarray(vecs, dtype=np.complex128).reshape(len(slots), -1)

    def pop_get(self, which, slots, length):
        assert which == 0
        return self.X[np.asarray(slots), :length].copy()

    def matvec_rayleigh(self, slots):
        num = np.array([np.vdot(self.X[s], self.A @ self.X[s]) for s in slots])
        den = np.array([np.vdot(self.X[s], self.X[s]) for s in slots])
        return num, den

    # -- the pieces of a step
    def _dots(self, V, w):
        n = w.size
        hi = n - 1 if self.fault == "dot_tail" else min(n, JOIN * SPAN) if self.fault == "join_blocks" else n
        Vs = V[:, :hi]
        return (Vs if self.fault == "no_conj" else Vs.conj()) @ w[:hi]

    def _norm(self, w):
        if self.fault == "norm_stretch":
            w = np.concatenate([w[:SPAN], w[2 * SPAN:]])
        elif self.fault == "join_blocks":
            w = w[:JOIN * SPAN]
        return float(np.sqrt(np.sum(w.real * w.real + w.imag * w.imag)))

    def _orth(self, V, w):
        hs = []
        for _ in range(1 if self.fault == "one_pass" else 2):
            h = self._dots(V, w) if len(V) else np.zeros(0, dtype=np.complex128)
            if len(V):
                w = w - V.T @ h
            hs.append(h)
        if len(hs) == 1:
            hs.append(np.zeros_like(hs[0]))
        return hs, w

    def _scaled(self, w, nrm, tol, strict=True):
        above = nrm > tol if strict else nrm >= tol
        return kr.scale_ref(w, nrm) if above else np.zeros_like(w)

    # -- the entry points
    def lanczos_begin(self, v0, ncv):
        assert 1 <= ncv <= min(self.rows, MAXV)
        self.B = np.zeros((ncv + 1, self.rows), dtype=np.complex128)
        self.R = None
        self.lanczos_inject(0, v0)

    def lanczos_inject(self, j, v):
        assert self.B is not None and 0 <= j < self.B.shape[0]
        _hs, w = self._orth(self.B[:j], np.array(v, dtype=np.complex128))
        self.B[j] = self._scaled(w, self._norm(w), 0.0)

    def lanczos_extend(self, j0, j1, tol_abs):
        assert self.B is not None and 0 <= j0 < j1 <= self.B.shape[0] - 1 and tol_abs >= 0.0
        alpha, beta = np.zeros(j1 - j0), np.zeros(j1 - j0)
        for j in range(j0, j1):
            hs, w = self._orth(self.B[:j + 1], self.A @ self.B[j])
            i = j - 1 if self.fault == "alpha_prev" and j > 0 else j
            alpha[j - j0] = hs[0][i].real + hs[1][i].real
            beta[j - j0] = self._norm(w)
            self.B[j + 1] = self._scaled(w, beta[j - j0], tol_abs, strict=self.fault != "threshold_ge")
        return alpha, beta

    def _s(self, S):
        S = np.ascontiguousarray(S, dtype=np.float64)
        return S.ravel().reshape(S.shape[1], S.shape[0]).T if self.fault == "s_transposed" else S

    def lanczos_restart(self, S):
        m, keep = S.shape
        assert self.B is not None and 1 <= keep < m <= self.B.shape[0] - 1
        S = self._s(S)
        if self.fault == "restart_in_place":
            last = self.B[m].copy()
            for i in range(keep):
                self.B[i] = S[:, i] @ self.B[:m]
            self.B[keep] = last
        elif self.fault == "keep_row_first":
            self.B[keep] = self.B[m]
            self.B[:keep] = S.T @ self.B[:m]
        else:
            new, last = S.T @ self.B[:m], self.B[m].copy()
            self.B[:keep] = new
            self.B[keep] = last

    def lanczos_finish(self, S):
        m, k = S.shape
        assert self.B is not None
        self.R = None
        if k:
            assert 1 <= k <= min(m, MAXK) and m <= self.B.shape[0] - 1
            R = self._s(S).T @ self.B[:m]
            for q in range(k):
                _hs, w = self._orth(R[:q], R[q])
                R[q] = self._scaled(w, self._norm(w), 0.0)
            self.R = R
        self.B = None

    def lanczos_get_basis(self, j0, count):
        assert self.B is not None and 0 <= j0 and 1 <= count and j0 + count <= self.B.shape[0]
        return self.B[j0:j0 + count].copy()

    def get_ritz_rows(self):
        assert self.R is not None
        return self.R.copy()

    def herm_match_rows(self, slots):
        assert self.R is not None and self.X is not None
        R, n = self.R, self.rows
        hi = min(n, JOIN * MSPAN) if self.fault == "join_blocks_match" else n
        idx, nrm = np.empty(len(slots), dtype=np.int32), np.empty(len(slots))
        for g, s in enumerate(slots):
            x = self.X[s, :hi]
            with np.errstate(invalid="ignore"):
                re = np.sum(R[:, :hi].real * x.real + R[:, :hi].imag * x.imag, axis=1)
                im = np.sum(R[:, :hi].imag * x.real - R[:, :hi].real * x.imag, axis=1)
                a = np.hypot(re, im)
            if self.fault == "tie_last":
                j = len(a) - 1 - int(np.argmax(a[::-1]))
            elif self.fault == "nan_ignored":
                j = 0 if np.all(np.isnan(a)) else int(np.nanargmax(a))
            else:
                j = int(np.argmax(a))
            nrm[g] = self._norm(R[0] if self.fault == "wrong_norm" else R[j])
            idx[g] = j
            with np.errstate(divide="ignore", invalid="ignore"):
                self.X[s] = kr.scale_ref(R[j], nrm[g])
        return idx, nrm
