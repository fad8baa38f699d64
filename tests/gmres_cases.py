"""Case table of the batched device GMRES (tests/test_gmres_cases_host.py on the CPU, tests/test_gpu_gmres_edges.py on the
device), the traced restatement that guards the count comparisons, and the checker functions both tiers share.

A case is a dict
    name     unique id
    build    () -> dict(A = ndarray or scipy.sparse matrix, csr = bool, B = k x n right-hand sides, shift = k complex,
                        psi = k float): candidate i solves ((A - shift_i I) + psi_i I) x = B[i] from x0 = B[i]
    jacobi   0 / 1 (every candidate) or a list of k
    rtol, restart, maxiter   as Context.gmres takes them
    mode     "shared": maus_gmres (zgemm / SpMM product); "dense": maus_gmres_pert with PERT_NONE (materialised H_k, GEMV)
    exact    True: every intermediate is a small dyadic number, the device must return SciPy's x bit for bit
and optionally `expect` = (info, inner) of the first candidate where the outcome is known in closed form.

Rounded cases are compared in info, inner count, x (1e-9 relative, the bound of tests/test_gpu_gmres.py) and true residual.
The count can only be compared where no decision of the algorithm sits on its threshold: traced() is the oracle's restatement
with one addition, the distance |ln(value / threshold)| of every decision it takes, and GUARD = 0.01 is the smallest distance
a case of this table may have (rounding moves presid by about 1e-8 relative at rtol = 1e-8: four orders of margin).  The
seeds below were chosen on the CPU so that every case meets it; test_gmres_cases_host.py asserts that."""
import functools

import numpy as np
import scipy.sparse as sp

import scenarios
from oracle import maus_oracle as orc

GUARD = 0.01
EPS = np.finfo(np.float64).eps


def _dist(value, threshold):
    if value == threshold:
        return 0.0
    if value == 0 or threshold == 0 or not (np.isfinite(value) and np.isfinite(threshold)):
        return np.inf
    return abs(float(np.log(value / threshold)))


def traced(H, b, x0, inv_diag, rtol=1e-8, maxiter=50, restart=20):
    """oracle.gmres_restated, statement for statement, plus the distance of every decision from its threshold: rnorm against
    atol, presid against ptol, h1 against eps * h0 on the steps that are no breakdown.
    Returns (x, info, inner, cycles, closest)."""
    n = b.shape[0]
    b = np.asarray(b, dtype=np.complex128)
    x = np.array(x0, dtype=np.complex128, copy=True)
    closest = [np.inf]

    def decide(value, threshold):
        closest[0] = min(closest[0], _dist(value, threshold))

    def psolve(v):
        return v.copy() if inv_diag is None else inv_diag * v

    bnrm2 = np.linalg.norm(b)
    atol = max(0.0, rtol * float(bnrm2))
    if bnrm2 == 0:
        return b.copy(), 0, 0, 0, np.inf
    restart = min(restart, n)
    Mb_nrm2 = np.linalg.norm(psolve(b))
    ptol_max_factor = 1.0
    ptol = Mb_nrm2 * min(ptol_max_factor, atol / bnrm2)
    presid = 0.0
    V = np.empty((restart + 1, n), dtype=np.complex128)
    Hh = np.zeros((restart, restart + 1), dtype=np.complex128)
    giv = np.zeros((restart, 2), dtype=np.complex128)
    inner = 0
    cycles = 0
    rnorm = np.inf
    for cycle in range(maxiter):
        if cycle == 0:
            r = b - H @ x if x.any() else b.copy()
            decide(np.linalg.norm(r), atol)
            if np.linalg.norm(r) < atol:
                return x, 0, inner, cycles, closest[0]
        cycles += 1
        V[0] = psolve(r)
        tmp = np.linalg.norm(V[0])
        V[0] *= (1 / tmp)
        S = np.zeros(restart + 1, dtype=np.complex128)
        S[0] = tmp
        breakdown = False
        col = 0
        for col in range(restart):
            w = psolve(H @ V[col])
            h0 = np.linalg.norm(w)
            for k in range(col + 1):
                t = np.vdot(V[k], w)
                Hh[col, k] = t
                w -= t * V[k]
            h1 = np.linalg.norm(w)
            Hh[col, col + 1] = h1
            V[col + 1] = w
            if h1 <= EPS * h0:
                Hh[col, col + 1] = 0
                breakdown = True
            else:
                decide(h1, EPS * h0)
                V[col + 1] *= (1 / h1)
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
            if not breakdown:
                decide(presid, ptol)
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
        x += y @ V[: col + 1]
        r = b - H @ x
        rnorm = np.linalg.norm(r)
        decide(rnorm, atol)
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
    return x, info, inner, cycles, closest[0]


# ---- operators -------------------------------------------------------------------------------------------------------------
def crand(seed, *shape):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def cyclic(n, unit=1.0):
    """e0 e0^T - 2 unit C, C the cyclic down-shift: GMRES from x0 = b = e0 stagnates completely (every rotation takes the
    f == 0 branch of zlartg) until the cycle closes at step n, where the last rotation takes g == 0."""
    H = np.zeros((n, n), dtype=np.complex128)
    H[0, 0] = 1.0
    H += -2 * unit * np.roll(np.eye(n), 1, axis=0)
    return H


def unit_vector(n, i, value=1.0):
    b = np.zeros(n, dtype=np.complex128)
    b[i] = value
    return b


def banded(n, s, weight=1.0):
    """Complex banded CSR matrix of the size-boundary cases: diagonal 2 + 0.5 sin(0.7 i + s) + 0.3j cos(0.3 i), sub-diagonal
    -0.4 + 0.1j, super-diagonal 0.3j, a diagonal at offset 37 of 0.2 - 0.1j; `weight` scales the three off-diagonals."""
    i = np.arange(n)
    d = 2.0 + 0.5 * np.sin(0.7 * i + s) + 0.3j * np.cos(0.3 * i)
    diags, offs = [d], [0]
    for v, k in ((-0.4 + 0.1j, -1), (0.3j, 1), (0.2 - 0.1j, 37)):
        if n - abs(k) > 0:
            diags.append(np.full(n - abs(k), weight * v, dtype=np.complex128))
            offs.append(k)
    A = sp.csr_matrix(sp.diags(diags, offs, shape=(n, n), dtype=np.complex128, format="csr"))
    A.sort_indices()
    return A


def spread(n, seed, c=0.05):
    """diag(linspace(1, 3, n)) + c G, G with N(0, 1) real and imaginary parts from default_rng(seed)."""
    return np.diag(np.linspace(1.0, 3.0, n)).astype(np.complex128) + c * scenarios.ginibre(n, seed, 1.0)


def shifted_ginibre(n, seed):
    return scenarios.ginibre(n, seed, 1.0) + 3.0 * np.sqrt(n) * np.eye(n)


def _one(A, b, csr=False, shift=0j, psi=0.0):
    return dict(A=A, csr=csr, B=np.asarray(b, dtype=np.complex128)[None, :].copy(),
                shift=np.array([shift], dtype=np.complex128), psi=np.array([psi], dtype=np.float64))


def _case(name, build, jacobi=0, rtol=1e-8, restart=20, maxiter=50, mode="shared", exact=False, expect=None):
    return dict(name=name, build=build, jacobi=jacobi, rtol=rtol, restart=restart, maxiter=maxiter, mode=mode, exact=exact,
                expect=expect)


# ---- the table -------------------------------------------------------------------------------------------------------------
def _exact_cases():
    out = []
    for form, mode, csr in (("zgemm", "shared", False), ("gemv", "dense", False), ("csr", "shared", True)):
        def wrap(A, csr=csr):
            return sp.csr_matrix(A) if csr else A
        for tag, unit in (("re", 1.0), ("im", 1j)):
            for n, mx, exp in ((8, 50, (0, 8)), (20, 50, (0, 20)), (21, 4, (4, 80)), (30, 4, (4, 80))):
                out.append(_case(f"cyclic_{tag}_n{n}_{form}", lambda n=n, unit=unit, wrap=wrap, csr=csr:
                                 _one(wrap(cyclic(n, unit)), unit_vector(n, 0), csr), maxiter=mx, mode=mode, exact=True, expect=exp))
        for jac in (0, 1):
            out.append(_case(f"eigvec_diag40_j{jac}_{form}", lambda wrap=wrap, csr=csr:
                             _one(wrap(np.diag(np.arange(1.0, 41.0)).astype(np.complex128)), unit_vector(40, 3, 2j), csr),
                             jacobi=jac, mode=mode, exact=True, expect=(0, 1)))
    def zero_pivot():
        H = np.zeros((12, 12), dtype=np.complex128)
        H[0, 0] = 1.0
        return _one(H, unit_vector(12, 1))
    out.append(_case("zero_pivot_n12", zero_pivot, maxiter=5, exact=True, expect=(5, 1)))
    out.append(_case("x0_solves_n50", lambda: _one(np.eye(50, dtype=np.complex128), crand(11, 50)), exact=True, expect=(0, 0)))
    out.append(_case("x0_solves_n50_j1", lambda: _one(np.eye(50, dtype=np.complex128), crand(11, 50)), jacobi=1, exact=True,
                     expect=(0, 0)))
    out.append(_case("zero_rhs_n33", lambda: _one(spread(33, 2), np.zeros(33)), exact=True, expect=(0, 0)))
    return out


# Both sides of every size at which maus_gmres_run picks another post kernel (1024, 4096, 8192, 16384) and of the 256 entries
# one pass of a workgroup covers.  Weight 1.0: 16 to 20 inner iterations in one cycle; weight 2.2: 35 to 46 in 2 or 3 cycles.
# Phase s of banded(): 1, except where that puts a decision within 0.02 of its threshold (then the first s that does not).
BOUNDARY_SIZES = (255, 256, 257, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)
BOUNDARY_WEIGHTS = (1.0, 2.2)
BOUNDARY_SEED = {(256, 1, 1): 3, (257, 1, 0): 2}


def _boundary_cases():
    out = []
    for n in BOUNDARY_SIZES:
        for wi, wt in enumerate(BOUNDARY_WEIGHTS):
            for jac in (0, 1):
                s = BOUNDARY_SEED.get((n, wi, jac), 1)
                out.append(_case(f"band_n{n}_w{wi}_j{jac}", lambda n=n, s=s, wt=wt: _one(banded(n, s, wt), crand(n, n), True),
                                 jacobi=jac))
    return out


def _rounded_cases():
    out = _boundary_cases()
    for n in (1024, 1025):
        for jac in (0, 1):
            # 0.05 G has spectral radius 2.3 at this size, the spectrum surrounds the origin: all 50 cycles of 20 iterations
            # stagnate, info = 50, and no decision comes within e^18 of its threshold (the iterate moves by 3e-15 relative when
            # the products are summed in another order).  The second system (G scaled to the unit disk) converges in 20 to 25.
            out.append(_case(f"spread_n{n}_j{jac}", lambda n=n: _one(spread(n, 7), crand(n + 1, n)), jacobi=jac, expect=(50, 1000)))
            out.append(_case(f"spread_conv_n{n}_j{jac}", lambda n=n: _one(spread(n, 7, 0.5 / np.sqrt(n)), crand(n + 1, n)),
                             jacobi=jac))
    sys64 = lambda scale=1.0: _one(spread(64, 7), scale * crand(65, 64))
    for R in (1, 2, 5, 19):
        out.append(_case(f"restart{R}_n64", sys64, restart=R))
    out.append(_case("restart5_n64_j1", sys64, restart=5, jacobi=1))
    out.append(_case("maxiter1_restart4_n64", sys64, restart=4, maxiter=1, expect=(1, 4)))
    for n in (1, 2, 3, 5, 19):
        for jac in (0, 1):
            out.append(_case(f"small_n{n}_j{jac}", lambda n=n: _one(shifted_ginibre(n, 40 + n), crand(60 + n, n)), jacobi=jac))
    out.append(_case("scale_up_n64", lambda: sys64(1e120)))
    out.append(_case("scale_down_n64", lambda: sys64(1e-120)))
    return out


# one cycle of m steps from x0 = b with rtol = 0: x must be the minimiser of ||M (b - H x)|| over x0 + K_m (krylov_minimiser)
ONE_CYCLE = [(64, 8), (300, 12), (1025, 20)]


def _one_cycle_cases():
    out = []
    for n, m in ONE_CYCLE:
        for jac in (0, 1):
            out.append(_case(f"onecycle_n{n}_m{m}_j{jac}", lambda n=n: _one(spread(n, 7), crand(n + 1, n)), jacobi=jac, rtol=0.0,
                             restart=m, maxiter=1, expect=(1, m)))
    return out


def _dense_tail_cases():
    out = []
    for n in (5, 17, 63, 65, 100):
        def build(n=n):
            A = spread(n, 90 + n) if n > 5 else shifted_ginibre(n, 95)
            return dict(A=A, csr=False, B=crand(200 + n, 3, n), shift=np.array([0.1 + 0.2j, -0.3j, 0.25], dtype=np.complex128),
                        psi=np.array([1e-15, 1e-6, 1e-3]))
        out.append(_case(f"dense_tail_n{n}", build, jacobi=[0, 1, 1], mode="dense"))
    return out


EXACT = _exact_cases()
ROUNDED = _rounded_cases()
ONE_CYCLE_CASES = _one_cycle_cases()
DENSE_TAILS = _dense_tail_cases()
CASES = EXACT + ROUNDED + ONE_CYCLE_CASES + DENSE_TAILS
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- batch of 1100 eigenvector-form candidates at n = 64 (gmres_compact_kernel beyond 1024) -----------------------------------
BATCH_N, BATCH_P = 64, 1100
BATCH_ALONE = (0, 63, 64, 1023, 1024, 1099)
BATCH_RESTATED = (1, 36, 37, 38, 500, 777, 1001, 1025, 1073, 1098)


def batch_system():
    """spread(64, 21) with its first coordinate decoupled (A[0, 1:] = A[1:, 0] = 0, A[0, 0] = 2.5).  Every 37th candidate has
    shift 0.5 and right-hand side 2 e0, an exact eigenvector of its H_k (H_k e0 = 2 e0, all of it in small dyadic numbers, with
    and without the Jacobi scale 1/2): it breaks down at column 0 and is finished after one inner iteration while its
    neighbours, Gaussian right-hand sides and shifts, run on.  Jacobi on every odd candidate."""
    n, P = BATCH_N, BATCH_P
    A = spread(n, 21)
    A[0, 1:] = 0.0
    A[1:, 0] = 0.0
    A[0, 0] = 2.5
    B = crand(22, P, n)
    rng = np.random.default_rng(23)
    shift = (rng.standard_normal(P) + 1j * rng.standard_normal(P)) * 0.2
    for i in range(0, P, 37):
        B[i] = unit_vector(n, 0, 2.0)
        shift[i] = 0.5
    psi = np.zeros(P)
    jac = (np.arange(P) % 2).astype(np.int32)
    return A, B, shift, psi, jac


# ---- references and checkers -------------------------------------------------------------------------------------------------
def dense_h(A, shift, psi):
    """H_k with the roundings of the device and of FakeContext: (A - shift I) + psi I."""
    n = A.shape[0]
    return (A - shift * np.eye(n, dtype=np.complex128)) + np.complex128(psi) * np.eye(n, dtype=np.complex128)


def sparse_h(A, shift, psi):
    n = A.shape[0]
    return sp.csr_matrix((A - shift * sp.eye(n, dtype=np.complex128)) + sp.identity(n, dtype=np.complex128, format="csr") * np.complex128(psi))


def jacobi_list(case, k):
    j = case["jacobi"]
    return np.asarray([j] * k if np.isscalar(j) else j, dtype=np.int32)


def systems(case):
    """[(H, b, inv_diag)] of the case's candidates."""
    d = case["build"]()
    k = d["B"].shape[0]
    jac = jacobi_list(case, k)
    out = []
    for i in range(k):
        H = sparse_h(d["A"], d["shift"][i], d["psi"][i]) if d["csr"] else dense_h(d["A"], d["shift"][i], d["psi"][i])
        diag = H.diagonal()
        out.append((H, d["B"][i], (1.0 / diag) if jac[i] else None))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """[(x, info, inner, cycles, closest)] of the case's candidates from traced(); computed once per process."""
    case = BY_NAME[name]
    return [traced(H, b, b, inv, rtol=case["rtol"], maxiter=case["maxiter"], restart=case["restart"]) for H, b, inv in systems(case)]


def run_case(ctx, case):
    """The case through a context (the device's or a test double's) -> (X, info, inner, status)."""
    d = case["build"]()
    k, n = d["B"].shape
    if d["csr"]:
        ctx.set_matrix_csr(d["A"])
    else:
        ctx.set_matrix(d["A"])
    ctx.pop_reserve(k)
    slots = list(range(k))
    ctx.pop_put(0, slots, d["B"])
    jac = jacobi_list(case, k)
    kw = dict(rtol=case["rtol"], restart=case["restart"], maxiter=case["maxiter"])
    if case["mode"] == "dense":
        info, inner, status, used = ctx.gmres_pert(slots, d["shift"], d["psi"], 0, jac, 0, None, **kw)
        assert np.array_equal(np.asarray(used, dtype=bool), jac.astype(bool)), (case["name"], used)
    else:
        info, inner, status = ctx.gmres(slots, d["shift"], d["psi"], 0, jac, **kw)
    return ctx.pop_get(2, slots, n), np.asarray(info), np.asarray(inner), np.asarray(status)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.complex128)
    b = np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_exact(got, ref, tag=""):
    """got = (x, info, inner, status) of one candidate, ref = (x, info, inner, ...): bit for bit."""
    x, info, inner, status = got
    assert int(info) == int(ref[1]), (tag, "info", int(info), int(ref[1]))
    assert int(inner) == int(ref[2]), (tag, "inner", int(inner), int(ref[2]))
    assert int(status) == 0, (tag, "status", int(status))
    assert same_bits(x, ref[0]), (tag, "x differs in", int(np.sum(np.asarray(x) != np.asarray(ref[0]))), "entries")


def check_rounded(got, ref, H, b, rtol, tag="", xtol=1e-9):
    """info and inner count equal to the reference's, ||x - x_ref|| <= xtol ||x_ref||, and where the reference converged the
    true residual in long double within rtol ||b|| (1 + 1e-6)."""
    x, info, inner, status = got
    xr = ref[0]
    assert int(info) == int(ref[1]), (tag, "info", int(info), int(ref[1]))
    assert int(inner) == int(ref[2]), (tag, "inner", int(inner), int(ref[2]))
    assert int(status) == 0, (tag, "status", int(status))
    err = np.linalg.norm(x - xr)
    assert err <= xtol * np.linalg.norm(xr), (tag, "x", err / np.linalg.norm(xr))
    if int(ref[1]) == 0:
        res = residual_norm_ld(H, x, b)
        bn = np.sqrt(np.sum(np.abs(b).astype(np.longdouble) ** 2))
        assert res <= np.longdouble(rtol) * bn * (1 + 1e-6), (tag, "residual", float(res / bn))


def residual_norm_ld(H, x, b):
    """||b - H x|| with the products and sums in long double."""
    x = np.asarray(x)
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    if sp.issparse(H):
        C = sp.coo_matrix(H)
        pr = C.data.real.astype(np.longdouble) * xr[C.col] - C.data.imag.astype(np.longdouble) * xi[C.col]
        pi = C.data.real.astype(np.longdouble) * xi[C.col] + C.data.imag.astype(np.longdouble) * xr[C.col]
        yr = np.zeros(H.shape[0], dtype=np.longdouble)
        yi = np.zeros(H.shape[0], dtype=np.longdouble)
        np.add.at(yr, C.row, pr)
        np.add.at(yi, C.row, pi)
    else:
        Hr, Hi = H.real.astype(np.longdouble), H.imag.astype(np.longdouble)
        yr, yi = Hr @ xr - Hi @ xi, Hr @ xi + Hi @ xr
    rr, ri = b.real.astype(np.longdouble) - yr, b.imag.astype(np.longdouble) - yi
    return np.sqrt(np.sum(rr * rr + ri * ri))


def check_case(case, got):
    """All candidates of a case against the traced reference: check_exact for the exact cases, check_rounded for the others."""
    X, info, inner, status = got
    ref = reference(case["name"])
    for i, (H, b, inv) in enumerate(systems(case)):
        g = (X[i], info[i], inner[i], status[i])
        tag = f"{case['name']}[{i}]"
        if case["exact"]:
            check_exact(g, ref[i], tag)
        else:
            check_rounded(g, ref[i], H, b, case["rtol"], tag)
    if case["expect"] is not None:
        assert (int(info[0]), int(inner[0])) == tuple(case["expect"]), (case["name"], int(info[0]), int(inner[0]))


def krylov_minimiser(H, b, inv_diag, m):
    """argmin ||M (b - H x)|| over x0 + K_m(M H, M (b - H x0)), x0 = b, with no code of the restatement: Krylov basis by
    classical Gram-Schmidt applied twice per vector, least squares by np.linalg.lstsq."""
    M = (lambda v: v) if inv_diag is None else (lambda v: inv_diag * v)
    r0 = M(b - H @ b)
    Q = np.empty((b.shape[0], m), dtype=np.complex128)
    v = r0
    for j in range(m):
        for _ in range(2):
            v = v - Q[:, :j] @ (Q[:, :j].conj().T @ v)
        Q[:, j] = v / np.linalg.norm(v)
        v = M(H @ Q[:, j])
    W = np.stack([M(H @ Q[:, j]) for j in range(m)], axis=1)
    y = np.linalg.lstsq(W, r0, rcond=None)[0]
    return b + Q @ y


# the restatement's own distance from the minimiser, relative to ||x - x0||: a few roundings times the condition of the m-column
# least-squares problem (measured 4e-16 .. 1.1e-15 on the systems of ONE_CYCLE); above this the independent reference itself
# is in doubt and the case has to be replaced
ONE_CYCLE_OWN_MAX = 1e-13


def check_one_cycle(case, got):
    """x after one cycle of m steps against krylov_minimiser: the device may deviate 64 x as far as the restatement does on the
    same system (the margin covers the 256-way reduction order).  Returns (device deviation / restatement deviation,
    restatement deviation)."""
    (H, b, inv), = systems(case)
    xm = krylov_minimiser(H, b, inv, case["restart"])
    scale = np.linalg.norm(xm - b)
    own = np.linalg.norm(reference(case["name"])[0][0] - xm) / scale
    dev = np.linalg.norm(got[0][0] - xm) / scale
    assert own <= ONE_CYCLE_OWN_MAX, (case["name"], "restatement vs minimiser", own)
    assert dev <= 64 * own, (case["name"], "device vs minimiser", dev, "restatement", own)
    return dev / own, own
