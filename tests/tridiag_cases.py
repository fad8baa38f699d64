"""Adversarial real symmetric tridiagonal matrices for the device eigen-solver (csrc/herm.hip: tri_bisect_kernel,
tri_twisted_kernel, tri_scale_kernel, tri_resid_kernel and the host part tri_solve), a NumPy restatement of that solver, and
the checks that tests/test_tridiag_cases_host.py (CPU) and tests/test_gpu_tridiag_cases.py (device) apply to a result.

CASES is the table: (name, d, e, verdict) with verdict "device" (engine.device_eigh keeps the device vectors) or "host" (the
gap test must send the problem to LAPACK dstemr).  Every n is the smallest at which the feature exists.  Two conditions hold
for the whole table (asserted on the restatement by the host test):
    * no case has gap / ||T|| inside [1e-9, 1e-5], so that the device and the restatement cannot disagree on the verdict through
      the rounding of a vector or of an eigenvalue;
    * no case has a residual above 10 * 1e-15.
Random members are seeded; a seed that landed in either band was replaced, the bands were not widened.

restate() repeats Context._scaled_tridiagonal, tri_solve and the four kernels operation by operation, vectorised over the
eigenvalue index.  Its eigenvalues are meant to be the device's bit for bit: the bisection contains no product that feeds a
sum (e2 = e * e is rounded on the host, 0.5 * x is exact), so contraction into fma cannot change it, and fp64 division is
correctly rounded.  Its vectors are not: the device contracts (d - lam) - l * e into one fma.

certify() is independent of both and of LAPACK: the number of negative pivots of the L D L^T of T - x in 50-digit arithmetic
is the number of eigenvalues below x (Sylvester), so w is the spectrum of T to within delta when count(w_i - delta) <= i and
count(w_i + delta) >= i + 1 for every i.  delta = ratio * eps * ||T|| + floor, where the floor is what no fp64 bisection with
dstebz's pivot guard can resolve: 2 pivmin (a pivot smaller than pivmin is counted as negative; pivmin = safmin * max(1,
emax^2) in the solver's power-of-two scaling) plus half the spacing of the subnormal numbers (the rounding of any fp64 result;
it matters for the matrix scaled by 1e-310 only, where it is 5e-15 ||T||).  The pivmin term is below 1e-307 ||T|| whenever ||T|| > 0.

CERT_RECORDED is the largest certifying ratio measured on the restatement over the table (host test; ladder of powers of two)
and CERT_BAR = 4 * CERT_RECORDED the bar every eigenvalue check uses -- DESIGN section 13.
"""
import functools
import math

import numpy as np

EPS = 2.220446049250313e-16
SAFMIN = 2.2250738585072014e-308
MIN_GAP = 1e-7                 # engine.TRIDIAG_MIN_GAP and TRIDIAG_MAX_RESID (the GPU test asserts that they are these)
MAX_RESID = 1e-13
GAP_BAND = (1e-9, 1e-5)
RESID_BAND = 10 * 1e-15
CERT_LADDER = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
CERT_RECORDED = 1.0            # measured by test_tridiag_cases_host.py::test_certificate_ratio_is_the_recorded_one
CERT_BAR = 4 * CERT_RECORDED


# ---- the table --------------------------------------------------------------------------------------------------------------
def _gauss(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), rng.standard_normal(max(n - 1, 0))


def _wilkinson(m):
    return np.abs(np.arange(-m, m + 1)).astype(np.float64), np.ones(2 * m)


def _build_cases():
    c = []
    for n in (65, 257):
        c.append((f"toeplitz_2_-1_n{n}", np.full(n, 2.0), np.full(n - 1, -1.0), "device"))
    for n in (63, 64):
        c.append((f"toeplitz_0_1_n{n}", np.zeros(n), np.ones(n - 1), "device"))
    k = np.arange(1, 40)
    c.append(("clement_n40", np.zeros(40), np.sqrt(k * (40.0 - k)), "device"))
    d, e = _gauss(64, 101)
    e[[15, 31, 47]] = 0.0
    c.append(("reducible_n64", d, e, "device"))
    # even significands: the bisection then returns d_k itself, and d_k - lambda is an exact zero for the guard to catch
    c.append(("diagonal_n8", np.array([3.0, -1.0, 4.0, 1.5, -9.0, 2.5, 6.0, 0.5]), np.zeros(7), "device"))
    c.append(("single_n1", np.array([-3.5]), np.zeros(0), "device"))
    c.append(("pair_e0_n2", np.array([1.0, -2.0]), np.array([0.0]), "device"))
    c.append(("pair_n2", np.array([1.0, -2.0]), np.array([0.75]), "device"))
    d, e = _gauss(30, 102)
    c.append(("negative_offdiag_n30", d, -np.abs(e) - 0.01, "device"))
    d, e = _gauss(20, 103)
    c.append(("tiny_offdiag_n20", d, np.full(19, 1e-200), "device"))
    c.append(("localised_n100", np.arange(1.0, 101.0), np.full(99, 1e-3), "device"))
    c.append(("localised_n300", np.arange(1.0, 301.0), np.full(299, 1e-4), "device"))
    d, e = _gauss(24, 104)
    for tag, f in (("1e-310", 1e-310), ("1e-150", 1e-150), ("1e140", 1e140), ("1e300", 1e300)):
        c.append((f"scale_{tag}_n24", d * f, e * f, "device"))
    # seeds: the first ones found (LAPACK eigenvalues, CPU) with min gap / ||T|| above 3e-5; the spacing of a random
    # tridiagonal matrix is Poissonian, so most seeds at n = 513 land inside the gap band
    for n, seed in ((255, 204), (256, 200), (257, 203), (513, 1236)):
        d, e = _gauss(n, seed)
        c.append((f"block_edge_n{n}", d, e, "device"))
    d, e = _wilkinson(10)
    c.append(("wilkinson21", d, e, "host"))
    c.append(("glued_wilkinson_n63", np.concatenate([d, d, d]),
              np.concatenate([e, [1e-8], e, [1e-8], e]), "host"))
    k = np.arange(64)
    c.append(("graded_n64", 10.0 ** (-k / 4.0), 10.0 ** (-k[:-1] / 4.0 - 1.0), "host"))
    c.append(("scalar_2.5_n4", np.full(4, 2.5), np.zeros(3), "host"))
    c.append(("zero_n4", np.zeros(4), np.zeros(3), "host"))
    c.append(("repeated_diagonal_n5", np.array([2.0, 5.0, 1.0, 3.0, 2.0]), np.zeros(4), "host"))   # the pair is gap 1 of 0..3
    for _, d, e, _ in c:
        d.setflags(write=False)
        e.setflags(write=False)
    return tuple(c)


CASES = _build_cases()
NAMES = tuple(c[0] for c in CASES)
BY_NAME = {c[0]: c for c in CASES}
ACCEPTED = tuple(c[0] for c in CASES if c[3] == "device")
REJECTED = tuple(c[0] for c in CASES if c[3] == "host")


def analytic(name):
    """(eigenvalues ascending, eigenvectors as columns or None) in long double for the families with a closed form."""
    _, d, e, _ = BY_NAME[name]
    n = d.shape[0]
    ld = np.longdouble
    if name.startswith("toeplitz"):
        k = np.arange(1, n + 1, dtype=ld)
        j = np.arange(1, n + 1, dtype=ld)
        pi = ld(math.pi) + ld(1.2246467991473532e-16)                      # pi to long double precision
        U = np.sqrt(ld(2) / (n + 1)) * np.sin(np.outer(j, k) * pi / (n + 1))   # column k - 1: sin(j k pi / (n + 1))
        if name.startswith("toeplitz_2_-1"):
            return 2 - 2 * np.cos(k * pi / (n + 1)), U
        return (2 * np.cos(k * pi / (n + 1)))[::-1].copy(), U[:, ::-1].copy()
    if name.startswith("clement"):
        return np.arange(-(n - 1), n, 2).astype(ld), None
    return None


# ---- the restatement --------------------------------------------------------------------------------------------------------
def scaled_tridiagonal(d, e):
    """Context._scaled_tridiagonal: T / s with s the power of two below the largest entry (exact)."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    n = d.shape[0]
    t = max(float(np.max(np.abs(d))) if n else 0.0, float(np.max(np.abs(e))) if n > 1 else 0.0)
    s = 2.0 ** int(np.floor(np.log2(t))) if t > 0.0 else 1.0
    return n, d / s, (e / s if n > 1 else np.zeros(0)), s


def host_scalars(d, e):
    """The host part of tri_solve on the scaled matrix: (gl, gu, tnorm, pivmin, tiny), gl and gu already widened."""
    n = d.shape[0]
    d, e = [float(x) for x in d], [float(x) for x in e]
    gl = gu = d[0]
    emax = 0.0
    for k in range(n):
        a = (abs(e[k - 1]) if k > 0 else 0.0) + (abs(e[k]) if k + 1 < n else 0.0)
        gl = min(gl, d[k] - a)
        gu = max(gu, d[k] + a)
        if k + 1 < n:
            emax = max(emax, abs(e[k]))
    tnorm = max(abs(gl), abs(gu))
    pivmin = SAFMIN * max(1.0, emax * emax)
    gl -= 2.0 * EPS * n * tnorm + 2.0 * pivmin
    gu += 2.0 * EPS * n * tnorm + 2.0 * pivmin
    return gl, gu, tnorm, pivmin, EPS * max(tnorm, SAFMIN / EPS)


def bisect(d, e2, gl, gu, pivmin, count_ge=False):
    """tri_bisect_kernel for every eigenvalue index at once (lanes that have left the loop are dropped from the arrays)."""
    n = d.shape[0]
    lo, hi = np.full(n, gl), np.full(n, gu)
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(1100):
            if idx.size == 0:
                break
            l, h = lo[idx], hi[idx]
            mid = 0.5 * (l + h)
            go = (mid > l) & (mid < h)
            idx, l, h, mid = idx[go], l[go], h[go], mid[go]
            if idx.size == 0:
                break
            q = d[0] - mid
            q = np.where(np.abs(q) < pivmin, -pivmin, q)
            cnt = (q < 0.0).astype(np.int64)
            for k in range(1, n):
                q = (d[k] - mid) - e2[k - 1] / q
                q = np.where(np.abs(q) < pivmin, -pivmin, q)
                cnt += q < 0.0
            up = (cnt >= idx) if count_ge else (cnt > idx)
            hi[idx] = np.where(up, mid, h)
            lo[idx] = np.where(up, l, mid)
    return 0.5 * (lo + hi)


def twisted(d, e, w, tiny, twist_last=False, guard_on=True):
    """tri_twisted_kernel, tri_scale_kernel and tri_resid_kernel: (Z[k][i] normalised, res[i])."""
    n = d.shape[0]
    ez = np.zeros(n)
    ez[: n - 1] = e

    def guard(x):
        return np.where(np.abs(x) < tiny, np.copysign(tiny, x), x) if guard_on else x

    with np.errstate(all="ignore"):
        Dp, Dm = np.empty((n, n)), np.empty((n, n))
        dp = guard(d[0] - w)
        Dp[0] = dp
        for k in range(n - 1):
            l = ez[k] / dp
            dp = guard((d[k + 1] - w) - l * ez[k])
            Dp[k + 1] = dp
        dm = guard(d[n - 1] - w)
        Dm[n - 1] = dm
        best = np.abs(dp + dm - (d[n - 1] - w))
        r = np.full(n, n - 1)
        for k in range(n - 2, -1, -1):
            u = ez[k] / dm
            dm = guard((d[k] - w) - u * ez[k])
            Dm[k] = dm
            g = np.abs(Dp[k] + dm - (d[k] - w))
            if not twist_last:
                take = g < best
                best = np.where(take, g, best)
                r = np.where(take, k, r)
        Z = np.zeros((n, n))
        cols = np.arange(n)
        Z[r, cols] = 1.0
        for k in range(n - 2, -1, -1):
            m = k < r
            Z[k, m] = -(ez[k] / Dp[k, m]) * Z[k + 1, m]
        for k in range(n - 1):
            m = k >= r
            Z[k + 1, m] = -(ez[k] / Dm[k + 1, m]) * Z[k, m]
        ss = np.ones(n)                                            # z_k^2 in the order the kernel adds them: r - 1 .. 0, r + 1 .. n - 1
        for k in range(n - 2, -1, -1):
            m = k < r
            ss[m] += Z[k, m] * Z[k, m]
        for k in range(1, n):
            m = k > r
            ss[m] += Z[k, m] * Z[k, m]
        Z *= 1.0 / np.sqrt(ss)
        worst = np.zeros(n)
        for k in range(n):
            rk = (d[k] - w) * Z[k]
            if k > 0:
                rk = ez[k - 1] * Z[k - 1] + rk
            if k + 1 < n:
                rk = ez[k] * Z[k + 1] + rk
            worst = np.fmax(worst, np.abs(rk))
    return Z, worst


class Result:
    """What Context.herm_tridiag_eig returns, plus what it leaves on the device: w, (gap, resid, tnorm), Z[k][i]; ws and s are
    the eigenvalues before the final w * s and the scale, tnorm_s is ||T|| of the scaled matrix (diag[2] = tnorm_s * s rounds
    when T is subnormal)."""
    def __init__(self, w, diag, Z, ws, s, tnorm_s=None):
        self.w, self.diag, self.Z, self.ws, self.s, self.tnorm_s = w, diag, Z, ws, s, tnorm_s

    @property
    def verdict(self):
        gap, resid, _ = self.diag
        return "device" if bool(np.isfinite(self.w).all()) and gap >= MIN_GAP and resid <= MAX_RESID else "host"


def restate(d, e, count_ge=False, twist_last=False, guard_on=True, gap_stride=1, vectors=True):
    """Context.herm_tridiag_eig (vectors=False: herm_tridiag_eigvals) restated.  The keyword arguments switch on the wrong rules
    that the host test must be able to tell from the right ones."""
    n, ds, es, s = scaled_tridiagonal(d, e)
    gl, gu, tnorm, pivmin, tiny = host_scalars(ds, es)
    ws = bisect(ds, es * es, gl, gu, pivmin, count_ge=count_ge)
    if not vectors:
        return Result(ws * s, None, None, ws, s, tnorm)
    Z, res = twisted(ds, es, ws, tiny, twist_last=twist_last, guard_on=guard_on)
    scale = tnorm if tnorm > 0.0 else 1.0
    finite = bool(np.all(res == res) and np.all(ws == ws))
    gap = float(np.min(np.diff(ws)[::gap_stride])) / scale if n > 1 else 1.0
    resid = float(np.max(res)) / scale if finite else 1e300
    return Result(ws * s, (gap, resid, tnorm * s), Z, ws, s, tnorm)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's result for a tabled case, computed once per process and not to be modified."""
    _, d, e, _ = BY_NAME[name]
    r = restate(d, e)
    for a in (r.w, r.Z, r.ws):
        a.setflags(write=False)
    return r


# ---- the certificate --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mp():
    """A 50-digit mpmath context of our own: the global one keeps its precision."""
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 50
    return ctx


def cert_context(d, e):
    """(d, e^2, eps ||T||, floor) as 50-digit numbers; ||T|| is the Gershgorin radius tri_solve calls tnorm."""
    mp = _mp()
    n = len(d)
    dm = [mp.mpf(float(x)) for x in d]
    em = [mp.mpf(float(x)) for x in e]
    rad = [abs(dm[k]) + (abs(em[k - 1]) if k > 0 else 0) + (abs(em[k]) if k + 1 < n else 0) for k in range(n)]
    tnorm = max(rad)
    t = max([abs(x) for x in dm] + [abs(x) for x in em])
    s = mp.mpf(2) ** int(mp.floor(mp.log(t, 2))) if t > 0 else mp.mpf(1)
    emax = max([abs(x) for x in em]) if em else mp.mpf(0)
    pivmin = mp.mpf(SAFMIN) * max(mp.mpf(1), (emax / s) ** 2) * s
    floor = 2 * pivmin + mp.mpf(2) ** -1075
    return dm, [x * x for x in em], mp.mpf(EPS) * tnorm, floor


def abs_floor(d, e):
    """The floor of cert_context as a long double."""
    n, ds, es, s = scaled_tridiagonal(d, e)
    emax = float(np.max(np.abs(es))) if n > 1 else 0.0
    ld = np.longdouble
    return 2 * ld(SAFMIN) * ld(max(1.0, emax * emax)) * ld(s) + ld(2) ** -1075


def sturm_count(dm, e2m, x):
    """Eigenvalues of T below x: negative pivots of the L D L^T of T - x (an exact zero pivot is an eigenvalue of the leading
    block sitting on x; it is taken as infinitesimally negative, which is dstebz's convention too)."""
    mp = _mp()
    big = mp.mpf(10) ** 100000
    cnt = 0
    q = dm[0] - x
    for k in range(len(dm)):
        if k:
            q = (dm[k] - x) - (e2m[k - 1] / q if q != 0 else (-big if e2m[k - 1] != 0 else 0))
        if q <= 0:
            cnt += 1
    return cnt


def cert_indices(n):
    return list(range(n)) if n <= 100 else sorted(set(range(0, n, 8)) | {0, n - 1})


def certified(d, e, w, ratio, ctx=None):
    """True when every checked w_i is an eigenvalue i of T to within ratio * eps ||T|| + floor."""
    mp = _mp()
    dm, e2m, unit, floor = ctx or cert_context(d, e)
    if not np.all(np.isfinite(w)) or np.any(np.diff(w) < 0):
        return False
    delta = mp.mpf(ratio) * unit + floor
    for i in cert_indices(len(dm)):
        wi = mp.mpf(float(w[i]))
        if sturm_count(dm, e2m, wi - delta) > i or sturm_count(dm, e2m, wi + delta) < i + 1:
            return False
    return True


def certify(d, e, w):
    """The smallest ratio of CERT_LADDER that certifies w, or inf."""
    ctx = cert_context(d, e)
    start = CERT_LADDER.index(1.0)
    if certified(d, e, w, 1.0, ctx):
        best = 1.0
        for r in reversed(CERT_LADDER[:start]):
            if not certified(d, e, w, r, ctx):
                break
            best = r
        return best
    for r in CERT_LADDER[start + 1:]:
        if certified(d, e, w, r, ctx):
            return r
    return math.inf


# ---- vector checks in long double -------------------------------------------------------------------------------------------
def vector_figures(d, e, w, Z, want_orth=True):
    """Of the claimed eigenpairs (w_i, Z[:, i]) of T: (max_k |(T z - lambda z)_k| / ||T|| over all i, max | ||z|| - 1 |,
    max |Z^T Z - I|) in long double; ||T|| is the Gershgorin radius."""
    ld = np.longdouble
    n = d.shape[0]
    dl, el, wl, Zl = d.astype(ld), e.astype(ld), np.asarray(w).astype(ld), np.asarray(Z).astype(ld)
    R = (dl[:, None] - wl[None, :]) * Zl
    if n > 1:
        R[1:] += el[:, None] * Zl[:-1]
        R[:-1] += el[:, None] * Zl[1:]
    rad = np.abs(dl)
    if n > 1:
        rad[1:] += np.abs(el)
        rad[:-1] += np.abs(el)
    tnorm = rad.max()
    resid = float(np.abs(R).max() / tnorm) if tnorm > 0 else float(np.abs(R).max())
    norms = np.sqrt((Zl * Zl).sum(axis=0))
    orth = float(np.abs(Zl.T @ Zl - np.eye(n, dtype=ld)).max()) if want_orth else None
    return resid, float(np.abs(norms - 1).max()), orth


def angle_to(U, Z):
    """max_i || z_i - u_i (u_i^T z_i) || in long double: the sine of the angle to the known unit vector, without the
    cancellation of sqrt(1 - (u^T z)^2)."""
    ld = np.longdouble
    U, Z = np.asarray(U).astype(ld), np.asarray(Z).astype(ld)
    c = (U * Z).sum(axis=0)
    return float(np.sqrt(((Z - U * c[None, :]) ** 2).sum(axis=0)).max())


def check_result(name, r, bar=CERT_BAR, exact_diagnostics=True):
    """Everything a result (restated or from the device, as a Result) must satisfy for the tabled case `name`; raises
    AssertionError with the figures.  Returns them."""
    _, d, e, verdict = BY_NAME[name]
    n = d.shape[0]
    gap, resid, tnorm = r.diag
    fig = dict(gap=gap, resid=resid)
    assert np.isfinite(r.w).all() and np.isfinite(r.Z).all(), (name, "non-finite output")
    assert certified(d, e, r.w, bar), (name, "eigenvalues not certified within", bar)
    closed = analytic(name)
    tn_ld = np.longdouble(tnorm)
    if closed is not None:
        err = float(np.abs(r.w.astype(np.longdouble) - closed[0]).max() / tn_ld)
        fig["closed_form"] = err / EPS
        assert err <= bar * EPS, (name, "closed form", err / EPS)
    # the diagnostics are true statements about (w, Z)
    scale = r.tnorm_s if r.tnorm_s > 0 else 1.0
    if exact_diagnostics:
        assert gap == (float(np.min(np.diff(r.ws))) / scale if n > 1 else 1.0), (name, "gap is not min diff(w) / tnorm", gap)
    res_ld, norm_err, orth = vector_figures(d / r.s, e / r.s, r.ws, r.Z)
    fig.update(resid_ld=res_ld, norm_err=norm_err, orth=orth)
    assert abs(resid - res_ld) <= 16 * EPS, (name, "resid is not the residual of (w, Z)", resid, res_ld)
    assert r.verdict == verdict, (name, "verdict", r.verdict, r.diag)
    if verdict == "device":
        assert res_ld <= MAX_RESID, (name, "residual", res_ld)
        assert norm_err <= (n + 4) * EPS, (name, "norm", norm_err / EPS)
        assert orth <= max(50 * EPS / gap, 1e3 * EPS), (name, "orthogonality", orth, gap)
        if closed is not None and closed[1] is not None:
            ang = angle_to(closed[1], r.Z)
            fig["angle"] = ang
            assert ang <= 50 * EPS / gap, (name, "angle to the closed form", ang, gap)
    return fig
