"""The seven per-candidate kernels of csrc/popops.hip (rayleigh_dots, relax_normalise, residual, svd_resid, norm_scale, norm,
herm_pick) at lengths around the thread and wave counts, in scattered slots, on both sides of the 1e-10 threshold, with
non-finite entries at the positions where a strided loop or a reduction could lose them, and with tied / NaN scores.

Each check reads back what the device itself produced upstream (pop_get of Y / W), so the vector kernel is judged on its own
inputs and not on the zgemm's rounding.  Element-wise results are compared bit for bit with the per-operation references of
tests/kernel_refs.py, reductions with long-double references inside the bounds derived there."""
import numpy as np
import pytest

import kernel_refs as kr

pytestmark = pytest.mark.gpu

POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3
KIND_EIG, KIND_LINEAR, KIND_SVD = 1, 2, 3
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 1000, 4097, 16385]
BATCHES = [1, 3, 70]


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


class Setup:
    """A context bound to a matrix with `n` rows and `count` candidates in scattered slots of a larger population.

    The matrix only feeds Y = A x, which every check reads back from the device, so it is kept cheap: three entries per row,
    uploaded dense up to n = 4097 and as CSR above (the vector kernels are the same on both paths); `matrix="none"` binds an
    n x 1 zero matrix for the calls that never multiply (relax_normalise takes its length from the row count)."""

    def __init__(self, ctx, n, count, seed, matrix=None):
        import scipy.sparse as sp
        self.ctx, self.n, self.count = ctx, n, count
        self.rng = rng = np.random.default_rng(seed)
        if isinstance(matrix, str):
            self.A = np.zeros((n, 1), dtype=np.complex128)
            ctx.set_matrix(self.A)
        elif matrix is not None:
            self.A = matrix
            ctx.set_matrix(matrix)
        else:
            i = np.arange(n)
            M = sp.csr_matrix((np.concatenate([crand(rng, n), crand(rng, n), np.full(n, 0.5j)]),
                               (np.tile(i, 3), np.concatenate([i, (i * 7 + 3) % n, (i + 1) % n]))), shape=(n, n))
            if n <= 4097:
                self.A = M.toarray()
                ctx.set_matrix(self.A)
            else:
                self.A = M
                ctx.set_matrix_csr(M)
        ctx.pop_reserve(2 * count + 5)
        self.cap = ctx.pop_capacity()
        self.slots = rng.permutation(self.cap)[:count].astype(np.int32)
        self.others = np.setdiff1d(np.arange(self.cap, dtype=np.int32), self.slots)

    def put(self, which, vecs):
        self.ctx.pop_put(which, self.slots, vecs)

    def get(self, which, length=None):
        return self.ctx.pop_get(which, self.slots, self.n if length is None else length)


def cases(lengths=LENGTHS, batches=BATCHES):
    # the 70-candidate batch at the two longest vectors costs a 70 x n x n product for nothing new: 3 candidates there
    return [(n, c) for n in lengths for c in batches if not (n > 1000 and c == 70)] + [(4097, 70)]


# ---- relax_normalise -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count", cases())
def test_relax_elementwise_bit_for_bit(ctx, n, count):
    """normalise = False: X is the per-operation reference bit for bit, for a complex alpha, alpha = 0, alpha = 1 and a
    different alpha per candidate; the returned norm is that X's norm; no other row changes."""
    s = Setup(ctx, n, count, seed=n * 100 + count, matrix="none")
    rng = s.rng
    guard = crand(rng, len(s.others), n)
    ctx.pop_put(POP_X, s.others, guard)
    for alphas in (np.full(count, 0.3 - 0.8j), np.zeros(count, complex), np.ones(count, complex), crand(rng, count)):
        X, W = crand(rng, count, n), crand(rng, count, n)
        s.put(POP_X, X); s.put(POP_W, W)
        nrm = ctx.relax_normalise(s.slots, alphas, normalise=False)
        got = s.get(POP_X)
        for k in range(count):
            ref = kr.relax_ref(X[k], W[k], alphas[k])
            kr.check_bits(got[k], ref, f"relax, candidate {k}, alpha {alphas[k]}")
            kr.check_norm(nrm[k], got[k], f"relax norm, candidate {k}")
        assert np.array_equal(s.get(POP_W), W)
    assert np.array_equal(ctx.pop_get(POP_X, s.others, n), guard)


@pytest.mark.parametrize("n,count", cases())
def test_relax_normalise_two_steps(ctx, n, count):
    """normalise = True: the norm is within (n + 2) u of the long-double norm of the relaxed vector (which the
    normalise = False call returns bit for bit, previous test), and X = fl(v * fl(1 / nrm_dev)) bit for bit."""
    s = Setup(ctx, n, count, seed=n * 100 + count + 1, matrix="none")
    rng = s.rng
    X, W, alphas = crand(rng, count, n), crand(rng, count, n), crand(rng, count)
    s.put(POP_X, X); s.put(POP_W, W)
    nrm = ctx.relax_normalise(s.slots, alphas, normalise=True)
    got = s.get(POP_X)
    worst = 0.0
    for k in range(count):
        v = kr.relax_ref(X[k], W[k], alphas[k])
        worst = max(worst, kr.check_norm(nrm[k], v, f"norm, candidate {k}"))
        kr.check_bits(got[k], kr.scale_ref(v, nrm[k]), f"normalised x, candidate {k}")
    print(f"RATIO relax_norm n={n} count={count} {worst:.3e}")


def _threshold_vectors(n):
    """One non-zero real entry each: zero vector, norm just below 1e-10, exactly 1e-10, just above.  sqrt(fl(x * x)) is |x|
    exactly for these x (checked on the host below), so the branch taken is known."""
    t = np.float64(1e-10)
    vals = [0.0, np.nextafter(t, 0.0), t, np.nextafter(t, 1.0)]
    for x in vals:
        assert np.sqrt(np.float64(x) * np.float64(x)) == x
    V = np.zeros((4, n), dtype=np.complex128)
    for k, x in enumerate(vals):
        V[k, (k * 97) % n] = x
    return V, vals


@pytest.mark.parametrize("n", [1, 64, 257, 4097])
def test_threshold_branches(ctx, n):
    """nrm > 1e-10 decides: relax_normalise leaves X unscaled at 0, below and AT 1e-10 and scales it above; norm_scale
    (svd_power_propose) uses inv = 1 in the first three cases and normalises in the fourth."""
    V, vals = _threshold_vectors(n)
    s = Setup(ctx, n, 4, seed=n, matrix=np.eye(n, dtype=np.complex128))
    s.put(POP_X, V); s.put(POP_W, V)                              # alpha = 1: x <- w = v exactly
    nrm = ctx.relax_normalise(s.slots, np.ones(4, complex), normalise=True)
    got = s.get(POP_X)
    assert list(nrm) == vals
    for k in range(3):
        kr.check_bits(got[k], V[k], f"relax, norm {vals[k]!r}: must stay unscaled")
    kr.check_bits(got[3], kr.scale_ref(V[3], vals[3]), "relax, norm just above 1e-10: scaled")
    assert got[3].real.max() == pytest.approx(1.0, abs=1e-15) and got[3].real.max() != vals[3]
    # norm_scale: A = I, so t = A v = v exactly; u = t * inv, then s = A^H u = u and v' = s * inv2
    s.put(POP_X, V)
    norms = ctx.svd_power_propose(s.slots)
    u, w = s.get(POP_Y), s.get(POP_W)
    assert list(norms[:, 0]) == vals and list(norms[:, 1]) == vals
    for k in range(3):
        kr.check_bits(u[k], V[k], f"norm_scale, norm {vals[k]!r}: inv must be 1")
        assert norms[k, 2] == vals[k] and norms[k, 3] == vals[k]
        kr.check_bits(w[k], V[k], f"norm_scale (second), norm {vals[k]!r}: inv must be 1")
    kr.check_bits(u[3], kr.scale_ref(V[3], vals[3]), "norm_scale, norm just above 1e-10: normalised")
    kr.check_norm(norms[3, 2], u[3])
    kr.check_bits(w[3], kr.scale_ref(u[3], norms[3, 3]), "second norm_scale")


# ---- norm / norm_scale through svd_power_propose ----------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,count", [(n, n, c) for n, c in cases([1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 1000, 4097], [3, 70])
                                              if not (n > 1000 and c == 70)] + [(384, 320, 40), (100, 37, 3), (257, 512, 33), (16385, 1, 3)])
def test_svd_power_propose_norms_and_scaling(ctx, rows, cols, count):
    """norms = (||v||, ||A v||, ||u||, ||A^H u||) and the two scalings, each judged on the device's own input: u (left in Y)
    is t * fl(1 / norms[1]) for SOME t whose norm is norms[1] -- t itself is overwritten in place, so it is recovered from
    a residual call on the same rows, which recomputes Y = A v with the same kernel; v' (left in W) against the product of u,
    which the SVD residual recomputes into W likewise."""
    rng = np.random.default_rng(rows * 31 + cols + count)
    A = crand(rng, rows, cols) / np.sqrt(cols)
    s = Setup(ctx, max(rows, cols), count, seed=rows + count, matrix=A)
    s.n = None
    Vv, Uu = crand(rng, count, cols), crand(rng, count, rows)
    s.put(POP_X, Vv); s.put(POP_U, Uu)
    norms = ctx.svd_power_propose(s.slots)
    u, vnew = s.get(POP_Y, rows), s.get(POP_W, cols)
    # the unscaled products, recomputed by the residual with the same kernels on the same rows (bit-identical: the products of
    # a batch do not depend on what else ran; test_gpu_kernels.py pins that for the batch size as well)
    s.put(POP_U, u)                                               # A^H u of the proposed u
    ctx.residual(KIND_SVD, s.slots, np.ones(count, complex))
    t, sdev = s.get(POP_Y, rows), s.get(POP_W, cols)
    worst = 0.0
    for k in range(count):
        worst = max(worst, kr.check_norm(norms[k, 0], Vv[k], "||v||"), kr.check_norm(norms[k, 1], t[k], "||A v||"))
        kr.check_bits(u[k], kr.scale_ref(t[k], norms[k, 1]), f"u, candidate {k}")
        worst = max(worst, kr.check_norm(norms[k, 2], u[k], "||u||"), kr.check_norm(norms[k, 3], sdev[k], "||A^H u||"))
        kr.check_bits(vnew[k], kr.scale_ref(sdev[k], norms[k, 3]), f"v, candidate {k}")
    print(f"RATIO svd_norms {rows}x{cols} count={count} {worst:.3e}")


# ---- reductions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count", cases())
def test_rayleigh_dots_within_bounds(ctx, n, count):
    s = Setup(ctx, n, count, seed=n * 7 + count)
    X = crand(s.rng, count, n)
    X[0] *= 1e-3 if count > 1 else 1.0
    s.put(POP_X, X)
    num, den = ctx.matvec_rayleigh(s.slots)
    Y = s.get(POP_Y)
    worst = 0.0
    for k in range(count):
        worst = max(worst, kr.check_rayleigh(num[k], den[k], X[k], Y[k]))
    print(f"RATIO rayleigh n={n} count={count} {worst:.3e}")
    # cancelling numerator: y = A x nearly orthogonal to x is the common case near convergence of other candidates; here
    # exactly: x real, A x imaginary (A = i * something real is not at hand, so the bound is simply checked again with
    # alternating signs in x)
    X2 = X * np.where(np.arange(n) % 2, -1.0, 1.0)
    s.put(POP_X, X2)
    num, den = ctx.matvec_rayleigh(s.slots)
    Y2 = s.get(POP_Y)
    for k in range(count):
        kr.check_rayleigh(num[k], den[k], X2[k], Y2[k])


@pytest.mark.parametrize("n,count", cases())
def test_residual_norms(ctx, n, count):
    """EIG, LINEAR and SVD residuals: the difference vector emulated per operation from the device's own Y (and W), its norm
    within (n + 2) u; the SVD residual is the double sum of its two norms."""
    s = Setup(ctx, n, count, seed=n * 11 + count)
    rng = s.rng
    X, Uu = crand(rng, count, n), crand(rng, count, n)
    lam = crand(rng, count)
    b = crand(rng, n)
    s.put(POP_X, X); s.put(POP_U, Uu)
    ctx.set_rhs(b)
    worst = 0.0
    res, fin = ctx.residual(KIND_EIG, s.slots, lam)
    Y = s.get(POP_Y)
    assert fin.all()
    for k in range(count):
        worst = max(worst, kr.check_norm(res[k], kr.eig_diff_ref(X[k], Y[k], lam[k]), f"eig residual {k}"))
    res, fin = ctx.residual(KIND_LINEAR, s.slots, None)
    Y = s.get(POP_Y)
    assert fin.all()
    for k in range(count):
        worst = max(worst, kr.check_norm(res[k], kr.linear_diff_ref(Y[k], b), f"linear residual {k}"))
    sig = (np.abs(rng.standard_normal(count)) + 0.5).astype(np.complex128)
    res, fin = ctx.residual(KIND_SVD, s.slots, sig)
    Y, W = s.get(POP_Y), s.get(POP_W)
    assert fin.all()
    for k in range(count):
        d1, d2 = kr.svd_diff_ref(Y[k], Uu[k], sig[k].real), kr.svd_diff_ref(W[k], X[k], sig[k].real)
        r1, r2 = kr.norm_ref(d1), kr.norm_ref(d2)
        bound = (n + 2) * kr.U * (r1 + r2) + kr.U * (r1 + r2)               # the two norms, and the rounding of their sum
        assert abs(kr.LD(res[k]) - (r1 + r2)) <= bound, (k, res[k], float(r1 + r2))
    print(f"RATIO residual n={n} count={count} {worst:.3e}")


BAD = [np.nan, np.inf, -np.inf]


def _positions(n):
    return sorted({p for p in (0, 255, 256, n - 1) if 0 <= p < n})


@pytest.mark.parametrize("n", [1, 2, 64, 256, 257, 511, 512, 1000, 4097])
def test_finite_flags(ctx, n):
    """The flag is np.isfinite over x (x and u for SVD) and nothing else: a non-finite entry at index 0, 255, 256 or n - 1, in
    the real or the imaginary part, clears the flag of that candidate alone; non-finite entries in Y only (a finite x against
    a matrix with a non-finite entry) leave every flag at 1, as in FakeContext.residual."""
    count = 5
    s = Setup(ctx, n, count, seed=n)
    rng = s.rng
    X, Uu = crand(rng, count, n), crand(rng, count, n)
    ctx.set_rhs(crand(rng, n))
    lam = crand(rng, count)
    sig = np.ones(count, complex)
    for pos in _positions(n):
        for j, bad in enumerate(BAD):
            for part in (1.0, 1j):
                victim = (pos + j) % count
                Xb = X.copy()
                Xb[victim, pos] = complex(bad, X[victim, pos].imag) if part == 1.0 else complex(X[victim, pos].real, bad)
                want = np.isfinite(Xb.real).all(axis=1) & np.isfinite(Xb.imag).all(axis=1)
                assert list(want) == [k != victim for k in range(count)]
                s.put(POP_X, Xb); s.put(POP_U, Uu)
                for kind, l in ((KIND_EIG, lam), (KIND_LINEAR, None), (KIND_SVD, sig)):
                    res, fin = ctx.residual(kind, s.slots, l)
                    assert list(fin) == list(want), (kind, "x", pos, bad, part)
                    assert np.all(np.isfinite(res[want])) and not np.isfinite(res[victim])
                # in u (SVD only): x finite again
                Ub = Uu.copy()
                Ub[victim, pos] = complex(bad, 0.0) if part == 1.0 else complex(0.0, bad)
                s.put(POP_X, X); s.put(POP_U, Ub)
                res, fin = ctx.residual(KIND_SVD, s.slots, sig)
                assert list(fin) == list(want), ("svd", "u", pos, bad, part)
                # both at different candidates
                other = (victim + 2) % count
                Xc = X.copy(); Xc[other, n - 1 - pos] = complex(bad, 1.0)
                s.put(POP_X, Xc)
                res, fin = ctx.residual(KIND_SVD, s.slots, sig)
                assert list(fin) == [k not in (victim, other) for k in range(count)], ("svd", "x and u", pos, bad)
    # Y only: one non-finite matrix entry makes entries of Y non-finite for every finite x; the flags stay 1
    for bad in BAD:
        A = s.A.copy()
        A[n // 2, 0] = bad
        ctx.set_matrix(A)
        ctx.pop_reserve(s.cap)
        s.put(POP_X, X); s.put(POP_U, Uu)
        for kind, l in ((KIND_EIG, lam), (KIND_LINEAR, None), (KIND_SVD, sig)):
            res, fin = ctx.residual(kind, s.slots, l)
            assert not np.all(np.isfinite(s.get(POP_Y).view(np.float64)))
            assert fin.all(), (kind, "Y only", bad)
            assert not np.isfinite(res).any()


# ---- herm_match ------------------------------------------------------------------------------------------------------
def _herm_setup(ctx, n, count, seed):
    rng = np.random.default_rng(seed)
    s = Setup(ctx, n, count, seed=seed, matrix=np.eye(n, dtype=np.complex128))
    V = crand(rng, n, n) / np.sqrt(n)
    return s, rng, V


def _check_match(s, V, idx, nrm, Xin):
    """Index against np.argmax(np.abs(.)) of the device's own scores; norm and written column by the two-step rule."""
    S = s.get(POP_Y)
    got = s.get(POP_X)
    for k in range(s.count):
        kr.check_argmax(idx[k], S[k])
        col = np.ascontiguousarray(V[:, idx[k]])
        if np.all(np.isfinite(col.view(np.float64))):
            kr.check_norm(nrm[k], col, f"column norm, candidate {k}")
        else:
            assert np.isnan(nrm[k])
        kr.check_bits(got[k], kr.scale_ref(col, nrm[k]), f"matched column, candidate {k}")
    return S


@pytest.mark.parametrize("n,count", [(1, 1), (2, 3), (63, 3), (64, 3), (65, 70), (255, 3), (256, 70), (257, 3), (511, 3), (512, 70),
                                     (1000, 70), (1000, 3), (4097, 3), (4096, 40)])
def test_herm_match_planted_and_two_step(ctx, n, count):
    """Distinct planted targets at every length (n not a multiple of 8: 4M scores; a multiple of 8, >= 64 and more than 32
    candidates: DMA scores), the result compared with np.argmax on the device's scores, norm and column by the two-step rule."""
    s, rng, V = _herm_setup(ctx, n, count, seed=n * 3 + count)
    ctx.set_eigvecs(V)
    targets = rng.integers(0, n, size=count)
    X = (V[:, targets].T * (2.0 + rng.random(count))[:, None]) + 1e-3 * crand(rng, count, n)
    s.put(POP_X, X)
    idx, nrm = ctx.herm_match(s.slots)
    _check_match(s, V, idx, nrm, X)
    if n > 8:
        assert list(idx) == list(targets)


@pytest.mark.parametrize("n,count,pairs", [
    (600, 3, [(5, 261), (5, 6), (70, 200), (300, 599)]),         # same thread (j2 = j1 + 256), same wave, other wave, far apart
    (1024, 40, [(0, 256), (63, 64), (255, 1023), (511, 767)]),    # n a multiple of 8, 40 candidates: scores from the DMA kernel
    (257, 3, [(0, 256), (1, 2)]),
])
def test_herm_match_ties_take_the_first_index(ctx, n, count, pairs):
    """Duplicate columns j1 < j2 of V give bit-identical scores; np.argmax takes j1, wherever the two sit: in one thread's
    stride, in one wave, in different waves -- and a different pair in every candidate of the batch."""
    s, rng, V0 = _herm_setup(ctx, n, count, seed=n + count)
    # one V for the batch: every pair duplicated; candidate k aims at pair k (mod the number of pairs)
    V = V0.copy()
    for j1, j2 in pairs:
        V[:, j2] = V[:, j1]
    ctx.set_eigvecs(V)
    aim = [pairs[k % len(pairs)] for k in range(count)]
    X = np.array([3.0 * V[:, j1] for j1, _ in aim]) + 1e-3 * crand(rng, count, n)
    s.put(POP_X, X)
    idx, nrm = ctx.herm_match(s.slots)
    S = _check_match(s, V, idx, nrm, X)
    for k, (j1, j2) in enumerate(aim):
        assert S[k, j1] == S[k, j2], "duplicate columns must score identically"
        assert np.argmax(np.abs(S[k])) == j1
        assert idx[k] == j1, (k, j1, j2, idx[k])


@pytest.mark.parametrize("n,count", [(300, 3), (1024, 40)])
def test_herm_match_nan_scores_rank_first(ctx, n, count):
    """np.argmax returns the index of the first NaN as soon as one score is NaN (AMS:169): one NaN column in V (a NaN score for
    every candidate, at a position behind the best finite score for some and before it for others), two NaN columns (the first
    wins), and a candidate whose own vector holds a NaN (every score NaN: index 0)."""
    s, rng, V0 = _herm_setup(ctx, n, count, seed=n * 5 + count)
    targets = np.array([(17 + 131 * k) % n for k in range(count)])
    for nan_cols in ([n // 2], [n - 1, 258], [0]):
        V = V0.copy()
        for j in nan_cols:
            V[3 % n, j] = complex(np.nan, 0.0)
        ctx.set_eigvecs(V)
        X = 3.0 * V0[:, targets].T + 1e-3 * crand(rng, count, n)
        X[-1, n - 1] = complex(0.0, np.nan)                       # last candidate: an all-NaN row of scores
        s.put(POP_X, X)
        idx, nrm = ctx.herm_match(s.slots)
        S = s.get(POP_Y)
        assert np.isnan(np.abs(S[:, nan_cols])).all() and np.isnan(np.abs(S[-1])).all()
        for k in range(count):
            kr.check_argmax(idx[k], S[k])
        assert list(idx[:-1]) == [min(nan_cols)] * (count - 1) and idx[-1] == 0
        _check_match(s, V, idx, nrm, X)
