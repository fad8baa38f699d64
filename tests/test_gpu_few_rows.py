"""Split-K population products of at most 32 rows (few_rows="splitk", maus_few_rows_set_method(ctx, 1), csrc/zgemm.hip; DESIGN
§3 "Few rows") on the device: the slice and join kernels against exact integer products and the a-priori bound of
tests/kernel_refs.py, rows that do not depend on the batch, confinement of the population products, the workspace, non-finite
rows, every call site, and three loop bodies of MAUS_Solver against the oracle.

Every case first asks the library (few_rows_kernel_for) whether split-K really runs: the rule and its constants live in
csrc/zgemm.hip alone.  `ctx` runs method 1; `ctx0` is a context whose method was never set (the default kernels)."""
import functools
import hashlib

import numpy as np
import pytest

import kernel_refs as kr

pytestmark = pytest.mark.gpu

POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3
# the forms the method covers: dot-product layout with any conjugation, plain layout with a conjugated operand
FORMS = [(1, False, False), (1, True, False), (1, False, True), (1, True, True), (0, True, False), (0, False, True), (0, True, True)]
FORM_IDS = [f"b{bl}{'_ca' if ca else ''}{'_cb' if cb else ''}" for bl, ca, cb in FORMS]


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    c.few_rows_set_method(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx0():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


class forced:
    """`with forced(ctx, S)`: S slices for the products inside, the rule again afterwards."""

    def __init__(self, ctx, S, method=1):
        self.ctx, self.S, self.method = ctx, S, method

    def __enter__(self):
        self.ctx.few_rows_set_method(self.method, self.S)

    def __exit__(self, *exc):
        self.ctx.few_rows_set_method(1, 0)


def split(ctx, M, N, K, bl, ca, cb, want=None):
    """Assert that split-K runs for this product (with `want` slices if given); returns S."""
    kern, S = ctx.few_rows_kernel_for(M, N, K, bl, ca, cb)
    assert kern == 1 and S >= 2, (M, N, K, bl, ca, cb, kern, S)
    assert want is None or S == want, (S, want)
    return S


@functools.lru_cache(maxsize=None)
def _exact(K):
    A, Bm = kr.exact_operands(32, 65, K, 1000 + K)
    return A, Bm, kr.real_products(A, Bm, dtype=np.int64)


def _exact_ref(prods, M, N, ca, cb):
    re, im = kr._combine({k: v[:M, :N] for k, v in prods.items()}, ca, cb)
    return re.astype(np.float64) + 1j * im.astype(np.float64) + 0.0


# ---- exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("S", [2, 3, 7, 32])
def test_exact_product_forced_slices(ctx, S, form):
    """Integer operands: the int64 product bit for bit at K = 16 S + 5 (last slice 21 long) and K = 16 S, every M on both sides
    of the 16-row tile, N inside one column tile, ragged, and in two; alpha = 1, beta = 0 and alpha = -1, beta = 1."""
    bl, ca, cb = form
    with forced(ctx, S):
        for K in (16 * S + 5, 16 * S):
            A, Bm, prods = _exact(K)
            for M in (1, 15, 16, 17, 32):
                for N in (1, 33, 65):
                    split(ctx, M, N, K, bl, ca, cb, want=S)
                    a, B = A[:M], kr.store_b(Bm[:, :N], bl)
                    ref = _exact_ref(prods, M, N, ca, cb)
                    C = ctx.zgemm(a, B, b_layout=bl, conj_a=ca, conj_b=cb)
                    assert np.array_equal(C + 0.0, ref), (M, N, K, np.argwhere(C + 0.0 != ref)[:3])
                    C0 = kr.exact_matrix(np.random.default_rng(K + M), M, N)
                    C = ctx.zgemm(a, B, C_in=C0, b_layout=bl, conj_a=ca, conj_b=cb, alpha=-1.0, beta=1)
                    assert np.array_equal(C + 0.0, C0 - ref + 0.0), (M, N, K, "alpha = -1, beta = 1")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_exact_product_under_the_rule(ctx, form):
    """The same with the rule's own S at N = 64, K = 1029 (the one shape the rule is bound to split)."""
    bl, ca, cb = form
    K = 1029
    A, Bm = kr.exact_operands(32, 64, K, 4242)
    prods = kr.real_products(A, Bm, dtype=np.int64)
    for M in (1, 15, 16, 17, 32):
        split(ctx, M, 64, K, bl, ca, cb)
        C = ctx.zgemm(A[:M], kr.store_b(Bm, bl), b_layout=bl, conj_a=ca, conj_b=cb)
        assert np.array_equal(C + 0.0, _exact_ref(prods, M, 64, ca, cb)), M


# ---- rounded -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rounded(kind, M, N, K):
    A, Bm = (kr.gaussian_operands if kind == "gauss" else kr.cancelling_operands)(M, N, K, 7919 * M + 31 * N + K)
    return A, Bm, kr.real_products(A, Bm)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("M,N,K", [(15, 65, 1029), (32, 33, 4101)])
@pytest.mark.parametrize("kind", ["gauss", "cancel"])
def test_rounded_within_the_derived_bound(ctx, ctx0, kind, M, N, K, form):
    """Inside 2 (K + 8) u S per part, the bound of the default kernels unchanged (it holds for any order of the 2K products,
    so for any slicing; the join adds S - 1 <= 31 roundings where the slices removed K - K / S of them).  Split-K and the default
    agree within twice that bound and, on Gaussian operands, differ somewhere: equal bits at S >= 2 would mean the path was
    not taken."""
    bl, ca, cb = form
    split(ctx, M, N, K, bl, ca, cb)
    assert ctx0.few_rows_kernel_for(M, N, K, bl, ca, cb) == (0, 1)
    A, Bm, prods = _rounded(kind, M, N, K)
    B = kr.store_b(Bm, bl)
    C = ctx.zgemm(A, B, b_layout=bl, conj_a=ca, conj_b=cb)
    D = ctx0.zgemm(A, B, b_layout=bl, conj_a=ca, conj_b=cb)
    r = kr.check_within_bound(C, A, Bm, ca, cb, products=prods)
    r0 = kr.check_within_bound(D, A, Bm, ca, cb, products=prods)
    bound = kr.zgemm_bound(A, Bm, K)
    gap = float(np.max(np.maximum(np.abs(C.real - D.real), np.abs(C.imag - D.imag)) / bound))
    print(f"RATIO few_rows {kind} {M}x{N}x{K} b{bl} ca{int(ca)} cb{int(cb)}: split-K {r:.3e} default {r0:.3e} gap {gap:.3e}")
    assert gap <= 2.0
    if kind == "gauss":
        assert not kr.same_bits(C, D)
    C0 = np.random.default_rng(1).standard_normal((M, N)) * np.sqrt(K) + 0.5j
    C1 = ctx.zgemm(A, B, C_in=C0, b_layout=bl, conj_a=ca, conj_b=cb, alpha=-1.0, beta=1)
    assert kr.check_within_bound(C1, A, Bm, ca, cb, alpha=-1.0, C_in=C0, products=prods) <= 1.0
    assert kr.same_bits(C, ctx.zgemm(A, B, b_layout=bl, conj_a=ca, conj_b=cb))            # two runs, the same bits


# ---- a row does not depend on the batch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [(1, False, False), (0, False, True), (0, True, False)], ids=["b1", "b0_cb", "b0_ca"])
def test_rows_do_not_depend_on_the_batch(ctx, form):
    """The same row alone (16-row tile), as row 0 of 15 and as row 31 of 32 (32-row tile): equal bits."""
    bl, ca, cb = form
    N, K = 65, 1029
    A, Bm = kr.gaussian_operands(32, N, K, 99)
    B = kr.store_b(Bm, bl)
    row = A[5:6]
    for M in (1, 15, 32):
        split(ctx, M, N, K, bl, ca, cb)
    alone = ctx.zgemm(row, B, b_layout=bl, conj_a=ca, conj_b=cb)
    A15 = np.vstack([row, A[10:24]])
    A32 = np.vstack([A[:5], A[6:], row])
    assert A15.shape[0] == 15 and A32.shape[0] == 32
    assert kr.same_bits(ctx.zgemm(A15, B, b_layout=bl, conj_a=ca, conj_b=cb)[0:1], alone)
    assert kr.same_bits(ctx.zgemm(A32, B, b_layout=bl, conj_a=ca, conj_b=cb)[31:32], alone)


def test_population_rows_do_not_depend_on_batch_or_gather_order(ctx):
    """Y = A X through the slot lists: a candidate's row alone, among 15, among 32, and in two gather orders."""
    n = 1029
    rng = np.random.default_rng(31)
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    ctx.set_matrix(A)
    ctx.pop_reserve(48)
    X = rng.standard_normal((48, n)) + 1j * rng.standard_normal((48, n))
    ctx.pop_put(POP_X, np.arange(48), X)
    for M in (1, 15, 32):
        split(ctx, M, n, n, 1, False, False)
    ctx.matvec_rayleigh([7])
    alone = ctx.pop_get(POP_Y, [7], n)
    order = [int(s) for s in rng.permutation(48)[:32] if s != 7][:14]
    for slots in ([7] + order, order + [7], order[::-1] + [7] + list(range(30, 47))):
        assert len(slots) in (15, 32)
        ctx.pop_put(POP_Y, [7], np.zeros((1, n)))                  # (writing Y drops the "Y = A X" stamps)
        ctx.matvec_rayleigh(slots)
        assert kr.same_bits(ctx.pop_get(POP_Y, [7], n), alone), slots


# ---- confinement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,count", [(1029, 1029, 15), (1029, 1029, 32), (1040, 1100, 17)])
def test_population_products_exact_and_confined(ctx, rows, cols, count):
    """The pattern of test_gpu_zgemm_variants.test_population_products_exact_and_confined under split-K: scattered slots,
    ldp > the row, capacity > batch; exact products in the listed rows, sentinels in every other row and in the columns >= N
    of the listed ones."""
    from adaptive_matrix_solver_amd._cabi import KIND_EIG, KIND_SVD
    from test_gpu_zgemm_variants import SENT, PopImage
    rng = np.random.default_rng(rows * 10007 + cols * 13 + count)
    square = rows == cols
    A = kr.exact_matrix(rng, rows, cols)
    ctx.set_matrix(A)
    ctx.pop_reserve(count + 20)
    cap, ldp = ctx.pop_capacity(), max(rows, cols)
    assert cap > count
    split(ctx, count, rows, cols, 1, False, False)               # A X
    split(ctx, count, cols, rows, 0, False, True)                # A^H u
    slots = rng.permutation(cap)[:count].astype(np.int32)
    pop = PopImage(ctx, cap, ldp)

    def filled(length=0):
        full = np.full((cap, ldp), SENT)
        if length:
            full[:, :length] = kr.exact_matrix(rng, cap, length)
        return full

    pop.put(POP_X, filled(cols))
    pop.put(POP_U, filled(rows))
    pop.put(POP_W, filled())
    X, Uu = pop.img[POP_X][slots, :cols], pop.img[POP_U][slots, :rows]
    AX, AHU = X @ A.T, Uu @ A.conj()

    def others_unchanged(*except_):
        for w in (POP_X, POP_U, POP_W, POP_Y):
            if w not in except_:
                pop.unchanged(w)

    if square:
        pop.put(POP_Y, filled())
        num, den = ctx.matvec_rayleigh(slots)
        pop.expect(POP_Y, slots, rows, AX)
        others_unchanged(POP_Y)
        assert np.array_equal(num, np.einsum("ki,ki->k", X.conj(), AX)) and np.array_equal(den, np.einsum("ki,ki->k", X.conj(), X))
        pop.put(POP_Y, filled())
        ctx.residual(KIND_EIG, slots, np.full(count, 2.0 - 1.0j))
        pop.expect(POP_Y, slots, rows, AX)
        others_unchanged(POP_Y)
    pop.put(POP_Y, filled())
    pop.put(POP_U, pop.img[POP_U])
    res, fin = ctx.residual(KIND_SVD, slots, np.full(count, 3.0 + 0j))
    pop.expect(POP_Y, slots, rows, AX)
    pop.expect(POP_W, slots, cols, AHU)
    others_unchanged(POP_Y, POP_W)
    assert fin.all()
    pop.put(POP_Y, filled())
    pop.put(POP_W, filled())
    ctx.svd_power_propose(slots)
    pop.expect(POP_Y, slots, rows, None)
    pop.expect(POP_W, slots, cols, None)
    others_unchanged(POP_Y, POP_W)
    if square:
        split(ctx, count, rows, rows, 0, True, False)            # conj(X) V
        V = kr.exact_matrix(rng, rows, rows)
        ctx.set_eigvecs(V)
        pop.put(POP_Y, filled())
        ctx.herm_match(slots)
        pop.expect(POP_Y, slots, rows, X.conj() @ V)
        pop.expect(POP_X, slots, rows, None)
        others_unchanged(POP_X, POP_Y)


# ---- workspace -----------------------------------------------------------------------------------------------------------
def test_workspace_is_sized_by_the_call_and_never_read_stale():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    try:
        c.few_rows_set_method(1)
        assert c.few_rows_workspace_allocs() == 0
        A, B = kr.exact_operands(32, 2048, 2048, 5, b_layout=1)       # parts up to 2^10: partial sums of ~2^30 in every slab
        split(c, 32, 2048, 2048, 1, False, False)
        ref = kr.exact_reference(A, B, b_layout=1) + 0.0
        assert np.array_equal(c.zgemm(A, B, b_layout=1) + 0.0, ref)
        first = c.few_rows_workspace_allocs()
        assert first >= 1
        assert np.array_equal(c.zgemm(A, B, b_layout=1) + 0.0, ref)
        assert c.few_rows_workspace_allocs() == first                  # the same shape again: no allocation
        with forced(c, 3):
            split(c, 3, 33, 53, 1, False, False, want=3)
            a, b = kr.exact_operands(3, 33, 53, 6, b_layout=1)
            assert kr.check_exact(c.zgemm(a, b, b_layout=1), a, b, b_layout=1) == 0.0
        rng = np.random.default_rng(8)
        for rows, cols in ((1100, 1040), (1029, 1029)):                # another matrix shape, another ldp
            M = kr.exact_matrix(rng, rows, cols)
            c.set_matrix(M)
            c.pop_reserve(40)
            X = kr.exact_matrix(rng, 17, cols)
            slots = np.arange(3, 20)
            c.pop_put(POP_X, slots, X)
            c.pop_put(POP_U, slots, kr.exact_matrix(rng, 17, rows))
            split(c, 17, rows, cols, 1, False, False)
            c.residual(3, slots, np.full(17, 1.0 + 0j))
            assert np.array_equal(c.pop_get(POP_Y, slots, rows), X @ M.T)
        assert c.few_rows_workspace_allocs() == first                  # all of them fit the first one
    finally:
        c.close()


# ---- non-finite ----------------------------------------------------------------------------------------------------------
def test_nan_in_one_gathered_row_stays_in_that_row(ctx):
    n, count = 1029, 15
    rng = np.random.default_rng(77)
    A = kr.exact_matrix(rng, n, n)
    ctx.set_matrix(A)
    ctx.pop_reserve(40)
    slots = rng.permutation(40)[:count].astype(np.int32)
    X = kr.exact_matrix(rng, count, n)
    X[4, 517] = complex(np.nan, 1.0)
    ctx.pop_put(POP_X, slots, X)
    split(ctx, count, n, n, 1, False, False)
    ctx.residual(1, slots, np.full(count, 1.0 + 0j))
    Y = ctx.pop_get(POP_Y, slots, n)
    ok = np.arange(count) != 4
    assert not np.isfinite(Y[4].view(np.float64)).any()
    assert np.array_equal(Y[ok], X[ok] @ A.T)


# ---- call sites ----------------------------------------------------------------------------------------------------------
def test_herm_match_scores_and_arg_max(ctx, ctx0):
    n, count = 1024, 15
    rng = np.random.default_rng(12)
    V, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    X = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    X += 40.0 * V[:, rng.permutation(n)[:count]].T                 # one clearly best column per candidate
    scores = X.conj() @ V
    top = np.sort(np.abs(scores), axis=1)
    assert np.all(top[:, -1] - top[:, -2] >= 1e-6)
    slots = rng.permutation(30)[:count].astype(np.int32)
    got = {}
    for name, c, method in (("split", ctx, 1), ("zero", ctx, 0), ("unset", ctx0, None)):
        c.set_matrix(np.eye(n, dtype=np.complex128))
        c.pop_reserve(30)
        c.set_eigvecs(V)
        c.pop_put(POP_X, slots, X)
        if method is not None:
            c.few_rows_set_method(method)
        try:
            assert c.few_rows_kernel_for(count, n, n, 0, True, False)[0] == (1 if method == 1 else 0)
            idx, nrm = c.herm_match(slots)
        finally:
            if method is not None:
                c.few_rows_set_method(1)
        got[name] = (idx, nrm, c.pop_get(POP_Y, slots, n))
    idx, _, Y = got["split"]
    assert np.array_equal(idx, np.argmax(np.abs(scores), axis=1))
    kr.check_within_bound(Y, X, V, conj_a=True)
    assert np.array_equal(got["zero"][0], got["unset"][0])          # method 0 is the default kernels, bit for bit
    assert kr.same_bits(got["zero"][1], got["unset"][1]) and kr.same_bits(got["zero"][2], got["unset"][2])
    assert not kr.same_bits(got["zero"][2], Y)


@pytest.mark.parametrize("count", [15, 32])
def test_gram_block(ctx, ctx0, count):
    n = 4101
    rng = np.random.default_rng(count)
    X = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    slots = rng.permutation(count + 9)[:count].astype(np.int32)
    out = {}
    for name, c, method in (("split", ctx, 1), ("zero", ctx, 0), ("unset", ctx0, None)):
        c.set_matrix(np.zeros((8, n), dtype=np.complex128))          # (a population row holds max(rows, cols) entries)
        c.pop_reserve(count + 9)
        c.pop_put(POP_X, slots, X)
        if method is not None:
            c.few_rows_set_method(method)
        try:
            assert c.few_rows_kernel_for(count, count, n, 1, True, False)[0] == (1 if method == 1 else 0)
            out[name] = c.gram(POP_X, slots, n)
        finally:
            if method is not None:
                c.few_rows_set_method(1)
    G = out["split"]
    kr.check_within_bound(G, X, X, conj_a=True, b_layout=1)
    bound = kr.zgemm_bound(X, X, n, b_layout=1)
    assert np.all(np.abs((G - G.conj().T).real) <= 2 * bound) and np.all(np.abs((G - G.conj().T).imag) <= 2 * bound)
    assert kr.same_bits(out["zero"], out["unset"]) and not kr.same_bits(out["zero"], G)


def test_svd_power_propose(ctx, ctx0):
    rows, cols, count = 1024, 768, 15
    rng = np.random.default_rng(3)
    A = (rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols))) / np.sqrt(cols)
    Xv = rng.standard_normal((count, cols)) + 1j * rng.standard_normal((count, cols))
    slots = rng.permutation(25)[:count].astype(np.int32)
    out = {}
    for name, c, method in (("split", ctx, 1), ("zero", ctx, 0), ("unset", ctx0, None)):
        c.set_matrix(A)
        c.pop_reserve(25)
        c.pop_put(POP_X, slots, Xv)
        if method is not None:
            c.few_rows_set_method(method)
        try:
            want = 1 if method == 1 else 0
            assert c.few_rows_kernel_for(count, rows, cols, 1, False, False)[0] == want
            assert c.few_rows_kernel_for(count, cols, rows, 0, False, True)[0] == want
            norms = c.svd_power_propose(slots)
        finally:
            if method is not None:
                c.few_rows_set_method(1)
        out[name] = (norms, c.pop_get(POP_Y, slots, rows), c.pop_get(POP_W, slots, cols))
    for a, b in zip(out["zero"], out["unset"]):
        assert kr.same_bits(a, b)
    norms, Yu, Wv = out["split"]
    LD, U = kr.LD, kr.U

    def judge(prod_ref, bound, sigma, scaled, length):
        """sigma = ||product|| and scaled = product / sigma against the long-double product: the product's a-priori bound per
        part, (length + 2) u on the norm, 4 u on the scaling."""
        re, im = prod_ref
        nref = np.sqrt(np.sum(re * re + im * im, axis=1)).astype(np.float64)
        dn = np.sqrt(2.0) * np.linalg.norm(bound, axis=1) + (length + 2) * U * nref
        assert np.all(np.abs(sigma - nref) <= dn), np.max(np.abs(sigma - nref) / dn)
        tol = (bound + (np.abs(re) + np.abs(im)).astype(np.float64) * (dn / nref + 4 * U)[:, None]) / nref[:, None]
        err = np.maximum(np.abs(scaled.real - (re / nref[:, None])), np.abs(scaled.imag - (im / nref[:, None]))).astype(np.float64)
        assert np.all(err <= tol), float(np.max(err / tol))

    judge(kr.zgemm_reference(Xv, A, b_layout=1), kr.zgemm_bound(Xv, A, cols, b_layout=1), norms[:, 1], Yu, rows)
    judge(kr.zgemm_reference(Yu, A, conj_b=True), kr.zgemm_bound(Yu, A, rows), norms[:, 3], Wv, cols)
    assert not kr.same_bits(out["zero"][1], Yu)


# ---- solver level ----------------------------------------------------------------------------------------------------------
FEW_SCENARIOS = {
    # Hermitian eigenproblem, 15 candidates: shortcut (conj(X) V), residual (A X), Gram block
    "few_herm768": dict(kind="eig", build=("hermitian", 768, 768), P=15, iters=3, seed=5, tol=1e-8),
    # general eigenproblem, 16 candidates on the direct path: Rayleigh quotient and residual (A X)
    "few_eig768": dict(kind="eig", build=("ginibre", 768, 768, 1.0), P=16, iters=3, seed=1234, tol=1e-8),
}
RUN_KW = {"few_herm768": dict(gram_min=2), "few_eig768": dict(pert_mode="uniform")}
CMP_KW = {"few_herm768": dict(tie_tol=1e-13), "few_eig768": {}}


@pytest.fixture(scope="module")
def scenarios_few():
    import scenarios
    scenarios.TRAJECTORIES.update(FEW_SCENARIOS)
    yield
    for k in FEW_SCENARIOS:
        scenarios.TRAJECTORIES.pop(k, None)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    import rounding
    ref, anorm = rounding.oracle_run(name, 3)
    pert, _ = rounding.oracle_run(name, 3, perturb_seed=1, ulps=1)
    return ref, anorm, pert


def _digest(run):
    h = hashlib.sha256()
    for it in run:
        for r in it["rows"]:
            h.update(repr((r["id"], r["state"], r["stuck"], r["retries"], r["resets"])).encode())
            h.update(np.float64(r["resid"]).tobytes() + np.complex128(r["lam"]).tobytes() + np.float64(r["w"]).tobytes())
            for v in r["vecs"]:
                h.update(np.ascontiguousarray(v, dtype=np.complex128).tobytes())
        h.update(repr((it["after"], it["rng"], it["n_distinct"], it["energy"])).encode())
    return h.hexdigest()


@pytest.mark.parametrize("name", list(FEW_SCENARIOS))
def test_solver_three_loop_bodies_against_the_oracle(scenarios_few, monkeypatch, name):
    """Three loop bodies under few_rows="splitk" against the oracle with test_gpu_step_parity's tolerances, bookkeeping and both
    RNG streams exact; then the same bodies under "auto" and with no keyword at all: equal digests (every solver has a context
    of its own, so the method of those was never set).  n = 768 so that K reaches the rule's shortest slices; most of the
    ~14 s per scenario is the CPU oracle, run twice (as it is, and with its solves perturbed by one ulp)."""
    import rounding
    import test_gpu_step_parity as sp
    monkeypatch.delenv("MAUS_FEW_ROWS", raising=False)
    ref, anorm, pert = _oracle(name)
    # a rounding-sized perturbation of the oracle's own solves leaves every integer decision of these scenarios where it is:
    # a difference in the device's bookkeeping below is a bug, not rounding
    for d, same, order, rng_same in rounding.drift(ref, pert):
        assert same and rng_same, name
        assert order, name
    got = sp.product_run(name, 3, few_rows="splitk", **RUN_KW[name])
    sp.compare(ref, got, anorm, name, **CMP_KW[name])
    for r, g in zip(ref, got):                                       # bookkeeping tuples and both RNG stream positions: exact
        assert sorted((x["id"], x["state"], x["stuck"], x["retries"], x["resets"]) for x in r["rows"]) == \
               sorted((x["id"], x["state"], x["stuck"], x["retries"], x["resets"]) for x in g["rows"])
        assert r["rng"] == g["rng"]
    # 'auto' never sets the method: the bits of a run in which nobody named the keyword, before and after a split-K run
    unset = _digest(sp.product_run(name, 3, **RUN_KW[name]))
    auto = _digest(sp.product_run(name, 3, few_rows="auto", **RUN_KW[name]))
    assert auto == unset
    assert _digest(got) != unset                                     # ... and split-K really ran in the solver


def test_solver_sets_the_method_and_the_products_split(scenarios_few):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    import scenarios
    A, _ = scenarios.build(FEW_SCENARIOS["few_herm768"])
    s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=15, quiet=True, few_rows="splitk")
    c = s.engine.ctx
    assert s.engine.few_rows == "splitk" and c.few_rows_method() == 1
    for M in (1, 15, 16):
        split(c, M, 768, 768, 1, False, False)
        split(c, M, 768, 768, 0, True, False)
        split(c, M, M, 768, 1, True, False) if M > 1 else None
    s2 = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=15, quiet=True)
    assert s2.engine.few_rows == "auto" and s2.engine.ctx.few_rows_method() == 0
