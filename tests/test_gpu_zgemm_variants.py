"""Every zgemm kernel that Context.zgemm can reach, against exact integer references and derived bounds; and the population
products (row gather / scatter, leading dimension larger than the row) against exact products and sentinels.

`variant()` (tests/zgemm_cases.py) is the Python statement of the dispatch rule of maus_zgemm_launch_rows (csrc/zgemm.hip);
tests/test_zgemm_plan_host.py holds the library's rule against it at every threshold.  The table CASES names, for every case,
the kernel instantiation the launcher picks, and test_table_covers_every_variant asserts that all of them are there.  That
the cases really reach the kernels they name was confirmed on an MI355X by running this file under
`rocprofv3 --kernel-trace --stats` and comparing the traced instantiations with `expected_kernel_names()` (test
tiers; profiles/zgemm_dispatch_refactor_rates.txt).  References and bounds: tests/kernel_refs.py."""
import functools

import numpy as np
import pytest

import kernel_refs as kr
from zgemm_cases import CASES, CONJ, all_variants, variant

pytestmark = pytest.mark.gpu


def _id(case):
    M, N, K, bl, ca, cb = case
    return f"{M}x{N}x{K}-{variant(*case)[0]}"


def expected_kernel_names():
    """The instantiations this file launches through Context.zgemm (for the comparison with a kernel trace)."""
    return sorted({variant(*c)[1] for c in CASES})


def is_3m(case):
    return not variant(*case)[0].startswith("4m_")


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


def test_table_covers_every_variant():
    names = all_variants()
    # 6 plain-layout kernels + the DMA-staged 3M kernel in 5 layout / conjugation forms x 2 tile shapes + the 4M kernel in 7
    # forms (plain layout without conjugation never reaches it) x 3 tile shapes
    assert len(names) == 6 + 10 + 21
    covered = {variant(*c)[0] for c in CASES}
    assert covered == set(names), sorted(set(names) - covered)
    assert len(set(names.values())) == len(names)


def judged_rows(M):
    """Rows of a Gaussian product that are compared with the long-double reference.  np.longdouble matmuls run at ~0.05
    GFLOP/s, so products with more than 200 rows are judged on 96 of them: the first and the last 32 (both edges of the tile
    grid) and 32 spread over the middle.  The device computes the whole product either way, and the exact-integer cases judge
    every element."""
    if M <= 200:
        return np.arange(M)
    return np.unique(np.concatenate([np.arange(32), np.linspace(32, M - 33, 32).astype(int), np.arange(M - 32, M)]))


@functools.lru_cache(maxsize=2)
def _operands(kind, M, N, K):
    """(A, Bm [K][N], real products, judged rows) shared by the two layouts and four conjugation forms of a shape."""
    seed = 7919 * M + 31 * N + K
    if kind == "exact":
        A, Bm = kr.exact_operands(M, N, K, seed)
        return A, Bm, kr.real_products(A, Bm, dtype=np.int64), np.arange(M)
    A, Bm = (kr.gaussian_operands if kind == "gauss" else kr.cancelling_operands)(M, N, K, seed)
    rows = judged_rows(M)
    return A, Bm, kr.real_products(A[rows], Bm), rows


def _exact_ref(prods, ca, cb):
    re, im = kr._combine(prods, ca, cb)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_exact_product(ctx, case):
    """Integer operands, alpha = 1, beta = 0: the int64 product bit for bit; then alpha = -1, beta = 1 on an integer C_in."""
    M, N, K, bl, ca, cb = case
    A, Bm, prods, _ = _operands("exact", M, N, K)
    B = kr.store_b(Bm, bl)
    ref = _exact_ref(prods, ca, cb)
    C = ctx.zgemm(A, B, b_layout=bl, conj_a=ca, conj_b=cb)
    assert C.shape == ref.shape
    bad = np.argwhere(C != ref)
    assert len(bad) == 0, f"{len(bad)} of {C.size} entries differ, first at {tuple(bad[0])}: {C[tuple(bad[0])]} != {ref[tuple(bad[0])]}"
    C0 = kr.exact_matrix(np.random.default_rng(K), M, N)
    C = ctx.zgemm(A, B, C_in=C0, b_layout=bl, conj_a=ca, conj_b=cb, alpha=-1.0, beta=1)
    bad = np.argwhere(C != C0 - ref)
    assert len(bad) == 0, f"alpha = -1, beta = 1: {len(bad)} of {C.size} entries differ, first at {tuple(bad[0])}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gaussian_within_derived_bound(ctx, case):
    """Gaussian operands against the long-double reference: inside 2 (K + 8) u S per part, and for K <= 512 inside the
    statistical form the existing tests assert.  beta = 1 through the same kernel as well."""
    M, N, K, bl, ca, cb = case
    A, Bm, prods, rows = _operands("gauss", M, N, K)
    B = kr.store_b(Bm, bl)
    C = ctx.zgemm(A, B, b_layout=bl, conj_a=ca, conj_b=cb)
    assert C.shape == (M, N) and np.all(np.isfinite(C.view(np.float64)))
    Ar = A[rows]                                                # (the checkers take B as the [K][N] matrix: b_layout 0)
    try:
        ratio = kr.check_within_bound(C[rows], Ar, Bm, ca, cb, products=prods)
        stat = kr.check_statistical(C[rows], Ar, Bm, ca, cb, products=prods) if K <= 512 else float("nan")
    finally:
        re, im = kr.zgemm_reference(Ar, Bm, ca, cb, products=prods)
        e = np.maximum(np.abs(C[rows].real - re), np.abs(C[rows].imag - im)).astype(np.float64)
        h = np.hypot((C[rows].real - re).astype(np.float64), (C[rows].imag - im).astype(np.float64))
        print(f"RATIO {variant(*case)[0]} {M}x{N}x{K} derived {np.max(e / kr.zgemm_bound(Ar, Bm, K)):.3e} "
              f"statistical {np.max(h / (np.abs(Ar) @ np.abs(Bm))) / (4e-16 * max(4.0, np.sqrt(K))):.3e}")
    assert ratio <= 1.0 and not stat >= 1.0
    C0 = np.random.default_rng(1).standard_normal((M, N)) * np.sqrt(K) + 0.5j
    C1 = ctx.zgemm(A, B, C_in=C0, b_layout=bl, conj_a=ca, conj_b=cb, alpha=-1.0, beta=1)
    assert kr.check_within_bound(C1[rows], Ar, Bm, ca, cb, alpha=-1.0, C_in=C0[rows], products=prods) <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if is_3m(c)], ids=_id)
def test_cancelling_operands_3m(ctx, case):
    """Ar = -Ai, Br = -Bi up to 1e-9: the operand sums of the third product cancel to nine digits.  Still inside the bound
    (the imaginary part of a 3M product has a normwise bound, which is what 2 (K + 8) u S is)."""
    M, N, K, bl, ca, cb = case
    A, Bm, prods, rows = _operands("cancel", M, N, K)
    C = ctx.zgemm(A, kr.store_b(Bm, bl), b_layout=bl, conj_a=ca, conj_b=cb)
    assert np.all(np.isfinite(C.view(np.float64)))
    r = kr.check_within_bound(C[rows], A[rows], Bm, ca, cb, products=prods)
    print(f"RATIO-CANCEL {variant(*case)[0]} {M}x{N}x{K} derived {r:.3e}")


@pytest.mark.parametrize("n", [64, 1536])
def test_identity_products_bit_for_bit(ctx, n):
    """The asymmetric operand check of the lane maps, on the DMA-staged kernels (K = n >= 64, M > 32) in every form that
    reaches them: I @ B == B, B @ I == B, and the same through conjugated operands (conj(I) = I, conj(conj(B)) = B)."""
    I = np.eye(n, dtype=np.complex128)
    k = np.arange(n * n).reshape(n, n)
    Bq = (k % 97 - 40 + 1j * (k % 89 - 50)).astype(np.complex128)
    for bl in (0, 1):
        st = lambda X: kr.store_b(X, bl)
        for ca, cb in CONJ:
            name = variant(n, n, n, bl, ca, cb)[0]
            want_right = Bq.conj() if cb else Bq                 # op(I) @ op(B)
            assert np.array_equal(ctx.zgemm(I, st(Bq), b_layout=bl, conj_a=ca, conj_b=cb), want_right), (name, "I @ B")
            want_left = Bq.conj() if ca else Bq                  # op(B) @ op(I)
            assert np.array_equal(ctx.zgemm(Bq, st(I), b_layout=bl, conj_a=ca, conj_b=cb), want_left), (name, "B @ I")
    assert variant(n, n, n, 0, True, False)[0].startswith("dma3m") and variant(n, n, n, 1, False, True)[0].startswith("dma3m")


# ---------------------------------------------------------------------------------------------------------------------
# population products: a_rows / c_rows, ldp = max(rows, cols) > row length, capacity > batch
# ---------------------------------------------------------------------------------------------------------------------
POP_X, POP_U, POP_W, POP_Y = 0, 1, 2, 3
SENT = complex(-7777.25, 3333.5)
POP_SHAPES = [(64, 64), (100, 100), (1000, 1000), (1536, 1536), (384, 320), (320, 384), (100, 37)]
COUNTS = [1, 32, 33, 40, 1600]


class PopImage:
    """Host image of the four population arrays, whole rows (length ldp): what the device must hold."""

    def __init__(self, ctx, cap, ldp):
        self.ctx, self.cap, self.ldp = ctx, cap, ldp
        self.all = np.arange(cap, dtype=np.int32)
        self.img = {}

    def put(self, which, full):
        assert full.shape == (self.cap, self.ldp)
        self.ctx.pop_put(which, self.all, full)
        self.img[which] = full.copy()

    def expect(self, which, slots, length, values):
        """The call must have left `values` (None: anything finite or not -- the values are judged elsewhere) in the first
        `length` entries of the rows `slots` of array `which`."""
        got = self.ctx.pop_get(which, self.all, self.ldp)
        if values is not None:
            bad = np.argwhere(got[slots, :length] != values)
            assert len(bad) == 0, (f"array {which}: {len(bad)} of {values.size} entries of the selected rows differ from the exact "
                                   f"product, first at row {slots[bad[0][0]]}, column {bad[0][1]}")
        self.img[which][slots, :length] = got[slots, :length]
        self.unchanged(which, got)

    def unchanged(self, which, got=None):
        got = self.ctx.pop_get(which, self.all, self.ldp) if got is None else got
        bad = np.argwhere(~kr_same(got, self.img[which]))
        assert len(bad) == 0, f"array {which}: stray write at row {bad[0][0]}, column {bad[0][1]} ({len(bad)} entries changed)"


def kr_same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("rows,cols", POP_SHAPES)
def test_population_products_exact_and_confined(ctx, rows, cols, count):
    """Exact products in the selected rows, sentinels everywhere else (see the module docstring).  The module's one context is
    re-bound from shape to shape on purpose, as a solver process does from problem to problem: everything sized by the vector
    length has to follow (the A^H u scratch of the SVD step once did not)."""
    from adaptive_matrix_solver_amd._cabi import KIND_EIG, KIND_LINEAR, KIND_SVD
    rng = np.random.default_rng(rows * 10007 + cols * 13 + count)
    square = rows == cols
    A = kr.exact_matrix(rng, rows, cols)
    ctx.set_matrix(A)
    ctx.pop_reserve(count + 60 if count < 1000 else 1700)
    cap, ldp = ctx.pop_capacity(), max(rows, cols)
    assert cap > count
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
    AX = X @ A.T                                             # integers: exact in any order
    AHU = Uu @ A.conj()

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

        pop.put(POP_Y, filled())                             # (writing Y drops the library's "Y = A X" stamps)
        ctx.residual(KIND_EIG, slots, np.full(count, 2.0 - 1.0j))
        pop.expect(POP_Y, slots, rows, AX)
        others_unchanged(POP_Y)

        ctx.set_rhs(kr.exact_matrix(rng, rows))
        pop.put(POP_Y, filled())
        ctx.residual(KIND_LINEAR, slots, None)
        pop.expect(POP_Y, slots, rows, AX)
        others_unchanged(POP_Y)

    pop.put(POP_Y, filled())
    pop.put(POP_U, pop.img[POP_U])                           # (writing U drops the "S = A^H U" stamps: no kept product)
    res, fin = ctx.residual(KIND_SVD, slots, np.full(count, 3.0 + 0j))
    pop.expect(POP_Y, slots, rows, AX)                       # Y = A v
    pop.expect(POP_W, slots, cols, AHU)                      # W = A^H u  (plain layout, conj_b)
    others_unchanged(POP_Y, POP_W)
    assert fin.all()

    pop.put(POP_Y, filled())
    pop.put(POP_W, filled())
    ctx.svd_power_propose(slots)
    pop.expect(POP_Y, slots, rows, None)                     # u and v are scaled in place: values in test_gpu_vector_kernels.py
    pop.expect(POP_W, slots, cols, None)
    others_unchanged(POP_Y, POP_W)

    if square:
        V = kr.exact_matrix(rng, rows, rows)
        ctx.set_eigvecs(V)
        pop.put(POP_Y, filled())
        ctx.herm_match(slots)
        pop.expect(POP_Y, slots, rows, X.conj() @ V)         # scores conj(x) V  (plain layout, conj_a)
        pop.expect(POP_X, slots, rows, None)                 # the matched column replaces x
        others_unchanged(POP_X, POP_Y)
