"""The lane-per-row SpMM on the CSR arrays (maus_spmm_set_method(ctx, 0), the default) and on the sliced-ELL copy
(maus_spmm_set_method(ctx, 1), sparse_spmm="sell") side by side in one process on the same matrix -> profiles/spmm_sell_rates.txt.

    python tools/spmm_rates.py [--out profiles/spmm_sell_rates.txt] [--quick] [--lib another/libmaus_hip.so]

Two contexts hold the same matrix and the same population rows, one per method.  One sample is REPS products Y = A X of P rows
through maus_residual (linear kind: the product is always recomputed there), timed by the library's HIP events around every
launch of the "spmm" class, as time per launch; the two methods alternate sample by sample and the figure is the median of 5
samples after a warm-up of each.  A^H is timed by binding scipy's CSR of A^H, which is the operand the library builds for it.

Algorithmic bytes, the same for both methods: X read + Y written (16 B per complex element each) + the operand (16 B value +
4 B index per nonzero, 4 B per row pointer) once per group of 8 candidates; the sliced-ELL copy also streams its padding
(fill = padded slots / nnz), which this count leaves out, so the share of the copy rate is that of the useful bytes.  The
reference copy rate is 6.29 TB/s.  The bar for an opt-in method is 1.25x over the default in the same process.
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adaptive_matrix_solver_amd import Context, _cabi  # noqa: E402

COPY_TBS = 6.29
BAR = 1.25
SAMPLES = 5
KERNEL = {0: "none", 1: "rows", 2: "wave", 3: "sell"}


def banded(n, per_row, seed=0):
    """per_row nonzeros per row: the diagonal and its nearest off-diagonals (tools/sparse_rates.py's operator)"""
    rng = np.random.default_rng(seed)
    offs = [o for o in range(-(per_row // 2), per_row // 2 + 1)][:per_row]
    diags = [rng.standard_normal(n - abs(o)) + 1j * rng.standard_normal(n - abs(o)) for o in offs]
    return sp.csr_matrix(sp.diags(diags, offs, shape=(n, n)) + sp.identity(n) * 2.0 * per_row)


def random_pattern(n, per_row, seed=1):
    """per_row random columns per row plus the diagonal (the pattern of tests/test_gpu_sparse.py): A^H has ragged rows"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, n * per_row)
    vals = rng.standard_normal(n * per_row) + 1j * rng.standard_normal(n * per_row)
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sum_duplicates()
    return A + sp.identity(n, format="csr") * 30.0


def sample(ctx, slots, reps):
    ctx.profile_enable(True)
    for _ in range(reps):
        ctx.residual(_cabi.KIND_LINEAR, slots)
    pr = ctx.profile_read()["spmm"]
    ctx.profile_enable(False)
    assert pr["launches"] == reps, pr
    return pr["ms"] / reps


def measure(name, A, Ps, out, reps=10):
    """One line per P: both methods on `A`, alternating."""
    A = sp.csr_matrix(A, dtype=np.complex128)
    A.sum_duplicates()
    A.sort_indices()
    n = A.shape[0]
    ctxs = [Context(0), Context(0)]
    try:
        X = None
        for method, ctx in enumerate(ctxs):
            ctx.spmm_set_method(method)
            ctx.set_matrix_csr(A)
            ctx.set_rhs(np.ones(n, dtype=np.complex128))
            ctx.pop_reserve(max(Ps))
            if X is None:
                rng = np.random.default_rng(1)
                X = rng.standard_normal((max(Ps), n)) + 1j * rng.standard_normal((max(Ps), n))
            ctx.pop_put(_cabi.POP_X, list(range(max(Ps))), X)
        kern = ctxs[1].spmm_kernel_for(False)
        ns = -(-n // 64)                                                         # the layout's size, whether or not it is resident
        lens = np.zeros(ns * 64, dtype=np.int64)
        lens[:n] = np.diff(A.indptr)
        padded = int(64 * lens.reshape(ns, 64).max(axis=1).sum())
        fill = padded / A.nnz
        assert ctxs[1].spmm_sell_info(False)[1] == (padded if kern == 3 else 0)
        assert ctxs[0].spmm_kernel_for(False) in (1, 2)
        for P in Ps:
            sl = list(range(P))
            for ctx in ctxs:
                sample(ctx, sl, 2)                                               # warm-up of this shape
            ts = [[], []]
            for _ in range(SAMPLES):
                for method, ctx in enumerate(ctxs):
                    ts[method].append(sample(ctx, sl, reps))
            ms0, ms1 = (float(np.median(t)) for t in ts)
            if P == Ps[0]:                                                       # the same bits, at the size that is timed
                y0, y1 = (ctx.pop_get(_cabi.POP_Y, sl, n) for ctx in ctxs)
                assert np.array_equal(y0, y1), name
            nbytes = 32.0 * n * P + (20.0 * A.nnz + 4.0 * (n + 1)) * ((P + 7) // 8)
            f0, f1 = (nbytes / (ms * 1e-3) / 1e12 / COPY_TBS for ms in (ms0, ms1))
            ratio = ms0 / ms1
            verdict = ("bar met" if ratio >= BAR else "bar NOT met") if kern == 3 else "stays on the CSR kernel (fill above the cap)"
            line = (f"{name:<34s} n={n:7d} nnz/row={A.nnz / n:5.1f} P={P:3d} kernel={KERNEL[kern]:4s} fill={fill:5.3f}: "
                    f"csr {ms0 * 1e3:8.1f} us ({f0:4.2f} of copy)  sell {ms1 * 1e3:8.1f} us ({f1:4.2f} of copy)  "
                    f"csr/sell {ratio:4.2f}x  {verdict}")
            print(line, flush=True)
            out.append(line)
    finally:
        for ctx in ctxs:
            ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_sell_rates.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 4096 only (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--lib", help="another build of libmaus_hip.so (side-by-side builds: profiles/spmm_sell_variants.txt)")
    args = ap.parse_args()
    if args.lib:
        _cabi.LIB_PATH = os.path.abspath(args.lib)
    probe = Context(0)
    dev = probe.device_info()["name"].strip()              # "<marketing name> (<arch>)"; some drivers leave the name empty
    if dev.startswith("("):
        dev = dev.strip("()")
    probe.close()
    out = [f"# tools/spmm_rates.py on {dev}: the CSR lane-per-row kernel -> the sliced-ELL kernel (maus_spmm_set_method 0 -> 1), the same",
           f"# matrix and rows in two contexts of one process, alternating; us per launch from HIP events, median of {SAMPLES} samples of 10",
           f"# launches after a warm-up; share of the {COPY_TBS} TB/s copy rate over the algorithmic bytes (padding not counted); bar {BAR}x.",
           "# The outputs of the two methods are compared bit for bit at the first P of every matrix."]
    if args.lib:
        out.append(f"# library: {os.path.basename(args.lib)}")
    print("\n".join(out), flush=True)
    out.append("# -- the shapes of profiles/sparse_rates.txt: banded, 5 and 27 per row")
    for n in (4096,) if args.quick else (4096, 16384):
        for per_row in (5, 27):
            measure(f"banded {per_row}/row", banded(n, per_row), (1, 33, 256), out)
    if not args.quick:
        out.append("# -- both operands of a random pattern at n = 16384 (A^H has ragged rows)")
        for per_row in (5, 27):
            A = random_pattern(16384, per_row)
            measure(f"random {per_row}/row, A", A, (1, 33, 256), out)
            measure(f"random {per_row}/row, A^H", A.conj().T.tocsr(), (1, 33, 256), out)
        out.append("# -- n = 2^20")
        measure("tridiagonal", banded(1 << 20, 3), (1, 64), out)
        measure("banded 27/row", banded(1 << 20, 27), (1, 64), out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
