"""Dense population products of at most 32 rows (csrc/zgemm.hip, DESIGN §3 "Few rows"): the default kernels and split-K
(maus_few_rows_set_method(ctx, 1)) side by side in one process on one device -> profiles/few_rows_rates.txt.

Rows: A X (the residual's product) at 1 / 15 / 16 / 32 rows for n = 2048, 4096, 8192, 16384; conj(X) V (the Hermitian match) at
15 rows for n = 8192; the Gram block of 15 and 32 rows of length 8192 and 16384; the pair of products of the SVD power step at 15
rows on 2048 x 2048.  The two methods alternate on the same resident operands after one warm-up call each; per method the
better of two timed windows of at least 0.2 s.  Times are the HIP-event brackets of the library's zgemm class around the
product (slice and join launches together under split-K), per call.  Per row:
    ms default / split-K and their ratio; the bar is 1.25
    TB/s          algorithmic bytes (both operands and the result once) over each time, and as a share of the 6.29 TB/s copy rate
    bound         which of HBM (bytes at the copy rate) and the fp64 matrix pipe (8 M N K flops on 16-row tiles at 78 TFLOP/s)
                  takes longer for the shape
    S             the rule's slices
Then the sweep over forced slices (1 = the default kernels) the rule's constants were chosen from.

    python tools/few_rows_rates.py [--out profiles/few_rows_rates.txt] [--quick] [--bodies]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402

COPY, PIPE, BAR, WINDOW = 6.29e12, 78e12, 1.25, 0.2
POP_X, POP_U = 0, 1


def block_matrix(rows, cols, seed):
    """Random-looking complex matrix built from one 512 x 512 block (the values do not matter for the rates)."""
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal((512, 512)) + 1j * rng.standard_normal((512, 512))) / np.sqrt(cols)
    return np.ascontiguousarray(np.tile(b, ((rows + 511) // 512, (cols + 511) // 512))[:rows, :cols])


def measure(ctx, call, method, slices=0):
    """ms per product of `call` under (method, slices): zgemm-class event time over its launches, better of two windows."""
    ctx.few_rows_set_method(method, slices)
    call()
    best = None
    for _ in range(2):
        ctx.profile_enable(False)
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < WINDOW:
            for _ in range(8):
                call()
        pr = ctx.profile_read()["zgemm"]
        ms = pr["ms"] / pr["launches"]
        best = ms if best is None else min(best, ms)
    ctx.profile_enable(False)
    ctx.few_rows_set_method(_cabi.FEW_ROWS_DEFAULT)
    return best


def report(out, name, M, N, K, form, nprod, ms0, ms1, S):
    by = 16.0 * (M * K + N * K + M * N) * nprod
    t_hbm, t_pipe = by / COPY, 8.0 * (16 * ((M + 15) // 16)) * N * K * nprod / PIPE
    ratio = ms0 / ms1
    line = (f"{name:<26} {M:>2} x {N:>5} x {K:>5} | ms {ms0:8.4f} -> {ms1:8.4f} (x{ratio:5.2f}) | TB/s {by / ms0 / 1e9:6.3f} ({by / ms0 / 1e9 / (COPY / 1e12):5.3f} of copy)"
            f" -> {by / ms1 / 1e9:6.3f} ({by / ms1 / 1e9 / (COPY / 1e12):5.3f}) | bound {'HBM' if t_hbm >= t_pipe else 'fp64 pipe'} "
            f"({1e3 * t_hbm:.4f} / {1e3 * t_pipe:.4f} ms) | S {S:>2} | bar {BAR}: {'met' if ratio >= BAR else 'NOT met'}")
    print(line, flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "few_rows_rates.txt"))
    ap.add_argument("--quick", action="store_true", help="n up to 4096 only")
    ap.add_argument("--bodies", action="store_true", help="also the 15-candidate loop bodies of configs[3]'s shape (n = 8192 Hermitian)")
    args = ap.parse_args()
    ctx = _cabi.Context(0)
    dev = ctx.device_info()["name"].strip() or "the device"
    out = [f"# tools/few_rows_rates.py on {dev}: default kernels -> split-K (maus_few_rows_set_method 0 -> 1), same resident operands,",
           "# alternating after a warm-up; ms per product from the zgemm class's HIP events, better of two windows of >= 0.2 s"]
    sweep = ["# sweep over forced slices (ms per product; 1 = the default kernels; * = the rule's choice)"]
    sizes = (2048, 4096) if args.quick else (2048, 4096, 8192, 16384)
    SW = (1, 2, 4, 8, 16, 32)
    slots = {M: np.arange(M, dtype=np.int32) for M in (1, 15, 16, 32)}

    def sweep_row(name, M, N, K, form, call):
        S = ctx_S(M, N, K, form)
        ms = [measure(ctx, call, 0) if s == 1 else measure(ctx, call, 1, s) for s in SW]
        line = f"{name:<26} {M:>2} x {N:>5} x {K:>5} | " + "  ".join(f"S={s:<2}{'*' if s == S else ' '}{m:8.4f}" for s, m in zip(SW, ms))
        print(line, flush=True)
        sweep.append(line)

    def ctx_S(M, N, K, form):
        ctx.few_rows_set_method(1)
        kern, S = ctx.few_rows_kernel_for(M, N, K, *form)
        ctx.few_rows_set_method(0)
        return S if kern else 1

    def both(name, M, N, K, form, call, nprod=1):
        ms0, ms1 = measure(ctx, call, 0), measure(ctx, call, 1)
        report(out, name, M, N, K, form, nprod, ms0 * nprod, ms1 * nprod, ctx_S(M, N, K, form))

    for n in sizes:
        ctx.set_matrix(block_matrix(n, n, n))
        ctx.pop_reserve(32)
        rng = np.random.default_rng(n)
        ctx.pop_put(POP_X, slots[32], rng.standard_normal((32, n)) + 1j * rng.standard_normal((32, n)))
        lam = np.zeros(32, dtype=np.complex128)
        for M in (1, 15, 16, 32):
            both("A X (residual)", M, n, n, (1, False, False), lambda: ctx.residual(_cabi.KIND_EIG, slots[M], lam[:M]))
        for M in (15, 32):
            sweep_row("A X (residual)", M, n, n, (1, False, False), lambda: ctx.residual(_cabi.KIND_EIG, slots[M], lam[:M]))
        if n in (8192, 16384) or (args.quick and n == 4096):
            for M in (15, 32):
                both("Gram block", M, M, n, (1, True, False), lambda: ctx.gram(POP_X, slots[M], n))
            sweep_row("Gram block", 15, 15, n, (1, True, False), lambda: ctx.gram(POP_X, slots[15], n))
        if n == 8192 or (args.quick and n == 4096):
            ctx.set_eigvecs(block_matrix(n, n, 7))
            both("conj(X) V (herm_match)", 15, n, n, (0, True, False), lambda: ctx.herm_match(slots[15]))
            sweep_row("conj(X) V (herm_match)", 15, n, n, (0, True, False), lambda: ctx.herm_match(slots[15]))
            ctx.pop_put(POP_X, slots[32], rng.standard_normal((32, n)) + 1j * rng.standard_normal((32, n)))   # (the match replaced x)
        if n == 2048:
            both("SVD pair (A v, A^H u)", 15, n, n, (0, False, True), lambda: ctx.svd_power_propose(slots[15]), nprod=2)
            sweep_row("SVD pair (A v, A^H u)", 15, n, n, (0, False, True), lambda: ctx.svd_power_propose(slots[15]))
    out += sweep
    ctx.close()
    if args.bodies:
        out += bodies()
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


def bodies(n=8192, P=15, count=3):
    """ms per loop body of MAUS_Solver on a Hermitian n x n eigenproblem with P candidates (configs[3]'s late bodies), few_rows
    auto and splitk.  Reported only: the body is bound by its eight synchronising calls."""
    import random
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    import scenarios
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    A = scenarios.hermitian(n, 8192)
    lines, diag = [], None
    for mode in ("auto", "splitk"):
        np.random.seed(1234); random.seed(1234); SolutionCandidate._candidate_id_counter = 0
        s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=P, quiet=True, record_history=False, few_rows=mode, diag_info=diag)
        diag = s.diag_info
        ms = []
        for it in range(1, count + 2):
            t0 = time.perf_counter()
            steps = s.loop_body(it)
            s.engine.ctx.sync()
            ms.append((1e3 * (time.perf_counter() - t0), steps))
        lines.append(f"MAUS_Solver Hermitian n {n} P {P}, few_rows={mode:<6}: loop bodies 2.. " + ", ".join(f"{m:.2f} ms / {st} steps" for m, st in ms[1:])
                     + "  (wall, reported only)")
        print(lines[-1], flush=True)
    return lines


if __name__ == "__main__":
    main()
