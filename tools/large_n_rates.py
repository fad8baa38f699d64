"""ms per solve of maus_shifted_lu_solve above the old n <= 8192 limit (device-regenerated perturbation: the bench's mode),
one solve per call and a whole workspace per call, with the split of one profiled call by kernel class.

    python tools/large_n_rates.py [n ...]          (default 8192 12288 16384; profiles/large_n_lu_rates.txt)

TFLOP/s are algorithmic: 8/3 n^3 per solve (complex LU counted as 8 real flops per multiply-add, the back substitution
left out).  The profiled call brackets every launch with HIP events, so its classes add up to a little more than the
timed calls.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import scenarios  # noqa: E402
from adaptive_matrix_solver_amd import Context  # noqa: E402
from adaptive_matrix_solver_amd._cabi import PERT_MT19937  # noqa: E402

SPLIT = [("panel", ("lu_panel",)), ("trsm", ("trsm",)), ("zgemm", ("zgemm", "zgemm_k128", "zgemm_k64", "zgemm_k32", "zgemm_k16")),
         ("backsolve", ("backsolve",)), ("build_h", ("build_h",))]

sizes = [int(a) for a in sys.argv[1:]] or [8192, 12288, 16384]
for n in sizes:
    A = scenarios.ginibre(n, n)
    ctx = Context(0)
    try:
        ctx.set_matrix(A)
        cap = ctx.lu_reserve(n, 512)                      # the workspace maximum: 80 % of free HBM, MAUS_LU_BATCH
        P = cap
        ctx.pop_reserve(P)
        rng = np.random.default_rng(1)
        V = (rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))) / np.sqrt(n)
        ctx.pop_put(0, list(range(P)), V)
        num, den = ctx.matvec_rayleigh(list(range(P)))
        lam = num / den
        psi = np.full(P, 1e-20)
        np.random.seed(3)
        st = np.random.get_state()
        print(f"# n={n}: workspace capacity {cap} solves ({ctx.lu_workspace_allocations()} allocation)", flush=True)
        for G in sorted({1, cap}):
            sl = list(range(G))
            desc = (st, 4 * n * n, 0, np.arange(G, dtype=np.int32))
            status = ctx.shifted_lu_solve(sl, lam[:G], psi[:G], 0, PERT_MT19937, desc)          # warm
            assert (status == 0).all(), status
            reps = 2
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.shifted_lu_solve(sl, lam[:G], psi[:G], 0, PERT_MT19937, desc)
            dt = (time.perf_counter() - t0) / reps
            ctx.profile_enable(1)
            ctx.shifted_lu_solve(sl, lam[:G], psi[:G], 0, PERT_MT19937, desc)
            pr = ctx.profile_read()
            ctx.profile_enable(False)
            parts = {k: sum(pr[c]["ms"] for c in cls) for k, cls in SPLIT}
            tot = sum(parts.values())
            tf = 8.0 / 3.0 * n ** 3 * G / dt / 1e12
            split = " ".join(f"{k} {v:.1f} ({100 * v / tot:.1f} %)" for k, v in parts.items())
            print(f"n={n:5d} G={G:3d}: {dt * 1e3:9.1f} ms per call, {dt * 1e3 / G:8.2f} ms per solve, {tf:5.1f} TFLOP/s"
                  f" | profiled call, ms: {split}", flush=True)
    finally:
        ctx.close()
