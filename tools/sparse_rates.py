"""Rates of the sparse path: the CSR SpMM and a sparse linear loop body beside the dense one.

    python tools/sparse_rates.py [--no-dense]          (profiles/sparse_rates.txt)

SpMM: one product Y = A X of P population rows through maus_residual (linear kind: the product is always recomputed there),
timed by the library's HIP-event profile of the "spmm" class.  Algorithmic bytes: X read + Y written (16 B per complex
element each) + the CSR operand (16 B value + 4 B index per nonzero, 4 B per row pointer) once per group of 8 candidates.
The reference copy rate is MI355X_MICROARCH's measured 6.29 TB/s.

Loop bodies: candidate-steps/s of MAUS_Solver.loop_body on a sparse linear system (n = 16384, P = 256, GMRES preferred:
a sparse problem is 'Critical', AMS:405-412), and of the same loop body on a dense matrix (every entry nonzero) given the
same strategy through diag_info, so that both take the GMRES path.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adaptive_matrix_solver_amd import Context  # noqa: E402

COPY_TBS = 6.29


def banded(n, per_row, seed=0):
    """per_row nonzeros per row: the diagonal and its nearest off-diagonals (banded, as a stencil operator)"""
    rng = np.random.default_rng(seed)
    offs = [o for o in range(-(per_row // 2), per_row // 2 + 1)][:per_row]
    diags = [rng.standard_normal(n - abs(o)) + 1j * rng.standard_normal(n - abs(o)) for o in offs]
    return sp.csr_matrix(sp.diags(diags, offs, shape=(n, n)) + sp.identity(n) * 2.0 * per_row)


def spmm_rates():
    print("# SpMM  Y = A X  (one product, P population rows; HIP-event time of the spmm class, median of 5)")
    for n in (4096, 16384):
        for per_row in (5, 27):
            A = banded(n, per_row)
            ctx = Context(0)
            try:
                ctx.set_matrix_csr(A)
                ctx.set_rhs(np.ones(n, dtype=np.complex128))
                ctx.pop_reserve(256)
                rng = np.random.default_rng(1)
                ctx.pop_put(0, list(range(256)), rng.standard_normal((256, n)) + 1j * rng.standard_normal((256, n)))
                for P in (1, 33, 256):
                    sl = list(range(P))
                    ctx.residual(2, sl)
                    ts = []
                    for _ in range(5):
                        ctx.profile_enable(True)
                        ctx.residual(2, sl)
                        pr = ctx.profile_read()["spmm"]
                        ctx.profile_enable(False)
                        ts.append(pr["ms"] / max(1, pr["launches"]))
                    ms = float(np.median(ts))
                    nbytes = 32.0 * n * P + (20.0 * A.nnz + 4.0 * (n + 1)) * ((P + 7) // 8)
                    tbs = nbytes / (ms * 1e-3) / 1e12
                    print(f"n={n:5d} nnz/row={A.nnz / n:5.1f} P={P:3d} schedule={ctx.matrix_is_sparse():4s}: {ms * 1e3:8.1f} us, "
                          f"{nbytes / 1e6:8.2f} MB, {tbs:5.2f} TB/s = {tbs / COPY_TBS:4.2f} of copy", flush=True)
            finally:
                ctx.close()


def loop_body_rate(A, b, P, iters, **kw):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    np.random.seed(7)
    random.seed(7)
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=P, quiet=True, **kw)
    s.loop_body(1)                                                  # warm-up (workspaces, first allocations)
    steps0 = s.engine.steps_executed
    t0 = time.perf_counter()
    for it in range(iters):
        s.loop_body(it + 2)
    dt = time.perf_counter() - t0
    return (s.engine.steps_executed - steps0) / dt, s.problem_knowledge["local_solver_preference"], dt


def loop_bodies(dense=True):
    n, P = 16384, 256
    A = banded(n, 5, seed=3)
    b = np.random.default_rng(2).standard_normal(n) + 0j
    rate, pref, dt = loop_body_rate(A, b, P, 3, sparse_mode="device")
    print(f"# loop bodies, linear, n={n}, P={P}, gmres_compat='rtol'")
    print(f"sparse (nnz/row 5, CSR):  {rate:9.1f} candidate-steps/s  (3 bodies in {dt:.2f} s, preference {pref})", flush=True)
    if dense:
        D = A.toarray()
        D += 1e-3 * (np.random.default_rng(4).standard_normal((n, n)) + 0j)      # every entry nonzero: the dense path
        di = {"is_hermitian": False, "is_complex_symmetric": False, "is_sparse_init": False, "condition_number": np.inf,
              "is_singular": True}                                                 # the sparse problem's strategy
        rate, pref, dt = loop_body_rate(D, b, P, 2, diag_info=di)
        print(f"dense (same n, zgemm):    {rate:9.1f} candidate-steps/s  (2 bodies in {dt:.2f} s, preference {pref})", flush=True)


if __name__ == "__main__":
    spmm_rates()
    loop_bodies(dense="--no-dense" not in sys.argv)
