"""GMRES post-step rates (csrc/gmres.hip): the default schedule (one workgroup per candidate: a register kernel
up to n = 16384, the stream kernel above) and the wide step (maus_gmres_set_method(ctx, 1)) side by side in one process on one
device -> profiles/gmres_wide_rates.txt.

Rows: the 2-D 5-point operator (complex values) + 2 I at n = 65536 with P = 1, 15, 64, 256 and at n = 262144 with P = 1, 15, 64;
a complex tridiagonal operator at n = 2^20 with P = 1, 15, 46.  Every candidate has its own right-hand side and shift; a call
is a whole solve (restart 20, rtol 1e-8) from x0 = b.  The two methods alternate on the same systems from the same start; per
method one warm-up call, then the better of two timed calls.  Per row:
    wall ms per solve       time.perf_counter around the synchronising call, divided by P
    post ms per solve       the HIP-event profile of the post step's class ('vector' / 'gmres_wide'), divided by P
    stream / wide           of the post ms, and of the wall ms; the bar is 1.25
    launches per tick       2 (compact, SpMM) + the post step's: 1 by default; col + 4 under wide (6 in a residual tick)
    TB/s                    the wide step's algorithmic bytes (its profile class: 64 n per candidate and Gram-Schmidt column,
                            plus form, tail, finish and new-cycle passes) over each method's post time, and that as a share of
                            the 6.29 TB/s copy rate; under the default schedule and P workgroups it is also GB/s per workgroup
Then MAUS_Solver linear loop bodies at n = 65536, P = 64 on the GMRES path under both methods.

--register: instead, the register kernels of the default schedule, one row per instantiation of gmres_post_kernel, in the dense
shared-matrix mode (diag(linspace(1, 3, n)) + 0.5 G / sqrt(n), P = 256 candidates, one workgroup each) at n = 1024, 4096, 8192
and 12288, and one row of the dense mode (maus_gmres_pert, materialised H_k: gemv_dense_kernel + post) at n = 1024, P = 32.
--post FILE writes `row <tab> post ms per solve` of every row, for comparisons between two builds of the library; MAUS_LIB
names the build to load (default: the tree's).

    python tools/gmres_rates.py [--out profiles/gmres_wide_rates.txt] [--quick] [--register] [--no-loop] [--post FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402
if os.environ.get("MAUS_LIB"):                               # another build of the library, for before / after comparisons
    _cabi.LIB_PATH = os.environ["MAUS_LIB"]

COPY = 6.29e12
BAR = 1.25


def five_point_2i(m, seed=0):
    rng = np.random.default_rng(seed)
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    L = (sp.kron(sp.identity(m), T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(m))).tocsr()
    L = L.astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    return (L + 2.0 * sp.identity(m * m)).tocsr()


def tridiagonal(n, seed=14):
    rng = np.random.default_rng(seed)
    return sp.diags([rng.standard_normal(n - 1) + 0j, 4.0 + 1j + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1) + 0j],
                    [-1, 0, 1], format="csr")


def timed(ctx, method, P, shift, psi, jac, dense=False):
    """(post-step profile record, wall seconds, info, inner, ticks) of the better of two timed solves after a warm-up."""
    ctx.gmres_set_method(method)
    klass = "gmres_wide" if method == _cabi.GMRES_WIDE else "vector"
    slots = np.arange(P)
    if dense:
        solve = lambda: ctx.gmres_pert(slots, shift, psi, 0, jac, _cabi.PERT_NONE, None)[:3]
    else:
        solve = lambda: ctx.gmres(slots, shift, psi, 0, jac)
    solve()
    best = None
    for _ in range(2):
        ctx.profile_enable(False)
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        info, inner, status = solve()
        wall = time.perf_counter() - t0
        pr = ctx.profile_read()
        assert (status == 0).all(), status
        if best is None or pr[klass]["ms"] < best[0]["ms"]:
            best = (pr[klass], wall, info, inner, pr["spmm"]["launches"])
    ctx.profile_enable(False)
    return best


def launches_per_tick(inner, ticks, restart=20):
    """Mean kernel launches per tick of the wide step for a batch whose slowest candidate took `inner` iterations: a tick at
    column col issues compact, SpMM, form, col Gram-Schmidt columns, tail, state, finish; a residual tick compact, SpMM, form
    and three more."""
    total, left = 0, int(inner)
    while left > 0:
        m = min(restart, left)
        total += sum(col + 6 for col in range(m))
        left -= m
    resid = max(0, ticks - int(inner))
    return (total + 6 * resid) / max(1, int(inner) + resid)


def register_row(ctx, name, n, P, out, post, dense=False):
    """One row of the --register table: the default schedule alone, post-step (vector class) and wall us per solve."""
    rng = np.random.default_rng(2)
    shift = 0.1 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-3 if dense else 1e-20)
    jac = np.zeros(P, dtype=np.int32)
    ps, wall, info, inner, _ = timed(ctx, _cabi.GMRES_DEFAULT, P, shift, psi, jac, dense)
    line = (f"{name:<22} n {n:>8} P {P:>4} | wall us/solve {1e6 * wall / P:9.3f} | post us/solve {1e3 * ps['ms'] / P:9.3f} | "
            f"inner {int(inner.min())}..{int(inner.max())} converged {int((info == 0).sum())}/{P}")
    print(line, flush=True)
    out.append(line)
    post.append((f"{name} n {n} P {P}", ps["ms"] / P))


def bind_dense(ctx, n, P):
    rng = np.random.default_rng(n)
    A = (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) * (0.5 / np.sqrt(n))
    A[np.arange(n), np.arange(n)] += np.linspace(1.0, 3.0, n)
    ctx.set_matrix(A)
    ctx.pop_reserve(P)
    rng = np.random.default_rng(1)
    for k0 in range(0, P, 8):
        k1 = min(P, k0 + 8)
        ctx.pop_put(_cabi.POP_X, np.arange(k0, k1), rng.standard_normal((k1 - k0, n)) + 1j * rng.standard_normal((k1 - k0, n)))


def row(ctx, name, n, P, out, post):
    rng = np.random.default_rng(2)
    shift = 0.1 * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    psi = np.full(P, 1e-20)
    jac = np.zeros(P, dtype=np.int32)
    ps, wall_s, info_s, inner_s, _ = timed(ctx, _cabi.GMRES_DEFAULT, P, shift, psi, jac)
    pw, wall_w, info_w, inner_w, ticks = timed(ctx, _cabi.GMRES_WIDE, P, shift, psi, jac)
    ctx.gmres_set_method(_cabi.GMRES_DEFAULT)
    same = np.array_equal(info_s, info_w) and np.array_equal(inner_s, inner_w)
    by = pw["bytes"]
    rs, rw = by / (ps["ms"] / 1e3), by / (pw["ms"] / 1e3)
    post_ratio, wall_ratio = ps["ms"] / pw["ms"], wall_s / wall_w
    verdict = "met" if post_ratio >= BAR and wall_ratio >= BAR else ("met on the post step only" if post_ratio >= BAR else "NOT met")
    line = (f"{name:<22} n {n:>8} P {P:>4} | wall ms/solve {1e3 * wall_s / P:9.3f} {1e3 * wall_w / P:9.3f} (x{wall_ratio:5.2f}) | "
            f"post ms/solve {ps['ms'] / P:9.3f} {pw['ms'] / P:9.3f} (x{post_ratio:5.2f}) | launches/tick 3 -> {launches_per_tick(inner_w.max(), ticks):5.1f} | "
            f"TB/s {rs / 1e12:6.3f} ({rs / COPY:5.3f} of copy, {rs / 1e9 / P:7.1f} GB/s per workgroup) -> {rw / 1e12:6.3f} ({rw / COPY:5.3f}) | "
            f"inner {int(inner_w.min())}..{int(inner_w.max())} converged {int((info_w == 0).sum())}/{P} counts {'equal' if same else 'DIFFER'} | bar 1.25: {verdict}")
    print(line, flush=True)
    out.append(line)
    post.append((f"{name} n {n} P {P} default", ps["ms"] / P))
    post.append((f"{name} n {n} P {P} wide", pw["ms"] / P))


def bind(ctx, A, P):
    n = A.shape[0]
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(P)
    rng = np.random.default_rng(1)
    for k0 in range(0, P, 8):
        k1 = min(P, k0 + 8)
        ctx.pop_put(_cabi.POP_X, np.arange(k0, k1), rng.standard_normal((k1 - k0, n)) + 1j * rng.standard_normal((k1 - k0, n)))


def loop_rate(mode, bodies=3):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    A = five_point_2i(256, 7)
    rng = np.random.default_rng(8)
    b = rng.standard_normal(65536) + 1j * rng.standard_normal(65536)
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=64, quiet=True, sparse_mode="device",
                    gmres_compat="rtol", sparse_gmres=mode, diag_info=diag)
    s.loop_body(1)
    ctx = s.engine.ctx
    ctx.profile_enable(False)
    ctx.profile_enable(True)
    steps, t0 = 0, time.perf_counter()
    for it in range(bodies):
        steps += len(s.candidates)
        s.loop_body(it + 2)
    ctx.sync()
    wall = time.perf_counter() - t0
    pr = ctx.profile_read()
    ctx.profile_enable(False)
    post = pr["gmres_wide"]["ms"] if mode == "wide" else pr["vector"]["ms"]
    return steps / wall, post / bodies, pr["spmm"]["ms"] / bodies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gmres_wide_rates.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 65536 only (a check of the tool, not the record)")
    ap.add_argument("--register", action="store_true", help="the register kernels' table instead (dense modes, n <= 12288)")
    ap.add_argument("--no-loop", action="store_true", help="leave out the MAUS_Solver loop bodies")
    ap.add_argument("--post", default=None, help="write `row <tab> post ms per solve` of every row to this file")
    a = ap.parse_args()
    ctx = _cabi.Context(0)
    post = []
    if a.register:
        out = [f"# tools/gmres_rates.py --register on {(ctx.device_info()['name'].strip() or 'the device')}: the default schedule's register kernels,",
               "# one process; wall and post-step ('vector' class) us per solve, the better of two timed calls after a warm-up"]
        print("\n".join(out), flush=True)
        for n in (1024, 4096, 8192, 12288):
            bind_dense(ctx, n, 256)
            register_row(ctx, "dense shared", n, 256, out, post)
        bind_dense(ctx, 1024, 32)
        register_row(ctx, "dense H_k (gemv)", 1024, 32, out, post, dense=True)
        ctx.close()
        finish(a, out, post)
        return
    out = [f"# tools/gmres_rates.py on {(ctx.device_info()['name'].strip() or 'the device')}: default schedule -> wide step (maus_gmres_set_method 0 -> 1), same systems,",
           "# one process; wall and post-step ms per solve (better of two timed calls after a warm-up), stream / wide in brackets;",
           "# TB/s: the wide step's algorithmic bytes over each method's post-step time, and as a share of the 6.29 TB/s copy rate"]
    print("\n".join(out), flush=True)
    plan = [("5-point + 2 I", lambda: five_point_2i(256, 7), (1, 15, 64, 256))]
    if not a.quick:
        plan += [("5-point + 2 I", lambda: five_point_2i(512, 7), (1, 15, 64)), ("tridiagonal", lambda: tridiagonal(1 << 20), (1, 15, 46))]
    for name, make, Ps in plan:
        A = make()
        bind(ctx, A, max(Ps))
        for P in Ps:
            row(ctx, name, A.shape[0], P, out, post)
    ctx.close()
    if not a.quick and not a.no_loop:
        for mode in ("auto", "wide"):
            rate, post_ms, spmm = loop_rate(mode)
            line = (f"MAUS_Solver linear loop bodies n 65536 P 64, GMRES path, sparse_gmres={mode:<5}: {rate:8.1f} candidate-steps/s, "
                    f"post step {post_ms:8.2f} ms/body, spmm {spmm:8.2f} ms/body")
            print(line, flush=True)
            out.append(line)
    finish(a, out, post)


def finish(a, out, post):
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    if a.post:
        os.makedirs(os.path.dirname(a.post) or ".", exist_ok=True)
        with open(a.post, "w") as f:
            f.write("".join(f"{name}\t{ms:.6f}\n" for name, ms in post))


if __name__ == "__main__":
    main()
