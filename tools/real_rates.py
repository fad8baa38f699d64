"""Real against complex arithmetic for GMRES on real sparse systems (maus_real_set_method, csrc/gmres.hip and csrc/spmm.hip;
DESIGN §11 "GMRES in real arithmetic"), side by side in one process on one device -> profiles/real_arith_rates.txt.

Rows: the rows of tools/gmres_rates.py with real values -- the 2-D 5-point operator + 2 I at n = 65536 with P = 1, 15, 64, 256
and at n = 262144 with P = 1, 15, 64; a tridiagonal operator at n = 2^20 with P = 1, 15, 46 -- under both post schedules
(sparse_gmres auto / wide).  One real b (rhs_mode 1, x0 = b), a real shift per candidate; a call is a whole solve (restart 20,
rtol 1e-8).  The two paths alternate on the same systems: per path one warm-up call, then the better of two timed calls.
The baseline of every row is the complex path of the same build in the same process.  Per row:
    wall ms per solve       time.perf_counter around the synchronising call, divided by P           complex, real, (ratio)
    post ms per solve       the HIP-event profile of the post step's class ('vector' / 'gmres_wide' against 'gmres_real')
    spmm us per product     the profile of the product's class ('spmm' against 'spmm_real'), per launch
    TB/s                    the real path's own algorithmic bytes (its profile classes) over its time, and that as a share of the
                            6.29 TB/s copy rate
    bar 1.25                met where post step AND wall are 1.25 times faster; x, info and inner must be equal, or the row says so
Then the products alone under sparse_spmm csr and sell (P rows of the population per launch), and MAUS_Solver linear loop
bodies at n = 65536, P = 64 under real_arith off / on.

    python tools/real_rates.py [--out profiles/real_arith_rates.txt] [--quick] [--no-loop]
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402

COPY = 6.29e12
BAR = 1.25
FORCE = 1000000


def five_point_2i(m):
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    L = sp.kron(sp.identity(m), T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(m))
    return (L + 2.0 * sp.identity(m * m)).tocsr().astype(np.complex128)


def tridiagonal(n, seed=14):
    rng = np.random.default_rng(seed)
    return sp.diags([rng.standard_normal(n - 1), 4.0 + 0.1 * rng.standard_normal(n), rng.standard_normal(n - 1)],
                    [-1, 0, 1], format="csr").astype(np.complex128)


def timed(ctx, real, gm, P, shift, psi, jac):
    """(profile, wall seconds, x, info, inner) of the better of two timed solves after a warm-up."""
    ctx.real_set_method(_cabi.REAL_ON if real else _cabi.REAL_OFF)
    ctx.gmres_set_method(gm)
    assert ctx.real_plan(1, shift)["real"] == bool(real)
    post = "gmres_real" if real else ("gmres_wide" if gm else "vector")
    slots = np.arange(P)
    ctx.gmres(slots, shift, psi, 1, jac)
    best = None
    for _ in range(2):
        ctx.profile_enable(False)
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        info, inner, status = ctx.gmres(slots, shift, psi, 1, jac)
        wall = time.perf_counter() - t0
        pr = ctx.profile_read()
        assert (status == 0).all(), status
        if best is None or pr[post]["ms"] < best[0][post]["ms"]:
            best = (pr, wall, info, inner)
    ctx.profile_enable(False)
    x = ctx.pop_get(_cabi.POP_W, slots[: min(P, 4)], ctx.rows)
    return best + (x, post)


def row(ctx, name, n, P, gm, out):
    rng = np.random.default_rng(2)
    shift = 0.1 * rng.standard_normal(P) + 0j
    psi = np.full(P, 1e-20)
    jac = np.zeros(P, dtype=np.int32)
    pc, wall_c, info_c, inner_c, xc, post_c = timed(ctx, False, gm, P, shift, psi, jac)
    pr, wall_r, info_r, inner_r, xr, post_r = timed(ctx, True, gm, P, shift, psi, jac)
    ctx.real_set_method(_cabi.REAL_OFF)
    same = np.array_equal(info_c, info_r) and np.array_equal(inner_c, inner_r) and np.array_equal(xc, xr)
    post_ratio = pc[post_c]["ms"] / pr[post_r]["ms"]
    wall_ratio = wall_c / wall_r
    sp_c = 1e3 * pc["spmm"]["ms"] / max(1, pc["spmm"]["launches"])
    sp_r = 1e3 * pr["spmm_real"]["ms"] / max(1, pr["spmm_real"]["launches"])
    rate_post = pr[post_r]["bytes"] / (pr[post_r]["ms"] / 1e3)
    rate_spmm = pr["spmm_real"]["bytes"] / (pr["spmm_real"]["ms"] / 1e3)
    verdict = "met" if post_ratio >= BAR and wall_ratio >= BAR else ("met on the post step only" if post_ratio >= BAR else "MISSED")
    line = (f"{name:<14} n {n:>8} P {P:>4} {'wide' if gm else 'auto'} | wall ms/solve {1e3 * wall_c / P:9.3f} {1e3 * wall_r / P:9.3f} (x{wall_ratio:5.2f}) | "
            f"post ms/solve {pc[post_c]['ms'] / P:9.3f} {pr[post_r]['ms'] / P:9.3f} (x{post_ratio:5.2f}) | spmm us/product {sp_c:8.1f} {sp_r:8.1f} (x{sp_c / sp_r:5.2f}) | "
            f"real TB/s post {rate_post / 1e12:6.3f} ({rate_post / COPY:5.3f} of copy) spmm {rate_spmm / 1e12:6.3f} ({rate_spmm / COPY:5.3f}) | "
            f"inner {int(inner_r.min())}..{int(inner_r.max())} converged {int((info_r == 0).sum())}/{P} x, info, inner {'equal' if same else 'DIFFER'} | bar {BAR}: {verdict}")
    print(line, flush=True)
    out.append(line)


def products(ctx, name, n, P, out):
    """The product alone on P population rows: complex (maus_matvec_rayleigh's product) against real (maus_real_spmm), under
    both SpMM methods; us per launch from the profile classes, the better of three."""
    rng = np.random.default_rng(5)
    for k0 in range(0, P, 8):
        k1 = min(P, k0 + 8)
        ctx.pop_put(_cabi.POP_X, np.arange(k0, k1), rng.standard_normal((k1 - k0, n)) + 0j)
    slots = np.arange(P)
    ctx.real_set_method(_cabi.REAL_ON)
    for method, label in ((_cabi.SPMM_CSR, "csr"), (_cabi.SPMM_SELL, "sell")):
        ctx.spmm_set_method(method, FORCE if method else 0)
        best = {"spmm": None, "spmm_real": None}
        for _ in range(4):                                   # the first pass warms up
            for klass, call in (("spmm", lambda: ctx.matvec_rayleigh(slots)), ("spmm_real", lambda: ctx.real_spmm(slots))):
                ctx.pop_put(_cabi.POP_Y, [0], np.zeros((1, n), dtype=np.complex128))  # drops every kept-product stamp
                ctx.profile_enable(False)
                ctx.profile_enable(True)
                call()
                pr = ctx.profile_read()[klass]
                if best[klass] is None or pr["ms"] < best[klass]["ms"]:
                    best[klass] = pr
        ctx.profile_enable(False)
        c, r = best["spmm"], best["spmm_real"]
        ratio = c["ms"] / r["ms"]
        rate = r["bytes"] / (r["ms"] / 1e3)
        line = (f"product {name:<14} n {n:>8} P {P:>4} {label:<4} kernel {ctx.spmm_kernel_for(False)} | us/product {1e3 * c['ms']:9.1f} {1e3 * r['ms']:9.1f} (x{ratio:5.2f}) | "
                f"real TB/s {rate / 1e12:6.3f} ({rate / COPY:5.3f} of copy) | bar {BAR}: {'met' if ratio >= BAR else 'MISSED'}")
        print(line, flush=True)
        out.append(line)
    ctx.spmm_set_method(_cabi.SPMM_CSR)
    ctx.real_set_method(_cabi.REAL_OFF)


def bind(ctx, A, P):
    n = A.shape[0]
    ctx.set_matrix_csr(A)
    ctx.pop_reserve(P)
    ctx.set_rhs(np.random.default_rng(1).standard_normal(n) + 0j)


def loop_rate(mode, bodies=3):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    A = five_point_2i(256)
    b = np.random.default_rng(8).standard_normal(65536) + 0j
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=64, quiet=True, sparse_mode="device",
                    gmres_compat="rtol", real_arith=mode, diag_info=diag)
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
    post = pr["gmres_real"]["ms"] + pr["vector"]["ms"]
    spmm = pr["spmm_real"]["ms"] + pr["spmm"]["ms"]
    ctx.close()
    return steps / wall, post / bodies, spmm / bodies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "real_arith_rates.txt"))
    ap.add_argument("--quick", action="store_true", help="n = 65536 only (a check of the tool, not the record)")
    ap.add_argument("--no-loop", action="store_true", help="leave out the MAUS_Solver loop bodies")
    a = ap.parse_args()
    ctx = _cabi.Context(0)
    out = [f"# tools/real_rates.py on {(ctx.device_info()['name'].strip() or 'the device')}: complex -> real arithmetic (maus_real_set_method 0 -> 1), same real systems,",
           "# one process, the two paths alternating; wall and post-step ms per solve and SpMM us per product (better of two timed calls",
           "# after a warm-up), complex / real in brackets; TB/s: the real kernels' own algorithmic bytes over their time, and as a share",
           "# of the 6.29 TB/s copy rate.  Expected from the bytes alone: post step towards 2x, SpMM 1.7-2x, less where a row is launch-bound."]
    print("\n".join(out), flush=True)
    plan = [("5-point + 2 I", lambda: five_point_2i(256), (1, 15, 64, 256))]
    if not a.quick:
        plan += [("5-point + 2 I", lambda: five_point_2i(512), (1, 15, 64)), ("tridiagonal", lambda: tridiagonal(1 << 20), (1, 15, 46))]
    for name, make, Ps in plan:
        A = make()
        bind(ctx, A, max(Ps))
        for gm in (_cabi.GMRES_DEFAULT, _cabi.GMRES_WIDE):
            for P in Ps:
                row(ctx, name, A.shape[0], P, gm, out)
        ctx.gmres_set_method(_cabi.GMRES_DEFAULT)
        products(ctx, name, A.shape[0], min(64, max(Ps)), out)
    ctx.close()
    if not a.quick and not a.no_loop:
        rates = {}
        for mode in ("off", "on"):
            rates[mode] = loop_rate(mode)
            rate, post_ms, spmm = rates[mode]
            line = (f"MAUS_Solver linear loop bodies n 65536 P 64, GMRES path, real_arith={mode:<3}: {rate:8.1f} candidate-steps/s, "
                    f"vector + post step {post_ms:8.2f} ms/body, spmm {spmm:8.2f} ms/body")
            print(line, flush=True)
            out.append(line)
        ratio = rates["on"][0] / rates["off"][0]
        line = f"MAUS_Solver loop bodies, on / off: x{ratio:5.2f} candidate-steps/s | bar {BAR}: {'met' if ratio >= BAR else 'MISSED'}"
        print(line, flush=True)
        out.append(line)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
