"""Band solve rates (csrc/band.hip), the column kernel and the blocked method side by side in one process
-> profiles/band_blocked_rates.txt (profiles/band_rates.txt is the column kernel's record from before the blocked method).

The 2-D 5-point operator (complex values, shuffled, then reordered by band.band_order) at n = 16384, 65536 and 262144: a lone
shifted solve and a batch, timed by the library's HIP-event profile of the "band" / "band_blocked" class (build +
factorisation + solve), first with the column kernel, then with the blocked method, same systems, same context.
Flops 8 n kl (kl + ku) + 8 n (2 kl + ku); bytes = the band storage read and written once (column kernel) or once per block
step over the full reach kl + ku (blocked: an upper end, a matrix that pivots little moves less); the bound is the larger
of the fp64 peak (MI355X: 78.6 TFLOP/s, no MFMA in these kernels) and HBM (8 TB/s).  Then both against the densified dense
LU at n = 16384 for the same 64 shifted systems, and MAUS_Solver linear loop bodies at n = 65536, P = 64 (5-point operator
+ 2 I) on the direct path (gmres_compat='scipy-legacy': every solve a band solve) with sparse_direct 'band' and 'blocked',
and on the GMRES path.

    python tools/band_rates.py [--out profiles/band_blocked_rates.txt]

With --table tiled: the tiled method (maus_band_set_method(ctx, 2)) beside the other two -> profiles/band_tiled_rates.txt.
First the bands only it takes, against the column kernel that runs there otherwise: the 3-D 7-point operator on 40^3
(complex values, shuffled, reordered) alone and in a batch of 8, and a five-diagonal band (offsets 0, +-1, +-k with random
complex values of one size, so that the factorisation pivots and fills the whole band) at n = 32768 with kl = ku = 2048 and
4096 in the identity ordering.  The column kernel takes minutes there: it is timed alone only, one call, no warm-up call.
Then the six rows of the blocked table, tiled beside blocked, same systems.

    python tools/band_rates.py --table tiled [--out profiles/band_tiled_rates.txt]

With --table wide: the wide method (maus_band_set_method(ctx, 4)) beside the tiled method and, where it runs, the blocked
method, in one process on the same systems -> profiles/band_wide_rates.txt: the four rows of the tiled table that only the
tiled and the wide method take, then the six rows of the blocked table.  Per row the ms per solve of each method (the better
of two timed calls after one warm-up call), tiled ms / wide ms, and the share of the fp64 MFMA peak that the wide method's
executed (4M) flops reach.

    python tools/band_rates.py --table wide [--out profiles/band_wide_rates.txt]

With --table narrow: the narrow method (maus_band_set_method(ctx, 8)) against the column kernel, which runs these bands in
every other mode, in one process on the same systems -> profiles/band_narrow_rates.txt.  Tridiagonal and pentadiagonal
operators at n = 65536, 262144 and 2^20 and kl = ku = 15 at n = 65536 and 262144 (complex normal values on every diagonal, the
identity ordering: the factorisation pivots and fills the band), each alone and in a batch of 64; per row the ms per solve of
both (the better of two timed calls after one warm-up call), the microseconds per column, and column ms / narrow ms against
the 1.25x bar of an opt-in schedule.  Then MAUS_Solver linear loop bodies on a tridiagonal operator at n = 262144, P = 64 on
the direct path with sparse_direct 'band' and 'narrow'.

    python tools/band_rates.py --table narrow [--out profiles/band_narrow_rates.txt]

With --table real: band solves in real arithmetic (maus_band_set_real(ctx, 1)) against the complex path of the same build, the
two alternating in one process on the same real systems -> profiles/band_real_rates.txt.  Tridiagonal, pentadiagonal and
kl = ku = 15 operators (real normal values on every diagonal, identity ordering, real shifts, b as the right-hand side) at
n = 65536, 262144 and 2^20, each alone and in a batch of 64, under the column kernel, under the narrow method and under narrow
with the split; one more row for the 5-point operator at n = 16384 (kl = 128) under the column kernel.  Per row the ms per solve
of both paths (the better of two timed calls after one warm-up call) and complex ms / real ms against the 1.25x bar of an
opt-in.  Then MAUS_Solver linear loop bodies on a real tridiagonal operator at n = 262144, P = 64 on the direct path under
narrow + split with real_direct 'off' and 'on'.

    python tools/band_rates.py --table real [--out profiles/band_real_rates.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402
from adaptive_matrix_solver_amd.band import band_order  # noqa: E402

PEAK_F64, HBM = 78.6e12, 8.0e12


def five_point(m, seed=0):
    rng = np.random.default_rng(seed)
    T = sp.diags([-1.0, 4.0, -1.0], [-1, 0, 1], shape=(m, m))
    L = (sp.kron(sp.identity(m), T) + sp.kron(sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m)), sp.identity(m))).tocsr()
    L = L.astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    p = rng.permutation(m * m)
    return L[p][:, p].tocsr()


def seven_point(m, seed=0):
    rng = np.random.default_rng(seed)
    I = sp.identity(m)
    T = sp.diags([-1.0, 6.0, -1.0], [-1, 0, 1], shape=(m, m))
    O = sp.diags([-1.0, -1.0], [-1, 1], shape=(m, m))
    L = (sp.kron(I, sp.kron(I, T)) + sp.kron(I, sp.kron(O, I)) + sp.kron(O, sp.kron(I, I))).tocsr().astype(np.complex128)
    L.data = L.data * (1.0 + 0.3j * rng.standard_normal(L.nnz))
    p = rng.permutation(m ** 3)
    return L[p][:, p].tocsr()


def five_diagonals(n, k, seed=0):
    """Offsets 0, +-1, +-k, complex normal values: kl = ku = k in the identity ordering, and partial pivoting fills the band."""
    rng = np.random.default_rng(seed)
    offs = [-k, -1, 0, 1, k]
    return sp.diags([rng.standard_normal(n - abs(o)) + 1j * rng.standard_normal(n - abs(o)) for o in offs], offs, format="csr")


def bind(ctx, A, P, identity=False):
    ctx.set_matrix_csr(A)
    perm, kl, ku = band_order(A)
    if identity:
        perm = np.arange(A.shape[0])
        kl, ku = ctx.band_prepare(perm)
    else:
        ctx.band_prepare(perm)
    ctx.pop_reserve(P)
    rng = np.random.default_rng(1)
    n = A.shape[0]
    ctx.pop_put(_cabi.POP_X, np.arange(P), rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n)))
    return kl, ku


def timed_band(ctx, count, klass="band", reps=2, warm=True):
    rng = np.random.default_rng(2)
    shift = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    psi = np.full(count, 1e-3)
    slots = np.arange(count)
    ctx.band_reserve(count)
    if warm:
        ctx.band_solve(slots, shift, psi, 0)                   # warm-up
    best = None
    for _ in range(reps):
        ctx.profile_enable(False)
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        st = ctx.band_solve(slots, shift, psi, 0)
        wall = time.perf_counter() - t0
        pr = ctx.profile_read()[klass]
        assert (st == 0).all(), st
        if best is None or pr["ms"] < best[0]["ms"]:
            best = (pr, wall)
    ctx.profile_enable(False)
    return best


def loop_rate(compat, direct="auto", bodies=3):
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    A = (five_point(256, 7) + 2.0 * sp.identity(65536)).tocsr()
    rng = np.random.default_rng(8)
    b = rng.standard_normal(65536) + 1j * rng.standard_normal(65536)
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=64, quiet=True, sparse_mode="device",
                    gmres_compat=compat, sparse_direct=direct, diag_info=diag)
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
    return steps / wall, (pr["band"]["ms"] + pr["band_blocked"]["ms"]) / bodies, pr["spmm"]["ms"] / bodies


KCLASS = {_cabi.BAND_COLUMN: "band", _cabi.BAND_BLOCKED: "band_blocked", _cabi.BAND_TILED: "band_tiled", _cabi.BAND_WIDE: "band_wide"}


def table_row(ctx, n, kl, ku, P, method, name, base_ms=None, **timing):
    """One timed row of `method` on the bound system; returns (line, ms of the batch)."""
    ctx.band_set_method(method)
    kern, nb = ctx.band_kernel_for(n, kl, ku)
    pr, wall = timed_band(ctx, P, KCLASS[kern], **timing)
    s = pr["ms"] / 1e3
    tf, tb = pr["flops"] / s / 1e12, pr["bytes"] / s / 1e12
    tc, tm = pr["flops"] / PEAK_F64, pr["bytes"] / HBM
    bound = "fp64" if tc >= tm else "HBM"
    up = "" if base_ms is None else f"{base_ms / (pr['ms'] / P):.2f}x"
    line = (f"{n:>7} {kl:>4} {ku:>4} {P:>5} {name:>8} {nb:>3} {pr['ms'] / P:>9.3f} {tf:>8.3f} {tb:>6.2f} {bound:>5} "
            f"{max(tc, tm) / s:>7.2%} {up:>8}")
    print(line, flush=True)
    return line, pr["ms"]


def main_tiled(args):
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    head = (f"{'n':>7} {'kl':>4} {'ku':>4} {'batch':>5} {'method':>8} {'nb':>3} {'ms/solve':>9} {'TFLOP/s':>8} {'TB/s':>6} {'bound':>5} "
            f"{'share':>7} {'speed-up':>8}")
    lines = [f"# band solves, csrc/band.hip, the tiled method beside the column kernel and the blocked method in one process -- "
             f"{info['name']}, {info['cus']} CUs",
             "# ms / solve from the 'band' / 'band_blocked' / 'band_tiled' profile class (HIP events around build + factor + solve of",
             "# one batch); bound = max(flops / 78.6 TFLOP/s fp64, bytes / 8 TB/s), bytes an upper end for blocked and tiled;",
             "# share = bound time / measured time",
             "",
             "# bands above kl = 1024: tiled (the better of two timed calls after one warm-up call) against the column kernel, which",
             "# runs there in every other mode (one timed call of a lone solve, no warm-up call: it takes minutes);",
             "# speed-up = column ms per solve (alone) / tiled ms per solve",
             head]
    wide = [("7-point 40^3", lambda: seven_point(40, 40), False, (1, 8))]
    wide += [(f"five diagonals k = {k}", (lambda k=k: five_diagonals(32768, k, k)), True, (1,)) for k in (2048, 4096)]
    for label, make, identity, batches in wide:
        if args.only and not any(o in label for o in args.only.split(",")):
            continue
        A = make()
        n = A.shape[0]
        kl, ku = bind(ctx, A, max(batches), identity=identity)
        lines.append(f"# {label}")
        col = None
        if not args.no_column:
            line, col = table_row(ctx, n, kl, ku, 1, _cabi.BAND_COLUMN, "column", reps=1, warm=False)
            lines.append(line)
        for P in batches:
            line, _ = table_row(ctx, n, kl, ku, P, _cabi.BAND_TILED, "tiled", base_ms=col)
            lines.append(line)
    lines += ["", "# the six rows of profiles/band_blocked_rates.txt (2-D 5-point operator), tiled beside blocked, the better of two timed",
              "# calls after one warm-up call each; speed-up = blocked ms / tiled ms (no bar: neither is a default)", head]
    cache = {}
    for item in ([] if args.only else args.sizes.split(",")):
        m, P = (int(v) for v in item.split(":"))
        n = m * m
        if m not in cache:
            A = five_point(m, m)
            cache.clear()
            cache[m] = (A, bind(ctx, A, 64))
        A, (kl, ku) = cache[m]
        line, blk = table_row(ctx, n, kl, ku, P, _cabi.BAND_BLOCKED, "blocked")
        lines.append(line)
        line, _ = table_row(ctx, n, kl, ku, P, _cabi.BAND_TILED, "tiled", base_ms=blk / P)
        lines.append(line)
    ctx.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main_wide(args):
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    head = (f"{'n':>7} {'kl':>4} {'ku':>4} {'batch':>5} {'nb':>3} {'wide ms':>10} {'tiled ms':>10} {'blocked ms':>10} {'tiled/wide':>10} "
            f"{'blocked/wide':>12} {'wide TFLOP/s':>12} {'of MFMA peak':>12}")
    lines = [f"# band solves, csrc/band.hip, the wide method beside the tiled and the blocked method in one process -- "
             f"{info['name']}, {info['cus']} CUs",
             "# ms per solve from the 'band_wide' / 'band_tiled' / 'band_blocked' profile class (HIP events around build + factor +",
             "# solve of one batch), the better of two timed calls after one warm-up call; nb = width of the inner steps (the outer",
             "# block is 64 columns); TFLOP/s = 8 n kl (kl + ku) + 8 n (2 kl + ku) executed real flops (4M: 8 per complex",
             "# multiply-add, the reach taken as full) over the wide time; peak = 78.6 TFLOP/s (fp64 MFMA)",
             head]

    def row(n, kl, ku, P):
        ms = {}
        for method, name in ((_cabi.BAND_WIDE, "wide"), (_cabi.BAND_TILED, "tiled"), (_cabi.BAND_BLOCKED, "blocked")):
            ctx.band_set_method(method)
            kern, nb = ctx.band_kernel_for(n, kl, ku)
            if kern != method:                                  # blocked above kl = 1024: the column kernel, minutes
                continue
            pr, _ = timed_band(ctx, P, KCLASS[kern])
            ms[name] = pr["ms"] / P
            if name == "wide":
                tf, inner = pr["flops"] / (pr["ms"] / 1e3) / 1e12, nb
        blk = f"{ms['blocked']:>10.3f}" if "blocked" in ms else f"{'':>10}"
        rb = f"{ms['blocked'] / ms['wide']:>11.2f}x" if "blocked" in ms else f"{'':>12}"
        line = (f"{n:>7} {kl:>4} {ku:>4} {P:>5} {inner:>3} {ms['wide']:>10.3f} {ms['tiled']:>10.3f} {blk} {ms['tiled'] / ms['wide']:>9.2f}x "
                f"{rb} {tf:>12.3f} {tf * 1e12 / PEAK_F64:>12.2%}")
        print(line, flush=True)
        lines.append(line)

    wide = [("7-point 40^3", lambda: seven_point(40, 40), False, (1, 8))]
    wide += [(f"five diagonals k = {k}", (lambda k=k: five_diagonals(32768, k, k)), True, (1,)) for k in (2048, 4096)]
    for label, make, identity, batches in wide:
        if args.only and not any(o in label for o in args.only.split(",")):
            continue
        A = make()
        kl, ku = bind(ctx, A, max(batches), identity=identity)
        lines.append(f"# {label}")
        for P in batches:
            row(A.shape[0], kl, ku, P)
    lines.append("# 2-D 5-point operator (the rows of profiles/band_blocked_rates.txt)")
    cache = {}
    for item in ([] if args.only else args.sizes.split(",")):
        m, P = (int(v) for v in item.split(":"))
        if m not in cache:
            A = five_point(m, m)
            cache.clear()
            cache[m] = (A, bind(ctx, A, 64))
        A, (kl, ku) = cache[m]
        row(m * m, kl, ku, P)
    ctx.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def diagonals(n, k, seed=0):
    """Offsets -k .. k, complex normal values: kl = ku = k in the identity ordering, and partial pivoting fills the band."""
    rng = np.random.default_rng(seed)
    offs = list(range(-k, k + 1))
    return sp.diags([rng.standard_normal(n - abs(o)) + 1j * rng.standard_normal(n - abs(o)) for o in offs], offs, format="csr")


def loop_rate_narrow(direct, n=262144, P=64, bodies=3, split="off"):
    """Candidate-steps per second and band-class ms per body of MAUS_Solver linear loop bodies on a tridiagonal operator
    (diagonal near 4 + i, off-diagonals of modulus <= 1) with every solve a band solve."""
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    rng = np.random.default_rng(8)
    off = [rng.uniform(0.2, 1.0, n - 1) * np.exp(2j * np.pi * rng.random(n - 1)) for _ in range(2)]
    A = sp.diags([off[0], 4.0 + 1j + 0.1 * rng.standard_normal(n), off[1]], [-1, 0, 1], format="csr")
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=P, quiet=True, sparse_mode="device",
                    gmres_compat="scipy-legacy", sparse_direct=direct, sparse_split=split, diag_info=diag)
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
    return steps / wall, (pr["band"]["ms"] + pr["band_split"]["ms"]) / bodies


def main_narrow(args):
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    head = (f"{'n':>8} {'kl':>3} {'ku':>3} {'batch':>5} {'column ms':>10} {'narrow ms':>10} {'column us/col':>13} {'narrow us/col':>13} "
            f"{'column/narrow':>13} {'1.25x bar':>9}")
    lines = [f"# band solves, csrc/band.hip, the narrow method against the column kernel in one process -- {info['name']}, {info['cus']} CUs",
             "# ms per solve from the 'band' profile class (HIP events around build + factor + solve of one batch), the better of two",
             "# timed calls after one warm-up call; us/col = ms per solve / n, for a batch the batch's time / (batch n); complex normal",
             "# values on every diagonal, identity ordering (the factorisation pivots and fills the band); bar: the 1.25x of an opt-in schedule",
             head]

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    shapes = [(k, n) for k in (1, 2) for n in (65536, 262144, 1 << 20)] + [(15, n) for n in (65536, 262144)]
    for k, n in shapes:
        if args.only and f"{k}:{n}" not in args.only.split(","):
            continue
        A = diagonals(n, k, k + n)
        kl, ku = bind(ctx, A, 64, identity=True)
        assert (kl, ku) == (k, k)
        for P in (1, 64):
            ms = {}
            for method, name in ((_cabi.BAND_COLUMN, "column"), (_cabi.BAND_NARROW, "narrow")):
                ctx.band_set_method(method)
                assert ctx.band_kernel_for(n, kl, ku) == (method, 1)
                pr, _ = timed_band(ctx, P, "band")
                ms[name] = pr["ms"] / P
            up = ms["column"] / ms["narrow"]
            lines.append(f"{n:>8} {kl:>3} {ku:>3} {P:>5} {ms['column']:>10.3f} {ms['narrow']:>10.3f} {ms['column'] * 1e3 / n:>13.4f} "
                         f"{ms['narrow'] * 1e3 / n:>13.4f} {up:>12.2f}x {'met' if up >= 1.25 else 'MISSED':>9}")
            print(lines[-1], flush=True)
            flush()
    ctx.close()                                                # its workspaces would crowd out the solver's own context
    if not args.only or "loop" in args.only.split(","):
        lines += ["", "# MAUS_Solver linear loop bodies on a tridiagonal operator at n = 262144, P = 64, direct path (gmres_compat='scipy-legacy':",
                  "# every solve a band solve): 1 untimed + 3 timed bodies; candidate-steps = candidates at the start of each timed body"]
        rates = {}
        for direct in ("band", "narrow"):
            rates[direct], band_ms = loop_rate_narrow(direct)
            lines.append(f"sparse_direct={direct:<7} {rates[direct]:9.1f} candidate-steps/s   (band class {band_ms:9.1f} ms per body)")
            print(lines[-1], flush=True)
        up = rates["narrow"] / rates["band"]
        lines.append(f"narrow / band: {up:.2f}x candidate-steps/s ({'meets' if up >= 1.25 else 'MISSES'} the 1.25x bar)")
        print(lines[-1], flush=True)
    flush()


def main_split(args):
    """The split beside the narrow method (the baseline) on the same systems in one process, at the rule's partition length m,
    at m / 2 and at 2 m."""
    from adaptive_matrix_solver_amd.band import split_len, split_shape
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    head = (f"{'n':>8} {'kl':>3} {'ku':>3} {'batch':>5} {'narrow ms':>10} {'m':>6} {'p':>5} {'n_red':>6} {'split m/2':>10} {'split m':>10} "
            f"{'split 2m':>10} {'TB/s at m':>9} {'of 8 TB/s':>9} {'narrow/split':>12} {'1.25x bar':>9}")
    lines = [f"# band solves, csrc/band.hip, the split (maus_band_set_split) against the narrow method in one process -- {info['name']}, {info['cus']} CUs",
             "# ms per solve from the 'band_split' / 'band' profile class (HIP events around build + local + reduced + back of one batch),",
             "# split: the better of two timed calls after one warm-up call, narrow: one timed call after one warm-up call; m = the rule's",
             "# partition length 64 ceil(sqrt(n (kl + ku)) / 64), p partitions, n_red the order of the reduced system at m; TB/s = the",
             "# split's arrays read and written once over the time at m; complex normal values on every diagonal, identity ordering;",
             "# bar: the 1.25x of an opt-in schedule, narrow ms / split ms at m",
             head]

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    shapes = [(k, n) for k in (1, 2, 15) for n in (65536, 262144, 1 << 20)]
    for k, n in shapes:
        if args.only and f"{k}:{n}" not in args.only.split(","):
            continue
        A = diagonals(n, k, k + n)
        kl, ku = bind(ctx, A, 64, identity=True)
        assert (kl, ku) == (k, k)
        m = split_len(n, kl, ku)
        p, n_red, _, _ = split_shape(n, kl, ku)
        ctx.band_set_method(_cabi.BAND_NARROW)
        for P in (1, 64):
            ctx.band_set_split(False, 0)
            nar = timed_band(ctx, P, "band", reps=1)[0]["ms"] / P
            ms = {}
            for f, mm in (("half", max(m // 2, 2 * (kl + ku) + 2)), ("rule", 0), ("twice", 2 * m)):
                ctx.band_set_split(True, mm)
                pr, _ = timed_band(ctx, P, "band_split")
                ms[f] = pr["ms"] / P
                if f == "rule":
                    tb = pr["bytes"] / (pr["ms"] / 1e3) / 1e12
            ctx.band_set_split(False, 0)
            up = nar / ms["rule"]
            lines.append(f"{n:>8} {kl:>3} {ku:>3} {P:>5} {nar:>10.3f} {m:>6} {p:>5} {n_red:>6} {ms['half']:>10.3f} {ms['rule']:>10.3f} "
                         f"{ms['twice']:>10.3f} {tb:>9.3f} {tb * 1e12 / HBM:>9.2%} {up:>11.2f}x {'met' if up >= 1.25 else 'MISSED':>9}")
            print(lines[-1], flush=True)
            flush()
    ctx.close()                                                # its workspaces would crowd out the solver's own context
    if not args.only or "loop" in args.only.split(","):
        lines += ["", "# MAUS_Solver linear loop bodies on a tridiagonal operator at n = 262144, P = 64, direct path (gmres_compat='scipy-legacy':",
                  "# every solve a band solve), sparse_direct='narrow': 1 untimed + 3 timed bodies; candidate-steps = candidates at the start",
                  "# of each timed body"]
        rates = {}
        for split in ("off", "on"):
            rates[split], band_ms = loop_rate_narrow("narrow", split=split)
            lines.append(f"sparse_split={split:<4} {rates[split]:9.1f} candidate-steps/s   (band classes {band_ms:9.1f} ms per body)")
            print(lines[-1], flush=True)
        up = rates["on"] / rates["off"]
        lines.append(f"on / off: {up:.2f}x candidate-steps/s ({'meets' if up >= 1.25 else 'MISSES'} the 1.25x bar)")
        print(lines[-1], flush=True)
    flush()


def real_diagonals(n, k, seed=0):
    """diagonals() with real normal values, stored as complex128 with imaginary parts +0.0."""
    rng = np.random.default_rng(seed)
    offs = list(range(-k, k + 1))
    return sp.diags([rng.standard_normal(n - abs(o)) + 0j for o in offs], offs, format="csr")


def timed_band_real(ctx, count, real, klass):
    """timed_band on the linear-system form (rhs_mode 1, real shifts) with the real path on or off: the better of two timed
    calls after one warm-up call, of the profile class the path counts in."""
    rng = np.random.default_rng(2)
    shift = rng.standard_normal(count) + 0j
    psi = np.full(count, 1e-3)
    slots = np.arange(count)
    ctx.band_set_real(1 if real else 0)
    assert ctx.band_real_plan(1, shift)["real"] == real
    ctx.band_reserve(count)
    ctx.band_solve(slots, shift, psi, 1)                       # warm-up
    best = None
    for _ in range(2):
        ctx.profile_enable(False)
        ctx.profile_enable(True)
        st = ctx.band_solve(slots, shift, psi, 1)
        pr = ctx.profile_read()["band_real" if real else klass]
        assert (st == 0).all(), st
        if best is None or pr["ms"] < best["ms"]:
            best = pr
    ctx.profile_enable(False)
    return best


def loop_rate_real(real_direct, n=262144, P=64, bodies=3):
    """loop_rate_narrow on a real tridiagonal operator (diagonal near 4, off-diagonals of modulus <= 1) under narrow + split."""
    import random
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    rng = np.random.default_rng(8)
    off = [rng.uniform(0.2, 1.0, n - 1) * rng.choice([-1.0, 1.0], n - 1) + 0j for _ in range(2)]
    A = sp.diags([off[0], 4.0 + 0.1 * rng.standard_normal(n) + 0j, off[1]], [-1, 0, 1], format="csr")
    b = rng.standard_normal(n) + 0j
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False,
            "is_complex_symmetric": False}
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=P, quiet=True, sparse_mode="device",
                    gmres_compat="scipy-legacy", sparse_direct="narrow", sparse_split="on", real_direct=real_direct, diag_info=diag)
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
    ctx.close()
    return steps / wall, (pr["band"]["ms"] + pr["band_split"]["ms"] + pr["band_real"]["ms"]) / bodies, pr["band_real"]["launches"]


def main_real(args):
    """The real path against the complex path, alternating in one process on the same real systems."""
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    head = (f"{'n':>8} {'kl':>3} {'ku':>3} {'batch':>5} {'schedule':>12} {'complex ms':>10} {'real ms':>10} {'complex/real':>12} "
            f"{'real TB/s':>9} {'1.25x bar':>9}")
    lines = [f"# band solves in real arithmetic (maus_band_set_real), csrc/band.hip, against the complex path of the same build, the two",
             f"# alternating in one process on the same real systems -- {info['name']}, {info['cus']} CUs",
             "# ms per solve from the 'band_real' / 'band' / 'band_split' profile class (HIP events around build + factor + solve of one",
             "# batch), the better of two timed calls after one warm-up call; real normal values on every diagonal, identity ordering,",
             "# real shifts, b as the right-hand side; real TB/s = the real path's byte count (the complex formulas at 8 B per value)",
             "# over its time; bar: the 1.25x of an opt-in, complex ms / real ms, per row",
             head]
    missed = []

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def row(n, kl, ku, P, name, method, split):
        ctx.band_set_method(method)
        ctx.band_set_split(split, 0)
        klass = "band_split" if ctx.band_real_plan(1, np.zeros(1))["split"] else "band"
        ms = {}
        for real in (False, True):
            pr = timed_band_real(ctx, P, real, klass)
            ms[real] = pr["ms"] / P
            if real:
                tb = pr["bytes"] / (pr["ms"] / 1e3) / 1e12
        up = ms[False] / ms[True]
        if up < 1.25:
            missed.append(f"{n}/{kl}/{P}/{name} {up:.2f}x")
        lines.append(f"{n:>8} {kl:>3} {ku:>3} {P:>5} {name:>12} {ms[False]:>10.3f} {ms[True]:>10.3f} {up:>11.2f}x {tb:>9.3f} "
                     f"{'met' if up >= 1.25 else 'MISSED':>9}")
        print(lines[-1], flush=True)
        flush()

    def bind_real(A, P):
        kl, ku = bind(ctx, A, P, identity=True)
        ctx.set_rhs(np.random.default_rng(4).standard_normal(A.shape[0]) + 0j)
        return kl, ku

    only = args.only.split(",") if args.only else None
    for k, n in [(k, n) for k in (1, 2, 15) for n in (65536, 262144, 1 << 20)]:
        if only and f"{k}:{n}" not in only:
            continue
        kl, ku = bind_real(real_diagonals(n, k, k + n), 64)
        assert (kl, ku) == (k, k)
        for P in (1, 64):
            for name, method, split in (("column", _cabi.BAND_COLUMN, False), ("narrow", _cabi.BAND_NARROW, False),
                                        ("narrow+split", _cabi.BAND_NARROW, True)):
                row(n, kl, ku, P, name, method, split)
    if not only or "5pt" in only:
        A = five_point(128, 7)
        A.data = A.data.real + 0j
        ctx.set_matrix_csr(A)
        perm, kl, ku = band_order(A)
        ctx.band_prepare(perm)
        ctx.pop_reserve(64)
        ctx.set_rhs(np.random.default_rng(4).standard_normal(16384) + 0j)
        for P in (1, 64):
            row(16384, kl, ku, P, "column", _cabi.BAND_COLUMN, False)
    ctx.close()                                                # its workspaces would crowd out the solver's own context
    if not only or "loop" in only:
        lines += ["", "# MAUS_Solver linear loop bodies on a real tridiagonal operator at n = 262144, P = 64, direct path (gmres_compat=",
                  "# 'scipy-legacy': every solve a band solve), sparse_direct='narrow', sparse_split='on': 1 untimed + 3 timed bodies;",
                  "# candidate-steps = candidates at the start of each timed body"]
        rates = {}
        for rd in ("off", "on"):
            rates[rd], band_ms, nreal = loop_rate_real(rd)
            lines.append(f"real_direct={rd:<4} {rates[rd]:9.1f} candidate-steps/s   (band classes {band_ms:9.1f} ms per body, {nreal} real band calls)")
            print(lines[-1], flush=True)
        up = rates["on"] / rates["off"]
        lines.append(f"on / off: {up:.2f}x candidate-steps/s ({'meets' if up >= 1.25 else 'MISSES'} the 1.25x bar)")
        print(lines[-1], flush=True)
    lines += ["", "# rows below the 1.25x bar (n/kl/batch/schedule): " + ("none" if not missed else ", ".join(missed))]
    flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=("blocked", "tiled", "wide", "narrow", "split", "real"), default="blocked")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="128:1,128:64,256:1,256:64,512:1,512:8")
    ap.add_argument("--only", default=None, help="--table tiled / wide: the wide-band rows whose label contains one of these, nothing else; "
                         "--table narrow / split / real: the rows k:n (half-bandwidth:size) and 'loop' (real: also '5pt') listed here, nothing else")
    ap.add_argument("--no-column", action="store_true", help="--table tiled: leave the column kernel's minutes out")
    ap.add_argument("--split", action="store_true", help="the split beside the narrow method (same as --table split); --only as for narrow")
    args = ap.parse_args()
    if args.split:
        args.table = "split"
    args.out = args.out or f"profiles/band_{args.table}_rates.txt"
    if args.table == "split":
        return main_split(args)
    if args.table == "tiled":
        return main_tiled(args)
    if args.table == "wide":
        return main_wide(args)
    if args.table == "narrow":
        return main_narrow(args)
    if args.table == "real":
        return main_real(args)
    ctx = _cabi.Context(0)
    info = ctx.device_info()
    lines = [f"# band solves, csrc/band.hip, column kernel and blocked method in one process -- {info['name']}, {info['cus']} CUs",
             "# ms / solve from the 'band' / 'band_blocked' profile class (HIP events around build + factor + solve of one batch),",
             "# the better of two timed calls after one warm-up call; bound = max(flops / 78.6 TFLOP/s fp64, bytes / 8 TB/s);",
             "# share = bound time / measured time; speed-up = column ms / blocked ms",
             f"{'n':>7} {'kl':>4} {'ku':>4} {'batch':>5} {'method':>8} {'nb':>3} {'ms/solve':>9} {'TFLOP/s':>8} {'TB/s':>6} {'bound':>5} "
             f"{'share':>7} {'speed-up':>8}"]
    cache = {}
    for item in args.sizes.split(","):
        m, P = (int(v) for v in item.split(":"))
        n = m * m
        if m not in cache:
            A = five_point(m, m)
            cache.clear()
            cache[m] = (A, bind(ctx, A, 64))
        A, (kl, ku) = cache[m]
        col_ms = None
        for method, name in ((_cabi.BAND_COLUMN, "column"), (_cabi.BAND_BLOCKED, "blocked")):
            ctx.band_set_method(method)
            kern, nb = ctx.band_kernel_for(n, kl, ku)
            pr, wall = timed_band(ctx, P, "band_blocked" if kern == _cabi.BAND_BLOCKED else "band")
            s = pr["ms"] / 1e3
            tf, tb = pr["flops"] / s / 1e12, pr["bytes"] / s / 1e12
            tc, tm = pr["flops"] / PEAK_F64, pr["bytes"] / HBM
            bound = "fp64" if tc >= tm else "HBM"
            up = "" if col_ms is None else f"{col_ms / pr['ms']:.2f}x"
            col_ms = pr["ms"] if col_ms is None else col_ms
            lines.append(f"{n:>7} {kl:>4} {ku:>4} {P:>5} {name:>8} {nb:>3} {pr['ms'] / P:>9.3f} {tf:>8.3f} {tb:>6.2f} {bound:>5} "
                         f"{max(tc, tm) / s:>7.2%} {up:>8}")
            print(lines[-1], flush=True)
    # band against dense at n = 16384: the same 64 shifted systems
    m, P = 128, 64
    A = five_point(m, 3)
    n = m * m
    bind(ctx, A, P)
    rng = np.random.default_rng(4)
    shift = rng.standard_normal(P) + 1j * rng.standard_normal(P)
    psi = np.full(P, 1e-3)
    slots = np.arange(P)
    tb, Wb = {}, {}
    for method, name in ((_cabi.BAND_COLUMN, "column"), (_cabi.BAND_BLOCKED, "blocked")):
        ctx.band_set_method(method)
        ctx.band_reserve(P)
        ctx.band_solve(slots, shift, psi, 0)
        t0 = time.perf_counter(); ctx.band_solve(slots, shift, psi, 0); tb[name] = time.perf_counter() - t0
        Wb[name] = ctx.pop_get(_cabi.POP_W, slots, n)
    ctx.lu_reserve(n, P)
    t0 = time.perf_counter(); ctx.shifted_lu_solve(slots, shift, psi, 0); td = time.perf_counter() - t0
    Wd = ctx.pop_get(_cabi.POP_W, slots, n)
    lines += ["", "# band vs dense (densified H_k, maus_shifted_lu_solve) at n = 16384, 64 shifted 5-point systems, wall clock per call"]
    for name in ("column", "blocked"):
        rel = max(np.linalg.norm(Wb[name][k] - Wd[k]) / np.linalg.norm(Wd[k]) for k in range(P))
        lines.append(f"band {name:<8} {tb[name] * 1e3 / P:9.3f} ms/solve, {td / tb[name]:6.1f}x the dense path, largest relative difference "
                     f"of the solutions {rel:.2e}")
    lines.append(f"dense         {td * 1e3 / P:9.3f} ms/solve")
    print("\n".join(lines[-4:]), flush=True)
    ctx.close()                                                # its workspaces would crowd out the solver's own context
    lines += ["", "# MAUS_Solver linear loop bodies at n = 65536, P = 64 (5-point + 2 I, GMRES preferred): 1 untimed + 3 timed bodies;",
              "# candidate-steps = candidates in the population at the start of each timed body"]
    for compat, direct, path in (("scipy-legacy", "band", "direct (column)"), ("scipy-legacy", "blocked", "direct (blocked)"),
                                 ("rtol", "auto", "GMRES")):
        rate, band_ms, spmm_ms = loop_rate(compat, direct)
        lines.append(f"{path:<16} {rate:9.1f} candidate-steps/s   (band classes {band_ms:8.1f} ms, spmm class {spmm_ms:8.1f} ms per body)")
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
