"""Candidate vectors drawn on the host against drawn on the device (vector_draws, csrc/mtdev.hip: pop_draw_kernel) on one
MI355X, alternating in one process -> profiles/pop_draw_rates.txt.

1. ms per bracket for N in {4096, 65536, 262144, 2^20} x draws in {1, 15, 64}.  A bracket is what end_deferred_push does for the
   new candidates of one loop body.  host: per draw normalise(np.random.rand(N) + 1j*np.random.rand(N)), then one pop_put of
   the stacked rows.  device: DeviceEngine.draw_vectors with every draw MAUS_DRAW_UNIT -- the plan, the uploads, the jump
   launches, the draw and join kernels, the read-back of the norms and the jump of the host stream.  Host clock around work
   that ends in a device synchronise (both calls synchronise before they return).  The first device call of a shape builds
   its jump polynomials and is recorded on its own; warm = mean over a window of at least 0.3 s (at least 3 calls) after it,
   host and device alternating.  Bar: host / device >= 1.25.
2. The sub-stream count: warm ms per device bracket at the rule's S, half and double (forced).
3. Candidate-steps/s of MAUS_Solver linear loop bodies on a tridiagonal operator at n = 262144, P = 64, sparse_direct='narrow',
   sparse_split='on', gmres_compat='scipy-legacy', vector_draws 'host' against 'device': two solvers in one process, one untimed
   body each, then 3 timed bodies each, alternating body by body.
4. Observed errors of the UNIT rows and norms against the host's, in units of 2^-53.
5. The device bracket alone at N = 65536, 64 draws -- no host bracket between the calls -- split into the maus_pop_draw call and
   the jump of the host stream.

    python tools/draw_rates.py [--out profiles/pop_draw_rates.txt] [--quick]
"""
import argparse
import math
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402
from adaptive_matrix_solver_amd.engine import DeviceEngine  # noqa: E402

BAR, WINDOW = 1.25, 0.3
UNIT = _cabi.DRAW_UNIT

RESOURCES = """# kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup:
#   pop_draw_kernel        36 VGPR   0 AGPR   78 SGPR   0 B scratch   14976 B LDS   occupancy 8 waves/SIMD
#   pop_draw_join_kernel   14 VGPR   0 AGPR   28 SGPR   0 B scratch       0 B LDS   occupancy 8 waves/SIMD
#   unchanged: mt_jump_kernel 63 VGPR, 44992 B LDS, 0 scratch; build_h_mt4_kernel 70 VGPR, 14976 B LDS, 0 scratch;
#   mt_copy_state_kernel 10 VGPR, 0 scratch"""


def host_bracket(ctx, n, draws):
    rows = []
    for _ in range(draws):
        v = (np.random.rand(n) + 1j * np.random.rand(n)).astype(np.complex128)
        rows.append(v / np.linalg.norm(v))
    ctx.pop_put(0, np.arange(draws), np.stack(rows))


def device_bracket(eng, n, draws, substreams=0):
    eng.draw_vectors(n, np.arange(draws), np.full(draws, UNIT, dtype=np.int32), substreams=substreams)


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def window(fs):
    """Mean ms per call of each function of fs, the functions alternating, until every one has run for WINDOW seconds."""
    tot, cnt = [0.0] * len(fs), 0
    while cnt < 3 or min(tot) < WINDOW * 1e3:
        for i, f in enumerate(fs):
            tot[i] += timed(f)
        cnt += 1
        if cnt >= 200:
            break
    return [t / cnt for t in tot]


def solver(n, P, mode):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    rng = np.random.default_rng(8)
    off = [rng.uniform(0.2, 1.0, n - 1) * np.exp(2j * np.pi * rng.random(n - 1)) for _ in range(2)]
    A = sp.diags([off[0], 4.0 + 1j + 0.1 * rng.standard_normal(n), off[1]], [-1, 0, 1], format="csr")
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    np.random.seed(3); random.seed(3); SolutionCandidate._candidate_id_counter = 0
    diag = {"is_sparse_init": True, "condition_number": 1e7, "is_singular": False, "is_hermitian": False, "is_complex_symmetric": False}
    t0 = time.perf_counter()
    s = MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=P, quiet=True, sparse_mode="device",
                    gmres_compat="scipy-legacy", sparse_direct="narrow", sparse_split="on", diag_info=diag, vector_draws=mode)
    s.engine.ctx.sync()
    return s, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pop_draw_rates.txt"))
    ap.add_argument("--quick", action="store_true", help="N up to 65536 and a loop at n = 16384 (rehearsal)")
    args = ap.parse_args()
    ctx = _cabi.Context(0)
    name = ctx.device_info()["name"]
    lines = [f"# tools/draw_rates.py on {name}; ms are host-clock times of calls that end in a device synchronise", RESOURCES, ""]

    def flush():
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    sizes = (4096, 65536) if args.quick else (4096, 65536, 262144, 1 << 20)
    lines += ["# 1. ms per bracket, host (draw + normalise + one upload) against device (maus_pop_draw + the host stream jump)",
              f"{'N':>8} {'draws':>5} {'S':>3} {'host ms':>10} {'device first':>13} {'device warm':>12} {'host/device':>12}  bar {BAR}"]
    sweep = []
    eng = DeviceEngine(ctx=ctx)
    for n in sizes:
        ctx.set_matrix_csr(sp.identity(n, format="csr", dtype=np.complex128))
        ctx.pop_reserve(64)
        for draws in (1, 15, 64):
            np.random.seed(5)
            S = _cabi.pop_draw_plan(n, np.arange(draws), 624)["S"]
            host_bracket(ctx, n, draws)                                   # warm-up of the host side
            first = timed(lambda: device_bracket(eng, n, draws))
            h, d = window([lambda: host_bracket(ctx, n, draws), lambda: device_bracket(eng, n, draws)])
            verdict = "meets" if h / d >= BAR else "MISSES"
            lines.append(f"{n:8d} {draws:5d} {S:3d} {h:10.3f} {first:13.3f} {d:12.3f} {h / d:12.2f}  {verdict}")
            print(lines[-1], flush=True)
            flush()
            if n >= 65536 and draws in (1, 15):
                sweep.append((n, draws, S))
    lines += ["", "# 2. the sub-stream count: warm ms per device bracket at the rule's S, half and double (forced; S = 1 has no half)",
              f"{'N':>8} {'draws':>5} {'S rule':>7} {'ms rule':>9} {'S/2':>4} {'ms':>9} {'2S':>4} {'ms':>9}"]
    for n, draws, S in sweep:
        ctx.set_matrix_csr(sp.identity(n, format="csr", dtype=np.complex128))
        ctx.pop_reserve(64)
        half, dbl = max(1, S // 2), min(64, 2 * S)
        for s_ in (S, half, dbl):
            device_bracket(eng, n, draws, s_)
        r, a, b = window([lambda: device_bracket(eng, n, draws, S), lambda: device_bracket(eng, n, draws, half),
                          lambda: device_bracket(eng, n, draws, dbl)])
        lines.append(f"{n:8d} {draws:5d} {S:7d} {r:9.3f} {half:4d} {a:9.3f} {dbl:4d} {b:9.3f}")
        print(lines[-1], flush=True)
        flush()

    lines += ["", "# 4. observed errors of MAUS_DRAW_UNIT against the host's v / np.linalg.norm(v), units of 2^-53 (bounds: 2N + 8 per",
              "#    component, N + 2 for the norm against sqrt(math.fsum))"]
    for n in sizes:
        ctx.set_matrix_csr(sp.identity(n, format="csr", dtype=np.complex128))
        ctx.pop_reserve(8)
        np.random.seed(11)
        st = np.random.get_state()
        host = [np.random.rand(n) + 1j * np.random.rand(n) for _ in range(3)]
        norms = ctx.pop_draw(0, n, [0, 1, 2], [UNIT] * 3, None, st, [0, 1, 2])
        X = ctx.pop_get(0, [0, 1, 2], n)
        ce = ne = 0.0
        for k in range(3):
            ref = host[k] / np.linalg.norm(host[k])
            ce = max(ce, np.max(np.abs(X[k].real - ref.real) / ref.real), np.max(np.abs(X[k].imag - ref.imag) / ref.imag))
            fs = math.sqrt(math.fsum((host[k].real ** 2).tolist() + (host[k].imag ** 2).tolist()))
            ne = max(ne, abs(norms[k] - fs) / fs)
        lines.append(f"{n:8d}  component {ce * 2.0 ** 53:8.2f} (bound {2 * n + 8})   norm {ne * 2.0 ** 53:6.2f} (bound {n + 2})")
        print(lines[-1], flush=True)
    from adaptive_matrix_solver_amd.engine import _advance_numpy_stream
    n, draws = 65536, 64
    ctx.set_matrix_csr(sp.identity(n, format="csr", dtype=np.complex128))
    ctx.pop_reserve(64)
    kinds = np.full(draws, UNIT, dtype=np.int32)
    st = np.random.get_state()
    call = lambda: ctx.pop_draw(0, n, np.arange(draws), kinds, None, st, np.arange(draws))
    jump = lambda: _advance_numpy_stream(4 * n * draws)
    call(); jump(); jump()
    c_ms, j_ms = window([call, jump])
    lines += ["", "# 5. the device bracket alone (no host bracket between the calls), warm",
              f"{n:8d} {draws:5d}   maus_pop_draw {c_ms:7.3f} ms   host stream jump {j_ms:7.3f} ms   together {c_ms + j_ms:7.3f} ms"]
    print(lines[-1], flush=True)
    flush()
    ctx.close()                                                           # its population would crowd out the solvers' own

    n, P = (16384, 64) if args.quick else (262144, 64)
    lines += ["", f"# 3. MAUS_Solver linear loop bodies, tridiagonal operator, n = {n}, P = {P}, sparse_direct='narrow', sparse_split='on',",
              "#    gmres_compat='scipy-legacy': construction (the initial population's draws), 1 untimed + 3 timed bodies per mode,",
              "#    alternating body by body; candidate-steps = candidates at the start of each timed body"]
    runs = {}
    for mode in ("host", "device"):
        s, ms = solver(n, P, mode)
        s.loop_body(1)
        s.engine.ctx.sync()
        runs[mode] = {"s": s, "init_ms": ms, "steps": 0, "wall": 0.0}
    for it in range(3):
        for mode in ("host", "device"):
            r = runs[mode]
            s = r["s"]
            before = len(s.candidates)
            r["steps"] += before
            t0 = time.perf_counter()
            s.loop_body(it + 2)
            s.engine.ctx.sync()
            r["wall"] += time.perf_counter() - t0
            r["born"] = sum(1 for c in s.candidates if c.id >= P)
    for mode in ("host", "device"):
        r = runs[mode]
        r["rate"] = r["steps"] / r["wall"]
        lines.append(f"vector_draws={mode:<7} construction {r['init_ms']:9.1f} ms   {r['steps']:4d} candidate-steps in {r['wall'] * 1e3:8.1f} ms "
                     f"= {r['rate']:8.1f} candidate-steps/s   ({r['wall'] * 1e3 / 3:7.1f} ms per body, {r['born']} candidates born in the timed bodies and the untimed one)")
    ratio = runs["device"]["rate"] / runs["host"]["rate"]
    lines.append(f"device / host = {ratio:.2f}   bar {BAR}: {'meets' if ratio >= BAR else 'MISSES'}      "
                 f"construction host / device = {runs['host']['init_ms'] / runs['device']['init_ms']:.2f}")
    print("\n".join(lines[-3:]), flush=True)
    flush()


if __name__ == "__main__":
    main()
