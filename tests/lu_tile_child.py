"""Child process of tests/test_gpu_lu_tile.py: solves every case of lu_tile_cases() through a fresh Context under the
MAUS_LU_TILE of its environment (the library reads the switch once per process) and writes, per case, status, ipiv and x
beside the planted ones, and the trailing-update launches of the case from the library's MAUS_LU_TRACE log.

    python lu_tile_child.py <out.npz>
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import lu_cases as lc  # noqa: E402


def lu_tile_cases():
    """name -> (MAUS_LU_NBO or None, batch builder).  The sizes are the smallest at which the first trailing update
    (M = npad - nbo, N = M + 32, K = nbo) is ragged against the 128 x 64 tile, at or above the 1536 rows from which the
    64 x 64 tile it is compared with is used, with later updates on both sides of the 128 x 64 tile's own 1024."""
    fam = lc._family(2080)

    def table(n, G, seed):
        return lambda: lc.case_batch(lc._case(f"tile_n{n}", n, G, ("default",), [], seed))

    def family(name):
        return lambda: tuple(a[None] for a in lc.system(2080, lc.family_seed(2080, name), **fam[name])[:4])

    return {
        "n2080_g2": (None, table(2080, 2, 2080)),            # 1568 x 1600 x 512: a quarter tile ragged in M, then 1056 x 1088
        "n2080_nbo64": (64, table(2080, 1, 2081)),           # K = 64: eight K-steps
        "n2080_nbo96": (96, table(2080, 1, 2082)),           # K = 96: twelve K-steps, M from 1984 down across 1536 and 1024
        "n2112_g3": (None, table(2112, 3, 2112)),            # 1600 x 1632 x 512: ragged against 128 both ways
        "n2080_piv_reverse": (None, family("piv_reverse")),  # A and C rows truly permuted
        "n2080_piv_random": (None, family("piv_random")),
    }


def gaussian_batch():
    return lc.gaussian(2080, 5000 + 2080, 2)


def main(out):
    from adaptive_matrix_solver_amd import Context
    trace_path = os.environ["MAUS_LU_TRACE"]
    ctx = Context(0)
    res = {}

    def trace_lines():
        if not os.path.exists(trace_path):
            return []
        with open(trace_path) as f:
            return [tuple(int(v) for v in ln.split()) for ln in f if ln.strip()]

    seen = len(trace_lines())
    for name, (nbo, build) in lu_tile_cases().items():
        if nbo:
            os.environ["MAUS_LU_NBO"] = str(nbo)
        else:
            os.environ.pop("MAUS_LU_NBO", None)
        A, b, x, ipiv = build()
        xg, status, pg = ctx.lu_solve(A, b, want_ipiv=True)
        lines = trace_lines()
        res[f"{name}/x"], res[f"{name}/ipiv"], res[f"{name}/status"] = xg, pg, status
        res[f"{name}/x_planted"], res[f"{name}/ipiv_planted"] = x, ipiv
        res[f"{name}/launches"] = np.array(lines[seen:], dtype=np.int64).reshape(-1, 4)
        seen = len(lines)
    os.environ.pop("MAUS_LU_NBO", None)
    A, b = gaussian_batch()
    xg, status, pg = ctx.lu_solve(A, b, want_ipiv=True)
    res["gaussian/x"], res["gaussian/ipiv"], res["gaussian/status"] = xg, pg, status
    res["mw_aborts"] = np.array(ctx.lu_mw_aborts())
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
