"""Case table of the wide GMRES step (sparse_gmres="wide", maus_gmres_set_method(ctx, 1), csrc/gmres.hip):
tests/test_gmres_wide_host.py on the CPU, tests/test_gpu_gmres_wide.py on the device.

The wide step splits n over workgroups of 512 entries and joins the per-piece partial sums with 256 threads, each of which adds
pieces t, t + 256, ...: the sizes below lie on both sides of one piece (512) and of the second level of the join (512 x 256 =
131072).  Operators, right-hand sides, the traced reference and the checkers are those of tests/gmres_cases.py; the phase s
of banded() follows that table's rule -- 1, except where that puts a decision within 0.02 of its threshold, then the first s
that does not."""
import functools

import gmres_cases as gc

PIECE = 512                       # GW_SPAN of csrc/gmres.hip
JOIN = 256                        # threads that join the partial sums
WIDE_SIZES = (PIECE - 1, PIECE, PIECE + 1, PIECE * JOIN - 1, PIECE * JOIN, PIECE * JOIN + 1)
WIDE_WEIGHTS = (1.0, 2.2)
WIDE_SEED = {(511, 1, 0): 2, (512, 1, 0): 2}


def _wide_cases():
    out = []
    for n in WIDE_SIZES:
        for wi, wt in enumerate(WIDE_WEIGHTS):
            for jac in (0, 1):
                s = WIDE_SEED.get((n, wi, jac), 1)
                out.append(gc._case(f"wide_n{n}_w{wi}_j{jac}", lambda n=n, s=s, wt=wt: gc._one(gc.banded(n, s, wt), gc.crand(n, n), True),
                                    jacobi=jac))
    return out


CASES = _wide_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES) == 24


@functools.lru_cache(maxsize=None)
def reference(name):
    """[(x, info, inner, cycles, closest)] of the case's one candidate from gc.traced(); computed once per process."""
    case = BY_NAME[name]
    return [gc.traced(H, b, b, inv, rtol=case["rtol"], maxiter=case["maxiter"], restart=case["restart"]) for H, b, inv in gc.systems(case)]


def check_case(case, got):
    """gc.check_case for a case of this table: every candidate through gc.check_rounded against reference()."""
    X, info, inner, status = got
    ref = reference(case["name"])
    for i, (H, b, inv) in enumerate(gc.systems(case)):
        gc.check_rounded((X[i], info[i], inner[i], status[i]), ref[i], H, b, case["rtol"], f"{case['name']}[{i}]")
