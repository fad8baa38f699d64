"""Rates of the device Lanczos of the sparse Hermitian shortcut (DESIGN §10 "Lanczos").

    python tools/lanczos_rates.py [--out profiles/lanczos_rates.txt] [--small]

For the two largest test operators (tests/lanczos_cases.py: the complex 1024 x 1000 lattice and the tridiagonal matrix of
order 2^20): restarts, products and wall time of one run to tol = 1e-10, and -- from a second run under the library's HIP-event
profile -- the time and the algorithmic bytes of the "lanczos" class (reorthogonalisation: about 4 (j + 1) 16 n bytes per step;
the restart and the final combination with theirs) against the 6.29 TB/s copy rate of DESIGN §10, and the "spmm" class beside it.
These are algorithmic bytes over time, not HBM traffic: part of a basis of a few hundred MB is served from the Infinity Cache.
Then the time of one match of 16 candidates against the resident rows (maus_herm_match_rows).
--small adds the 64 x 50 lattice with its eigenvalues beside SciPy's eigsh (a quick check of a new build)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from adaptive_matrix_solver_amd import Context  # noqa: E402
from adaptive_matrix_solver_amd.engine import eigsh_parameters, thick_restart_lanczos  # noqa: E402
import lanczos_cases  # noqa: E402

COPY_TBS = 6.29
EPS = np.finfo(np.float64).eps


def run(ctx, A, tol=1e-10):
    n = A.shape[0]
    k, ncv = eigsh_parameters(n)
    anorm = float(abs(A).sum(axis=0).max())
    t0 = time.perf_counter()
    r = thick_restart_lanczos(ctx, n, k, ncv, tol, EPS * anorm, 10 * n, lanczos_cases.start_vector(n) + 0j, lambda: 1 / 0)
    return r, time.perf_counter() - t0, anorm


def rates(name, A, out, check=False):
    n = A.shape[0]
    ctx = Context(0)
    try:
        ctx.set_matrix_csr(A)
        r, wall, anorm = run(ctx, A)
        R = ctx.get_ritz_rows()
        resid = max(np.linalg.norm(A @ R[q] - r["theta"][q] * R[q]) / abs(r["theta"][q]) for q in range(R.shape[0]))
        ctx.profile_enable(True)
        r2, wall2, _ = run(ctx, A)
        pr = ctx.profile_read()
        ctx.profile_enable(False)
        assert np.array_equal(r["theta"], r2["theta"]) and np.array_equal(R, ctx.get_ritz_rows()), "two runs differ"
        lz, sm = pr["lanczos"], pr["spmm"]
        tbs = lz["bytes"] / (lz["ms"] * 1e-3) / 1e12
        print(f"{name}: n = {n}, nnz = {A.nnz}, converged = {r['converged']}, restarts = {r['restarts']}, products = {r['products']}, "
              f"wall = {wall:.3f} s (profiled run {wall2:.3f} s), largest ||A y - theta y|| / |theta| = {resid:.2e}", file=out)
        print(f"    lanczos class: {lz['launches']} brackets, {lz['ms']:.2f} ms, {lz['bytes'] / 1e9:.2f} GB, {tbs:.2f} TB/s = "
              f"{tbs / COPY_TBS:.2f} of the {COPY_TBS} TB/s copy rate; spmm class: {sm['launches']} launches, {sm['ms']:.2f} ms, "
              f"{sm['bytes'] / (sm['ms'] * 1e-3) / 1e12 if sm['ms'] else 0.0:.2f} TB/s", file=out)
        print(f"    theta = {np.array2string(r['theta'], precision=12)}", file=out)
        # the match of AMS:197-202 against the resident rows, paid by every step of the population: P = 16 candidates
        P = 16
        ctx.pop_reserve(P)
        rng = np.random.default_rng(5)
        X = rng.standard_normal((P, n)) + 1j * rng.standard_normal((P, n))
        ts = []
        for _ in range(4):
            ctx.pop_put(0, list(range(P)), X)
            ctx.profile_enable(True)
            ctx.herm_match_rows(list(range(P)))
            m = ctx.profile_read()["lanczos"]
            ctx.profile_enable(False)
            ts.append((m["ms"], m["bytes"]))
        ms, nb = sorted(ts)[len(ts) // 2]
        print(f"    match of {P} candidates against the {R.shape[0]} rows: {ms:.3f} ms (median of 4, after a warm-up), {nb / 1e9:.2f} GB "
              f"algorithmic, {nb / (ms * 1e-3) / 1e12:.2f} TB/s", file=out)
        if check:
            import scipy.sparse.linalg as spla
            w = np.sort(spla.eigsh(A, k=6, which="LM", v0=lanczos_cases.start_vector(n), tol=1e-10)[0])
            print(f"    eigsh = {np.array2string(w, precision=12)}, largest difference {np.abs(w - r['theta']).max():.2e}", file=out)
        out.flush()
    finally:
        ctx.close()


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "lanczos_rates.txt")
    with open(path, "w") as out:
        print("# device thick-restart Lanczos, k = 6, ncv = 20, tol = 1e-10 (tools/lanczos_rates.py)", file=out)
        if "--small" in sys.argv:
            rates("lattice 64 x 50", lanczos_cases.lattice(64, 50), out, check=True)
        rates("lattice 1024 x 1000", lanczos_cases.lattice(1024, 1000), out)
        rates("tridiagonal 2^20", lanczos_cases.tridiagonal(1 << 20), out)
    print(open(path).read())
