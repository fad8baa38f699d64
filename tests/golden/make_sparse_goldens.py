#!/usr/bin/env python3
"""Generate tests/golden/sparse_*.json by importing the REFERENCE unmodified (sparse scenarios, sparse_scenarios.py).

Same harness as make_goldens.py (its loader, GMRES shim, row and record format); runs only where the reference is
present.  One fixture per scenario and gmres_compat mode: 'rtol' through the tol->rtol shim, 'scipy-legacy' unshimmed.  A fixture
holds digests (snapshot.py) per loop body; rows in full only where a tolerance check needs them (eigsh scenarios).

Usage:  python tests/golden/make_sparse_goldens.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
import snapshot  # noqa: E402
import sparse_scenarios  # noqa: E402


def run_sparse(mod, name, spec, mode):
    A, b = sparse_scenarios.build(name)
    real, shim = mg.gmres_shim(mod)
    if mode == "rtol":
        mod.spla = shim
    try:
        mg.seed_all(mod, spec["seed"])
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            solver = mod.MAUS_Solver(A, mg.ptype(mod, spec["kind"]), b_vector=b, initial_num_candidates=spec["P"],
                                     global_convergence_tol=spec["tol"])
        S = mod.SolutionCandidate.State
        pk = solver.problem_knowledge
        out = {"name": name, "mode": mode, "spec": {k: v for k, v in spec.items() if k != "modes"}, "versions": mg.versions(),
               "matrix_type": pk["matrix_type"], "M_format": type(solver.M).__name__, "M_dtype": str(solver.M.dtype),
               "cond": float(solver.cond_number).hex(), "hermitian": bool(pk["is_hermitian"]),
               "init": {"digest": snapshot.digest_rows(mg.rows_of(mod, solver.candidates, spec["kind"])),
                        "rng": snapshot.rng_digest(),
                        "globals": snapshot.globals_record(solver.landscape_energy, solver.avg_residual, solver.avg_stuckness, 0,
                                                           pk["numerical_stability_state"], pk["local_solver_preference"],
                                                           solver.strat_params)},
               "iters": []}
        for it in range(spec["iters"]):
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                solver._update_global_diagnostics(it + 1)
                solver._adjust_global_strategy(it + 1)
                steps = 0
                for c in solver.candidates:
                    if c.state not in (S.CONVERGED, S.RETIRED):
                        c.update_solution_step(solver.M, solver.b, solver.strat_params, solver.problem_knowledge)
                        steps += 1
                stepped = mg.rows_of(mod, solver.candidates, spec["kind"])
                solver._manage_candidates(it + 1)
            rows = mg.rows_of(mod, solver.candidates, spec["kind"])
            out["iters"].append({
                "steps": steps, "n_after": len(rows), "printed": log.getvalue().count("\n"),
                "digest_stepped": snapshot.digest_rows(stepped), "digest": snapshot.digest_rows(rows),
                "rng": snapshot.rng_digest(),
                "globals": snapshot.globals_record(solver.landscape_energy, solver.avg_residual, solver.avg_stuckness,
                                                   solver.num_distinct_converged_solutions, pk["numerical_stability_state"],
                                                   pk["local_solver_preference"], solver.strat_params),
                "next_id": int(mod.SolutionCandidate._candidate_id_counter)})
            if spec.get("arpack") and it == 0:           # eigsh vs one eigh per matrix: compared within tolerance
                out["iters"][-1]["rows"] = snapshot.full_rows(stepped, limit=48)
        return out
    finally:
        mod.spla = real


def main():
    mod = mg.load_reference()
    for name, spec in sparse_scenarios.SPARSE_TRAJECTORIES.items():
        for mode in spec["modes"]:
            rec = run_sparse(mod, name, spec, mode)
            fn = os.path.join(HERE, f"sparse_{name}_{mode.replace('-', '_')}.json")
            with open(fn, "w") as f:
                json.dump(rec, f, separators=(",", ":"))
            print(name, mode, "steps", [r["steps"] for r in rec["iters"]], os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
