"""bench.py --dump-outputs on CPU: the files hold what a caller of MAUS_Solver reads back from the population after the
last loop body (device phases replaced by the NumPy test double tests/fake_ctx.py), all float64 and finite, and a
population whose vectors exceed the budget is written as a fixed seeded sample of rows."""
import os
import random
import sys

import numpy as np

import scenarios
from fake_ctx import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _solver(name, iters=3):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    spec = scenarios.TRAJECTORIES[name]
    A, b = scenarios.build(spec)
    np.random.seed(spec["seed"]); random.seed(spec["seed"]); SolutionCandidate._candidate_id_counter = 0
    PT = {"eig": ProblemType.EIGENVALUE, "lin": ProblemType.SOLVE_LINEAR_SYSTEM, "svd": ProblemType.SVD}[spec["kind"]]
    eng = DeviceEngine(ctx=FakeContext(), pert_mode="uniform", gmres_compat="scipy-legacy")
    s = MAUS_Solver(A, PT, b_vector=b, initial_num_candidates=spec["P"], global_convergence_tol=spec["tol"], quiet=True,
                    engine=eng)
    for it in range(iters):
        s.loop_body(it + 1)
    return s


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_holds_what_a_caller_reads(tmp_path):
    s = _solver("eig64")
    bench.dump_outputs(s, str(tmp_path))
    got = _load(str(tmp_path))
    assert set(got) == {"candidate_id", "state", "lambda", "residual", "vector_rows", "v"}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    # every evaluated candidate, in list order; the ones spawned by the last body (residual_k = inf) are left out
    evaluated = [c for c in s.candidates if np.isfinite(c.residual_k)]
    assert 0 < len(evaluated) < len(s.candidates)
    P = len(evaluated)
    assert got["v"].shape == (P, 64, 2) and np.array_equal(got["vector_rows"], np.arange(P))
    for k, c in enumerate(evaluated):
        assert got["candidate_id"][k] == c.id and got["state"][k] == c.state.value
        assert complex(*got["lambda"][k]) == complex(c.lambda_k)
        assert got["residual"][k] == float(c.residual_k)
        assert np.array_equal(got["v"][k, :, 0] + 1j * got["v"][k, :, 1], c.v_k)


def test_dump_of_svd_and_linear_populations(tmp_path):
    for name, vecs in (("svd5x4", {"u": 5, "right_v": 4}), ("lin24", {"x": 24})):
        s = _solver(name)
        d = str(tmp_path / name)
        bench.dump_outputs(s, d)
        got = _load(d)
        P = sum(np.isfinite(c.residual_k) for c in s.candidates)
        assert all(np.isfinite(a).all() for a in got.values())
        for v, width in vecs.items():
            assert got[v].shape == (P, width, 2)
        assert ("sigma" in got) == (name == "svd5x4")


def test_dump_over_budget_writes_a_seeded_sample(tmp_path, monkeypatch):
    s = _solver("eig64")
    evaluated = [c for c in s.candidates if np.isfinite(c.residual_k)]
    P = len(evaluated)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 10 * 64 * 16 + 4 * 8 * P)
    bench.dump_outputs(s, str(tmp_path / "a"))
    bench.dump_outputs(s, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    rows = a["vector_rows"].astype(int)
    assert 0 < len(rows) < P and np.array_equal(rows, np.unique(rows))
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for j, k in enumerate(rows):
        assert np.array_equal(a["v"][j, :, 0] + 1j * a["v"][j, :, 1], evaluated[k].v_k)
