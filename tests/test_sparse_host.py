"""Sparse problem matrices (sparse_mode='device'): the host logic on CPU.

The device phases are replaced by FakeSparseContext, a test double that keeps the scipy.sparse matrix and answers with the
reference's own sparse calls (AMS:44-90): A @ v on the sparse matrix, spsolve of H = A - lam I + psi I, SciPy's GMRES with the
Jacobi preconditioner of AMS:67-72, and the k eigenpairs of largest |lambda| for the Hermitian shortcut.  Checked here: the
keyword and its default, the reference's diagnosis branches (AMS:374-404), the conversion of AMS:357-358, the strategy the
reference derives for a sparse problem, and that a sparse solve draws nothing from the NumPy stream (AMS:46-47)."""
import random

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from fake_ctx import FakeContext, check_restart


class FakeSparseContext(FakeContext):
    """FakeContext plus the CSR entry points of _cabi.Context, with the reference's sparse SciPy calls."""

    def set_matrix(self, A):
        self.sparse = None
        super().set_matrix(A)

    def set_matrix_csr(self, A):
        if A.shape != (self.rows, self.cols):
            self.pop = {}
            self.cap = 0
        self.A = A                      # the sparse matrix itself: every `self.A @ v` of FakeContext is the sparse product
        self.sparse = "rows"
        self.rows, self.cols = A.shape

    def matrix_is_sparse(self):
        return getattr(self, "sparse", None)

    def lu_max_n(self):
        return 16384

    def _h(self, k, shift, psi, rhs_mode):
        n = self.rows
        target = self.A - shift[k] * sp.eye(n, dtype=self.A.dtype) if rhs_mode == 0 else self.A      # AMS:270
        return target + sp.identity(n, dtype=target.dtype, format="csc") * np.complex128(psi[k])    # AMS:46-47, 55

    def shifted_lu_solve(self, slots, shift, psi, rhs_mode=0, pert_mode=0, pert_data=None):
        assert pert_mode == 0, "a sparse problem has no random term"
        n = self.rows
        status = np.zeros(len(slots), dtype=np.int32)
        for k, s in enumerate(slots):
            self.calls["lu"] += 1
            H = self._h(k, shift, psi, rhs_mode)
            rhs = self.pop[0][s, :n].copy() if rhs_mode == 0 else self.b
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    x = spla.spsolve(H.tocsc(), rhs)                                          # AMS:58
            if not np.all(np.isfinite(x)):
                status[k] = -2
            else:
                self.pop[2][s, :n] = x
        return status

    def jacobi_check(self, shift, psi):
        ok = np.zeros(len(shift), dtype=bool)
        d0 = self.A.diagonal()
        for k in range(len(shift)):
            d = (d0 - shift[k]) + psi[k]
            with np.errstate(all="ignore"):
                inv = 1.0 / d
            ok[k] = bool(np.all(np.isfinite(inv)) and np.all(np.abs(d) > 1e-12))
        return ok

    def gmres(self, slots, shift, psi, rhs_mode, use_jacobi, rtol=1e-8, restart=20, maxiter=50):
        check_restart("maus_gmres", restart)
        n = self.rows
        info = np.zeros(len(slots), dtype=np.int32)
        inner = np.zeros(len(slots), dtype=np.int32)
        status = np.zeros(len(slots), dtype=np.int32)
        for k, s in enumerate(slots):
            H = self._h(k, shift, psi, rhs_mode)
            rhs = self.pop[0][s, :n].copy() if rhs_mode == 0 else self.b
            if not (np.all(np.isfinite(H.data if sp.issparse(H) else np.asarray(H))) and np.all(np.isfinite(rhs))):
                # what SciPy reports after maxiter cycles of NaN and the device at once: info = maxiter, status 0
                info[k] = max(1, maxiter)
                self.pop[2][s, :n] = rhs
                continue
            M = sp.diags(1.0 / H.diagonal(), format="csc") if use_jacobi[k] else None           # AMS:67-75
            count = [0]
            x, inf = spla.gmres(H, rhs, x0=rhs, rtol=rtol, restart=restart, maxiter=maxiter, M=M,
                                callback=lambda r: count.__setitem__(0, count[0] + 1), callback_type="pr_norm")
            info[k], inner[k] = inf, count[0]
            if inf == 0 and not np.all(np.isfinite(x)):
                status[k] = -2
            self.pop[2][s, :n] = x
        return info, inner, status

    def gmres_pert(self, *a, **kw):
        raise AssertionError("a sparse problem never materialises H with a random term")


def _engine(mode="device", **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=FakeSparseContext(), pert_mode=kw.pop("pert_mode", "mt19937"), sparse_mode=mode, **kw)


def _solver(A, kind, b=None, P=12, tol=1e-8, seed=5, mode="device", **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, SolutionCandidate
    np.random.seed(seed)
    random.seed(seed)
    SolutionCandidate._candidate_id_counter = 0
    return MAUS_Solver(A, kind, b_vector=b, initial_num_candidates=P, global_convergence_tol=tol, quiet=True,
                       engine=_engine(mode, **kw), sparse_mode=mode)


def _tridiag(n, seed=0, far=3):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n), dtype=np.complex128)
    i = np.arange(n)
    A[i, i] = 4.0 + rng.standard_normal(n) + 1j * rng.standard_normal(n)
    A[i[:-1], i[:-1] + 1] = -1.0 + 0.3j * rng.standard_normal(n - 1)
    A[i[1:], i[1:] - 1] = -1.0 + 0.3j * rng.standard_normal(n - 1)
    for _ in range(far):
        r, c = rng.integers(0, n, 2)
        A[r, c] += 0.5 + 0.5j
    return A


def _herm(n, seed=1, real=False):
    rng = np.random.default_rng(seed)
    A = sp.random(n, n, density=3.0 / n, random_state=np.random.RandomState(seed), format="csr")
    A = A + sp.diags(rng.standard_normal(n))
    if not real:
        A = A + 1j * sp.random(n, n, density=2.0 / n, random_state=np.random.RandomState(seed + 1), format="csr")
    A = (A + A.conj().T) * 0.5
    return sp.csr_matrix(A)


# ---- the keyword --------------------------------------------------------------------------------------------------------
def test_default_sparse_mode_still_rejects(monkeypatch):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    monkeypatch.delenv("MAUS_SPARSE", raising=False)
    with pytest.raises(NotImplementedError, match="sparse_mode"):
        MAUS_Solver(sp.identity(8, format="csc"), ProblemType.EIGENVALUE)
    with pytest.raises(NotImplementedError, match="sparse_mode"):
        MAUS_Solver(np.eye(5), ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=np.ones(5), quiet=True,
                    engine=DeviceEngine(ctx=FakeContext()))
    with pytest.raises(ValueError):
        MAUS_Solver(np.eye(5), ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=np.ones(5), sparse_mode="dense")


def test_env_sets_the_default(monkeypatch):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    monkeypatch.setenv("MAUS_SPARSE", "device")
    s = MAUS_Solver(np.eye(5), ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=np.ones(5), initial_num_candidates=3, quiet=True,
                    engine=DeviceEngine(ctx=FakeSparseContext()))
    assert sp.issparse(s.M) and s.engine.sparse_mode == "device"
    monkeypatch.setenv("MAUS_SPARSE", "reject")
    with pytest.raises(NotImplementedError):
        MAUS_Solver(sp.identity(8, format="csc"), ProblemType.EIGENVALUE)


# ---- diagnosis (AMS:374-404) and conversion (AMS:357-358) -----------------------------------------------------------------
def test_ndarray_under_quarter_dense_is_converted_and_critical():
    from adaptive_matrix_solver_amd.solver import ProblemType
    s = _solver(np.eye(5), ProblemType.SOLVE_LINEAR_SYSTEM, b=np.ones(5), P=15, tol=1e-7)     # AMS:644 (20 % nonzeros)
    assert isinstance(s.M, sp.csc_matrix) and s.M.dtype == np.complex128
    pk, st = s.problem_knowledge, s.strat_params
    assert pk["matrix_type"] == "Sparse" and pk["is_sparse_problem"] and pk["is_hermitian"] and pk["is_complex_symmetric"]
    assert s.cond_number == np.inf
    assert pk["numerical_stability_state"] == "Critical" and pk["local_solver_preference"] == "iterative_gmres"
    assert st["overall_psi_aggression_factor"] == 50.0 and st["max_psi_retries"] == 50
    assert st["current_convergence_threshold"] == 1e-2
    assert s.engine.ctx.matrix_is_sparse() == "rows"


def test_spmatrix_keeps_dtype_and_label():
    from adaptive_matrix_solver_amd.solver import ProblemType
    A = sp.csr_matrix(np.diag(np.arange(1.0, 25.0)) + np.diag(np.ones(23), 1) + np.diag(np.ones(23), -1))
    s = _solver(A, ProblemType.EIGENVALUE, P=4)
    assert isinstance(s.M, sp.csr_matrix) and s.M.dtype == np.float64 and s.M is not A
    assert s.problem_knowledge["matrix_type"] == "Dense"              # csr is not converted, so not relabelled (AMS:357)
    assert s.problem_knowledge["is_hermitian"] and s.cond_number == np.inf
    L = sp.lil_matrix(A)
    s2 = _solver(L, ProblemType.EIGENVALUE, P=4)
    assert isinstance(s2.M, sp.csc_matrix) and s2.problem_knowledge["matrix_type"] == "Sparse"


def test_sparray_is_taken_as_the_spmatrix_of_its_format():
    from adaptive_matrix_solver_amd.solver import ProblemType
    A = sp.csr_array(_tridiag(16))
    s = _solver(A, ProblemType.EIGENVALUE, P=4)
    assert isinstance(s.M, sp.csr_matrix) and s.problem_knowledge["is_sparse_problem"]


def test_large_spmatrix_skips_the_symmetry_checks(capsys):
    from adaptive_matrix_solver_amd.solver import ProblemType
    A = sp.identity(3163, format="csr", dtype=np.complex128)          # 3163^2 > 1e7
    s = _solver(A, ProblemType.EIGENVALUE, P=2)
    assert "Sparse matrix too large for dense conversion" in capsys.readouterr().out
    assert not s.problem_knowledge["is_hermitian"] and not s.problem_knowledge["is_complex_symmetric"]
    B = sp.identity(3162, format="csr", dtype=np.complex128)
    assert _solver(B, ProblemType.EIGENVALUE, P=2).problem_knowledge["is_hermitian"]


def test_sharded_sparse_is_refused():
    from adaptive_matrix_solver_amd.engine import DeviceEngine

    class Comm:
        world, rank, on_device, in_root_call = 2, 0, False, False

    eng = DeviceEngine(ctx=FakeSparseContext(), sparse_mode="device")
    eng.comm = Comm()
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.bind_matrix(sp.identity(8, format="csr"))


# ---- the step -------------------------------------------------------------------------------------------------------------
def test_sparse_steps_draw_nothing_and_converge():
    """demo1 of the reference (AMS:644): GMRES on a Critical sparse problem; no random term, so the NumPy stream only moves
    where a candidate is (re)initialised."""
    from adaptive_matrix_solver_amd.solver import ProblemType
    s = _solver(np.eye(5), ProblemType.SOLVE_LINEAR_SYSTEM, b=np.ones(5), P=15, tol=1e-7)
    for it in range(4):
        s._update_global_diagnostics(it + 1)
        s._adjust_global_strategy(it + 1)
        before = np.random.get_state()
        s.step_population()
        after = np.random.get_state()
        assert before[2] == after[2] and np.array_equal(before[1], after[1]), f"iteration {it}: the solve drew random numbers"
        s._manage_candidates(it + 1)
    for c in s.candidates:
        if np.isfinite(c.residual_k):
            assert abs(c.residual_k - np.linalg.norm(s.M @ c.x_k - s.b)) <= 1e-12 * max(1.0, c.residual_k)


# ---- sparse Hermitian shortcut (AMS:186-216) ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,real", [(40, False), (24, True)])
def test_sparse_hermitian_picks_among_the_k_largest(n, real):
    import scipy.linalg as sla
    from adaptive_matrix_solver_amd.solver import ProblemType
    A = _herm(n, real=real)
    s = _solver(A, ProblemType.EIGENVALUE, P=10)
    assert s.problem_knowledge["is_hermitian"] and s.M.dtype == (np.float64 if real else np.complex128)
    s._update_global_diagnostics(1)
    s._adjust_global_strategy(1)
    s.step_population()
    ev = sla.eigvalsh(A.toarray())
    top = np.sort(ev[np.argsort(np.abs(ev))[-6:]])
    for c in s.candidates:
        assert c.state.name == "CONVERGED" and c.w_k == 1.0
        assert np.min(np.abs(top - c.lambda_k)) <= 1e-12 * np.abs(ev).max()
        assert np.linalg.norm(A @ c.v_k - c.lambda_k * c.v_k) <= 1e-10 * np.abs(ev).max()


def test_small_complex_hermitian_falls_back(capsys):
    """N = 6, complex: eigsh hands k = 5 >= N - 1 to eigs, which raises TypeError; the reference prints and the candidate
    takes the general inverse-iteration path."""
    from adaptive_matrix_solver_amd.solver import ProblemType
    A = _herm(6, seed=2)
    s = _solver(A, ProblemType.EIGENVALUE, P=5)
    s.loop_body(1)
    out = capsys.readouterr().out
    assert out.count("Unexpected error during sparse Hermitian solve: Cannot use scipy.linalg.eig for sparse A") == 5
    assert all(c.w_k != 1.0 or c.state.name == "CONVERGED" for c in s.candidates)


def test_inverse_iterate_solver_sparse_device(monkeypatch):
    from adaptive_matrix_solver_amd.solver import InverseIterateSolver
    monkeypatch.setattr(InverseIterateSolver, "_engine", FakeSparseContext())
    A = sp.csc_matrix(_tridiag(30, seed=7))
    b = np.arange(1, 31, dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="sparse_mode"):
        InverseIterateSolver(30, 1e-20, 25, is_sparse=True).solve(A, b, 0)
    for pref, compat in [("direct_solve", "rtol"), ("iterative_gmres", "rtol"), ("iterative_gmres", "scipy-legacy")]:
        before = np.random.get_state()
        s = InverseIterateSolver(30, np.complex128(1e-20), 25, pref, is_sparse=True, gmres_compat=compat, sparse_mode="device")
        x, tries = s.solve(A, b, 0)
        assert tries == 0 and np.array_equal(np.random.get_state()[1], before[1])
        assert np.linalg.norm(A @ x - b) <= 1e-8 * np.linalg.norm(b)
        if compat == "scipy-legacy":
            assert [r["method"] for r in s.last_trace] == ["iterative_gmres", "direct_solve"]


# ---- fixtures captured from the reference (tests/golden/make_sparse_goldens.py) ------------------------------------------
import json  # noqa: E402
import os  # noqa: E402

import snapshot  # noqa: E402
import sparse_scenarios  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(n, m) for n, s in sparse_scenarios.SPARSE_TRAJECTORIES.items() for m in s["modes"]]


def _rows(cands, kind):
    rows = []
    for c in cands:
        if kind == "eig":
            lam, vecs = c.lambda_k, [c.v_k]
        elif kind == "lin":
            lam, vecs = 0j, [c.x_k]
        else:
            lam, vecs = c.sigma_k, [c.u_k, c.right_v_k]
        rows.append({"id": c.id, "state": c.state.value, "stuck": c.stuck_counter, "retries": c.local_psi_retries_needed,
                     "resets": c.num_resets, "w": c.w_k, "resid": c.residual_k, "alpha": c.alpha_local_step,
                     "lam": lam, "vecs": vecs})
    return rows


def _close(a_hex, b_hex, rel):
    a, b = float.fromhex(a_hex), float.fromhex(b_hex)
    return a == b or (np.isfinite(a) and abs(a - b) <= rel * max(1.0, abs(a)))


@pytest.mark.parametrize("name,mode", CASES)
def test_sparse_host_logic_vs_reference_fixtures(name, mode, capsys):
    import scipy
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    with open(os.path.join(GOLD, f"sparse_{name}_{mode.replace('-', '_')}.json")) as f:
        gold = json.load(f)
    if gold["versions"]["numpy"] != np.__version__ or gold["versions"]["scipy"] != scipy.__version__:
        pytest.skip("fixture captured under different numpy/scipy versions")
    spec = sparse_scenarios.SPARSE_TRAJECTORIES[name]
    A, b = sparse_scenarios.build(name)
    np.random.seed(spec["seed"])
    random.seed(spec["seed"])
    SolutionCandidate._candidate_id_counter = 0
    PT = {"eig": ProblemType.EIGENVALUE, "lin": ProblemType.SOLVE_LINEAR_SYSTEM, "svd": ProblemType.SVD}[spec["kind"]]
    s = MAUS_Solver(A, PT, b_vector=b, initial_num_candidates=spec["P"], global_convergence_tol=spec["tol"], quiet=True,
                    engine=_engine(gmres_compat=mode), sparse_mode="device", record_history=True)
    pk = s.problem_knowledge
    assert (pk["matrix_type"], type(s.M).__name__, str(s.M.dtype)) == (gold["matrix_type"], gold["M_format"], gold["M_dtype"])
    assert float(s.cond_number).hex() == gold["cond"] and pk["is_hermitian"] == gold["hermitian"]
    assert snapshot.digest_rows(_rows(s.candidates, spec["kind"])) == gold["init"]["digest"]
    assert snapshot.rng_digest() == gold["init"]["rng"]
    exact = not spec.get("arpack")      # eigsh (ARPACK) vs one eigh per matrix: lambda, residual to rounding
    # (eigsh cases: after the first loop body the redundancy tests order converged candidates by residuals that are
    # rounding noise, SURVEY §7 'tie-sensitivity', so only the first body is compared)
    for it, g in enumerate(gold["iters"] if exact else gold["iters"][:1]):
        s._update_global_diagnostics(it + 1)
        s._adjust_global_strategy(it + 1)
        steps = s.step_population()
        stepped = _rows(s.candidates, spec["kind"])
        s._manage_candidates(it + 1)
        tag = f"{name}/{mode} iter {it}"
        assert steps == g["steps"], tag
        d = snapshot.digest_rows(stepped)
        assert d["ints"] == g["digest_stepped"]["ints"], f"{tag}: bookkeeping"
        assert snapshot.rng_digest() == g["rng"], f"{tag}: RNG streams"
        glob = snapshot.globals_record(s.landscape_energy, s.avg_residual, s.avg_stuckness, s.num_distinct_converged_solutions,
                                       pk["numerical_stability_state"], pk["local_solver_preference"], s.strat_params)
        if exact:
            assert d["floats"] == g["digest_stepped"]["floats"], f"{tag}: scalars"
            assert d["vecs"] == g["digest_stepped"]["vecs"], f"{tag}: vectors"
            assert snapshot.digest_rows(_rows(s.candidates, spec["kind"])) == g["digest"], f"{tag}: managed"
            assert glob == g["globals"], tag
        else:
            got = snapshot.full_rows(stepped, limit=48)
            for rg, rr in zip(got, g["rows"]):
                assert _close(rg["lam"][0], rr["lam"][0], 1e-10) and _close(rg["resid"], rr["resid"], 1.0) or \
                    float.fromhex(rr["resid"]) < 1e-8, (tag, rg, rr)
            for k in ("n_distinct", "stability", "pref", "max_retries"):
                assert glob[k] == g["globals"][k], (tag, k)
        assert int(SolutionCandidate._candidate_id_counter) == g["next_id"], tag
