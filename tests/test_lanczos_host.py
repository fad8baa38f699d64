"""Sparse Hermitian shortcut by thick-restart Lanczos (sparse_eigsh) and the symmetry test on stored entries
(sparse_hermitian_check='sparse'): the host logic on CPU.

FakeLanczosContext adds NumPy doubles of the Lanczos entry points of _cabi.Context (csrc/lanczos.hip) to FakeSparseContext:
the same steps -- product, classical Gram-Schmidt twice against every earlier row, alpha, beta, scaling -- on a NumPy basis.
Checked here: the symmetry verdicts against the reference's dense check (AMS:386-396), the keywords and their defaults, which
path each mode takes, the restart loop against SciPy's eigsh, and the no-convergence report (AMS:211-212)."""
import random

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import snapshot
from test_sparse_host import FakeSparseContext, _herm

EPS = np.finfo(np.float64).eps


class FakeLanczosContext(FakeSparseContext):
    """FakeSparseContext plus the Lanczos entry points; `calls` counts them."""

    def __init__(self):
        super().__init__()
        self.calls.update({"eigvecs": 0, "begin": 0, "extend": 0, "products": 0, "inject": 0, "restart": 0, "finish": 0,
                           "match_rows": 0, "match": 0})
        self.B = self.R = None

    def set_eigvecs(self, V):
        self.calls["eigvecs"] += 1
        super().set_eigvecs(V)

    def herm_match(self, slots):
        self.calls["match"] += 1
        return super().herm_match(slots)

    def _orth(self, w, cnt):
        for _ in range(2):
            h = self.B[:cnt].conj() @ w
            w = w - self.B[:cnt].T @ h
            yield h, w

    def lanczos_begin(self, v0, ncv):
        assert 1 <= ncv <= min(self.rows, 32)
        self.calls["begin"] += 1
        self.B = np.zeros((ncv + 1, self.rows), dtype=np.complex128)
        self.R = None
        self.lanczos_inject(0, v0)
        self.calls["inject"] -= 1

    def lanczos_inject(self, j, v):
        self.calls["inject"] += 1
        w = np.asarray(v, dtype=np.complex128).copy()
        for _h, w in self._orth(w, j):
            pass
        nrm = np.linalg.norm(w)
        self.B[j] = w / nrm if nrm > 0.0 else 0.0                # the device leaves a zero row where the norm is not above 0

    def lanczos_extend(self, j0, j1, tol_abs):
        self.calls["extend"] += 1
        alpha, beta = np.zeros(j1 - j0), np.zeros(j1 - j0)
        for j in range(j0, j1):
            self.calls["products"] += 1
            w = self.A @ self.B[j]
            hs = []
            for h, w in self._orth(w, j + 1):
                hs.append(h[j])
            alpha[j - j0] = (hs[0] + hs[1]).real
            beta[j - j0] = np.linalg.norm(w)
            self.B[j + 1] = w / beta[j - j0] if beta[j - j0] > tol_abs else 0.0
        return alpha, beta

    def lanczos_restart(self, S):
        self.calls["restart"] += 1
        m, keep = S.shape
        assert 1 <= keep < m <= self.B.shape[0] - 1
        new = S.T @ self.B[:m]
        last = self.B[m].copy()
        self.B[:keep] = new
        self.B[keep] = last

    def lanczos_finish(self, S):
        self.calls["finish"] += 1
        m, k = S.shape
        self.R = None
        if k:
            # as the device: the recombination, then row by row classical Gram-Schmidt (twice) against the rows before it; a row
            # of norm zero stays zero
            self.B = S.T @ self.B[:m]
            for q in range(k):
                w = self.B[q]
                for _h, w in self._orth(w, q):
                    pass
                nrm = np.linalg.norm(w)
                self.B[q] = w / nrm if nrm > 0.0 else 0.0
            self.R = self.B
        self.B = None

    def herm_match_rows(self, slots):
        self.calls["match_rows"] += 1
        n = self.rows
        idx = np.empty(len(slots), dtype=np.int32)
        nrm = np.empty(len(slots))
        for i, s in enumerate(slots):
            v = self.pop[0][s, :n]
            j = int(np.argmax(np.abs([np.vdot(v, self.R[q]) for q in range(self.R.shape[0])])))      # AMS:197-198
            nrm[i] = np.linalg.norm(self.R[j])
            self.pop[0][s, :n] = self.R[j] / nrm[i]
            idx[i] = j
        return idx, nrm

    def get_ritz_rows(self):
        return self.R.copy()

    def lanczos_get_basis(self, j0, count):
        assert self.B is not None and 0 <= j0 and 1 <= count and j0 + count <= self.B.shape[0]
        return self.B[j0:j0 + count].copy()


def _engine(ctx=None, **kw):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    return DeviceEngine(ctx=ctx if ctx is not None else FakeLanczosContext(), pert_mode="mt19937", sparse_mode="device", **kw)


def _solver(A, P=8, seed=5, engine=None, **kw):
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(seed)
    random.seed(seed)
    SolutionCandidate._candidate_id_counter = 0
    return MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=P, quiet=True,
                       engine=engine if engine is not None else _engine(), sparse_mode="device", **kw)


# ---- 1. the symmetry test on stored entries ---------------------------------------------------------------------------------
KINDS = ("hermitian", "complex_symmetric", "both", "neither_real", "neither_complex")
MUTATIONS = ("none", "half", "double", "nan", "inf", "one_side_small", "one_side_large")


def _symmetry_case(kind, mutation, seed):
    rng = np.random.default_rng([KINDS.index(kind), MUTATIONS.index(mutation), seed])
    n = int(rng.integers(2, 301))
    B = sp.random(n, n, density=min(1.0, 4.0 / n), random_state=np.random.RandomState(seed + 17), format="lil")
    B = B + sp.diags(rng.standard_normal(n))
    if kind != "both" and kind != "neither_real":
        B = B + 1j * sp.random(n, n, density=min(1.0, 3.0 / n), random_state=np.random.RandomState(seed + 31), format="lil")
    if kind == "hermitian":
        M = B + B.conj().T
    elif kind in ("complex_symmetric", "both"):
        M = B + B.T
    else:
        M = B
    M = sp.lil_matrix(M)
    # an off-diagonal position whose transposed position is stored too (every symmetric kind has one; else any entry)
    C = sp.coo_matrix(M)
    off = [(i, j) for i, j in zip(C.row.tolist(), C.col.tolist()) if i != j]
    i, j = off[int(rng.integers(len(off)))] if off else (0, n - 1)
    thr = 1e-8 + 1e-5 * abs(M[j, i])
    if mutation == "half":
        M[i, j] = M[i, j] + 0.5 * thr
    elif mutation == "double":
        M[i, j] = M[i, j] + 2.0 * thr
    elif mutation == "nan":
        M[i, j] = np.nan
    elif mutation == "inf":
        M[i, j] = np.inf
        M[j, i] = np.inf if rng.integers(2) else -np.inf
    elif mutation in ("one_side_small", "one_side_large"):
        free = [(a, b) for a in range(n) for b in range(n) if a != b and M[a, b] == 0 and M[b, a] == 0][:1]
        if free:
            M[free[0]] = 0.5e-8 if mutation == "one_side_small" else 3e-8
    fmt = ("csr", "csc", "coo")[seed % 3]
    return getattr(sp, f"{fmt}_matrix")(M)


def _verdicts(M, mode):
    """the two verdicts of MAUS_Solver._diagnose_matrix_initial under sparse_hermitian_check = mode"""
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    s = MAUS_Solver.__new__(MAUS_Solver)
    s._sparse_hermitian_check = mode
    s.problem_type = ProblemType.EIGENVALUE
    d = s._diagnose_matrix_initial(M)
    return d["is_hermitian"], d["is_complex_symmetric"]


def test_sparse_symmetry_check_gives_the_dense_verdicts(capsys):
    seen = set()
    count = 0
    for kind in KINDS:
        for mutation in MUTATIONS:
            for seed in range(6):
                M = _symmetry_case(kind, mutation, seed)
                D = M.todense()
                with np.errstate(invalid="ignore"):
                    want = (bool(np.allclose(D, D.conj().T)), bool(np.allclose(D, D.T)))       # AMS:394-395
                    assert _verdicts(M, "reference") == want
                    got = _verdicts(M, "sparse")
                assert got == want, (kind, mutation, seed, M.shape, got, want)
                seen.add((mutation,) + want)
                count += 1
    assert count >= 200
    # the cases do discriminate: every verdict pair occurs, the half-threshold move keeps a verdict the double one loses
    assert {w[1:] for w in seen} == {(True, True), (True, False), (False, True), (False, False)}
    assert ("half", True, False) in seen and ("double", True, False) not in seen
    assert ("one_side_small", True, False) in seen and ("one_side_large", True, False) not in seen
    assert not any(w[1] or w[2] for w in seen if w[0] == "nan")
    assert "too large" not in capsys.readouterr().out


def test_sparse_symmetry_check_explicit_zeros_and_duplicates():
    from adaptive_matrix_solver_amd.solver import sparse_symmetry_verdicts
    # duplicates are summed as todense() sums them; an explicitly stored zero is an entry like any other
    M = sp.coo_matrix((np.array([1.0, 1.0, 2.0, 0.0]), (np.array([0, 0, 1, 2]), np.array([1, 1, 0, 0]))), shape=(3, 3))
    D = M.todense()
    assert sparse_symmetry_verdicts(M) == (bool(np.allclose(D, D.conj().T)), bool(np.allclose(D, D.T))) == (True, True)
    assert sparse_symmetry_verdicts(sp.csr_matrix((4, 4))) == (True, True)


def test_sparse_symmetry_check_at_n_4000(capsys):
    A = _herm(4000, seed=3)
    s = _solver(A, P=2)
    assert "Sparse matrix too large for dense conversion" in capsys.readouterr().out
    assert not s.problem_knowledge["is_hermitian"]
    s = _solver(A, P=2, sparse_hermitian_check="sparse")
    assert "too large" not in capsys.readouterr().out
    assert s.problem_knowledge["is_hermitian"] and not s.problem_knowledge["is_complex_symmetric"]
    R = _herm(4000, seed=3, real=True)
    s = _solver(R, P=2, sparse_hermitian_check="sparse")
    assert s.problem_knowledge["is_hermitian"] and s.problem_knowledge["is_complex_symmetric"]


# ---- 2. the keywords --------------------------------------------------------------------------------------------------------
def test_keywords_are_validated(monkeypatch):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType
    monkeypatch.delenv("MAUS_SPARSE_EIGSH", raising=False)
    with pytest.raises(ValueError, match="sparse_eigsh"):
        DeviceEngine(ctx=FakeLanczosContext(), sparse_eigsh="arpack")
    with pytest.raises(ValueError, match="sparse_eigsh"):
        MAUS_Solver(np.eye(5), ProblemType.EIGENVALUE, sparse_eigsh="arpack")
    with pytest.raises(ValueError, match="sparse_hermitian_check"):
        MAUS_Solver(np.eye(5), ProblemType.EIGENVALUE, sparse_hermitian_check="dense")
    assert DeviceEngine(ctx=FakeLanczosContext()).sparse_eigsh == "auto"
    monkeypatch.setenv("MAUS_SPARSE_EIGSH", "lanczos")
    assert DeviceEngine(ctx=FakeLanczosContext()).sparse_eigsh == "lanczos"
    assert DeviceEngine(ctx=FakeLanczosContext(), sparse_eigsh="dense").sparse_eigsh == "dense"
    monkeypatch.setenv("MAUS_SPARSE_EIGSH", "nonsense")
    with pytest.raises(ValueError, match="sparse_eigsh"):
        DeviceEngine(ctx=FakeLanczosContext())


@pytest.mark.parametrize("mode,lu_max,lanczos", [("auto", 16384, False), ("auto", 100, True), ("dense", 100, False),
                                                  ("lanczos", 16384, True)])
def test_mode_chooses_the_path(mode, lu_max, lanczos):
    ctx = FakeLanczosContext()
    A = _herm(160, seed=4)
    s = _solver(A, P=6, engine=_engine(ctx, sparse_eigsh=mode))
    assert s.problem_knowledge["is_hermitian"]
    ctx.lu_max_n = lambda: lu_max                           # (after the start-up: the direct solves are not the subject)
    s._update_global_diagnostics(1)
    s._adjust_global_strategy(1)
    s.step_population()
    c = ctx.calls
    if lanczos:
        assert c["begin"] == 1 and c["finish"] == 1 and c["extend"] >= 1 and c["match_rows"] == 1
        assert c["eigvecs"] == 0 and c["match"] == 0
        assert s.engine.lanczos_stats["converged"] and s.engine.lanczos_stats["products"] == c["products"]
    else:
        assert c["eigvecs"] == 1 and c["match"] == 1
        assert c["begin"] == c["extend"] == c["finish"] == c["match_rows"] == 0
    ev = np.linalg.eigvalsh(A.toarray())
    top = np.sort(ev[np.argsort(np.abs(ev))[-6:]])
    for cand in s.candidates:
        assert cand.state.name == "CONVERGED" and cand.w_k == 1.0
        assert np.min(np.abs(top - cand.lambda_k)) <= 1e-9 * np.abs(ev).max()
    s.step_population()                                     # the outcome is cached per matrix object
    assert c["begin"] == (1 if lanczos else 0) and c["eigvecs"] == (0 if lanczos else 1)


def test_type_error_texts_stay_in_every_mode(capsys):
    for mode in ("dense", "lanczos", "auto"):
        A = _herm(6, seed=2)
        s = _solver(A, P=5, engine=_engine(sparse_eigsh=mode))
        s.loop_body(1)
        assert capsys.readouterr().out.count(
            "Unexpected error during sparse Hermitian solve: Cannot use scipy.linalg.eig for sparse A with k >= N - 1") == 5
        assert s.engine.ctx.calls["begin"] == 0
    R = sp.csr_matrix(np.diag(np.arange(1.0, 7.0)))
    eng = _engine(sparse_eigsh="lanczos")
    assert eng._eigsh_refusal(R) is None and eng._eigsh_refusal(R[:1, :1]).startswith("Cannot use scipy.linalg.eigh for sparse A")


# ---- 3. the restart loop ----------------------------------------------------------------------------------------------------
def _floor(A, ncv=20):
    """rounding floor of a residual: ncv eps ||A||_1 (SciPy's own eigsh leaves nothing above tol |theta| on these matrices)"""
    return ncv * EPS * abs(A).sum(axis=0).max()


def test_restart_loop_returns_eigsh_values_400():
    from adaptive_matrix_solver_amd.engine import eigsh_parameters, thick_restart_lanczos
    n, tol = 400, 1e-10
    A = _herm(n, seed=6)
    v0 = np.random.default_rng(1).standard_normal(n)
    want = np.sort(spla.eigsh(A, k=6, which="LM", v0=v0, tol=tol)[0])
    k, ncv = eigsh_parameters(n)
    assert (k, ncv) == (6, 20) and eigsh_parameters(5) == (4, 5) and eigsh_parameters(1) == (1, 1) and eigsh_parameters(12) == (6, 12)
    ctx = FakeLanczosContext()
    ctx.set_matrix_csr(A)
    anorm = abs(A).sum(axis=0).max()
    before = snapshot.rng_digest()
    run = thick_restart_lanczos(ctx, n, k, ncv, tol, EPS * anorm, 10 * n, v0 + 0j, lambda: 1 / 0)
    assert snapshot.rng_digest() == before
    assert run["converged"] and run["nconv"] == 6 and run["restarts"] >= 1
    assert run["restarts"] == ctx.calls["restart"] and ctx.calls["begin"] == ctx.calls["finish"] == 1
    # the first sweep takes ncv products, every restart ncv - keep with k <= keep <= k + (ncv - k) / 2
    assert run["products"] == ctx.calls["products"]
    assert ncv + run["restarts"] * (ncv - k - (ncv - k) // 2) <= run["products"] <= ncv + run["restarts"] * (ncv - k)
    theta, R = run["theta"], ctx.get_ritz_rows()
    assert np.all(np.diff(theta) > 0) and R.shape == (6, n) and ctx.B is None
    floor = _floor(A)
    assert np.all(np.abs(theta - want) <= 2 * (tol * np.abs(theta) + floor))
    for q in range(6):
        assert np.linalg.norm(A @ R[q] - theta[q] * R[q]) <= tol * abs(theta[q]) + floor
    assert np.linalg.norm(R.conj() @ R.T - np.eye(6)) <= 100 * EPS


def test_breakdown_continues_from_a_private_vector():
    """Three distinct eigenvalues: the Krylov space of v0 is exhausted after three steps; the run continues from fresh vectors
    (no draw from the global streams) and ends with six eigenpairs."""
    from adaptive_matrix_solver_amd.engine import thick_restart_lanczos
    n = 60
    d = np.repeat([5.0, -3.0, 1.0], n // 3)
    A = sp.diags(d).tocsr()
    ctx = FakeLanczosContext()
    ctx.set_matrix_csr(A)
    rng = np.random.default_rng(2)
    before = snapshot.rng_digest()
    run = thick_restart_lanczos(ctx, n, 6, 20, 1e-10, EPS * 5.0 * 50, 10 * n, rng.standard_normal(n) + 0j,
                                lambda: rng.standard_normal(n) + 0j)
    assert snapshot.rng_digest() == before
    assert run["converged"] and ctx.calls["inject"] >= 1
    R = ctx.get_ritz_rows()
    # two exhausted Krylov spaces of dimension three make an invariant subspace with k pairs: that is the result
    assert ctx.calls["inject"] == 1 and np.allclose(run["theta"], [-3, -3, 1, 1, 5, 5], atol=1e-12)
    for q in range(6):
        assert np.linalg.norm(A @ R[q] - run["theta"][q] * R[q]) <= 1e-12
    assert np.linalg.norm(R.conj() @ R.T - np.eye(6)) <= 1e-12
    # an invariant subspace that already holds k pairs is the result
    A2 = sp.diags(np.repeat(np.arange(1.0, 9.0), 5)).tocsr()
    ctx.set_matrix_csr(A2)
    run = thick_restart_lanczos(ctx, 40, 6, 20, 1e-10, EPS * 8.0 * 50, 400, rng.standard_normal(40) + 0j, lambda: 1 / 0)
    assert run["converged"] and run["restarts"] == 0 and np.allclose(run["theta"], np.arange(3.0, 9.0), atol=1e-12)


class NeverConverges(FakeLanczosContext):
    """Coefficients that grow from sweep to sweep, whatever the matrix: the largest Ritz values always sit on the newest rows,
    coupled to the residual vector with beta = 1, so no wanted pair ever passes the test."""

    def lanczos_extend(self, j0, j1, tol_abs):
        self.calls["extend"] += 1
        return 10.0 * self.calls["extend"] + np.arange(j0, j1), np.ones(j1 - j0)

    def lanczos_restart(self, S):
        self.calls["restart"] += 1


def test_no_convergence_prints_the_reference_line_and_falls_back(capsys):
    n, P = 40, 7
    A = _herm(n, seed=8)
    ctx = NeverConverges()
    s = _solver(A, P=P, engine=_engine(ctx, sparse_eigsh="lanczos"))
    eng = s.engine
    cands = list(s.candidates)
    slots = eng._slots(cands)
    states = [c.state for c in cands]
    vecs = [c.v_k.copy() for c in cands]
    for c in cands:
        c._push()
    before = snapshot.rng_digest()
    capsys.readouterr()
    left = eng._hermitian(cands, s.M, slots, s.strat_params)
    out = capsys.readouterr().out
    assert snapshot.rng_digest() == before
    assert left == cands and ctx.calls["restart"] == 10 * n and ctx.calls["match_rows"] == 0
    for c, st, v in zip(cands, states, vecs):
        assert c.state == st and c.state.name != "CONVERGED" and np.array_equal(c.v_k, v)
        assert f"Candidate {c.id}: Sparse Hermitian solver (eigsh) failed to converge: ARPACK error -1: No convergence " \
               f"({10 * n + 1} iterations, 0/6 eigenvectors converged). Falling back." in out
    # cached per matrix object: the next call reports again without another run
    eng._hermitian(cands, s.M, slots, s.strat_params)
    assert ctx.calls["begin"] == 1 and capsys.readouterr().out.count("failed to converge") == P
    # and a whole step takes the general path
    s.step_population()
    assert ctx.calls["begin"] == 1


# ---- the fixtures captured from the unmodified reference (ARPACK's eigsh) ------------------------------------------------------
def residual_bound(A, lam, tol=1e-10, ncv=20):
    """what the method promises of an accepted pair: tol |theta| plus the rounding floor ncv eps ||A||_1"""
    return tol * abs(lam) + min(ncv, A.shape[0]) * EPS * float(abs(sp.csr_matrix(A)).sum(axis=0).max())


def rows_agree_with_arpack(A, got_rows, gold_rows, tag):
    """lambda always within 1e-10 of ARPACK's; the residual equal to ARPACK's within its own size, or both below the bound"""
    from test_sparse_host import _close
    assert len(got_rows) == len(gold_rows)
    for rg, rr in zip(got_rows, gold_rows):
        assert _close(rg["lam"][0], rr["lam"][0], 1e-10), (tag, rg, rr)
        bound = residual_bound(A, float.fromhex(rr["lam"][0]))
        both_small = float.fromhex(rg["resid"]) <= bound and float.fromhex(rr["resid"]) <= bound
        assert _close(rg["resid"], rr["resid"], 1.0) or both_small, (tag, rg, rr, bound)


@pytest.mark.parametrize("name", ["sp_herm40", "sp_real_herm24"])
def test_reference_fixtures_through_the_restart_loop(name):
    """The first loop body of the reference's ARPACK cases under sparse_eigsh='lanczos', compared as tests/test_sparse_host.py
    compares them under the dense replacement: bookkeeping and both RNG streams exact, lambda to 1e-10, residuals at their level."""
    import json
    import os
    import scipy
    import sparse_scenarios
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    from test_sparse_host import GOLD, _rows
    with open(os.path.join(GOLD, f"sparse_{name}_rtol.json")) as f:
        gold = json.load(f)
    if gold["versions"]["numpy"] != np.__version__ or gold["versions"]["scipy"] != scipy.__version__:
        pytest.skip("fixture captured under different numpy/scipy versions")
    spec = sparse_scenarios.SPARSE_TRAJECTORIES[name]
    A, b = sparse_scenarios.build(name)
    np.random.seed(spec["seed"])
    random.seed(spec["seed"])
    SolutionCandidate._candidate_id_counter = 0
    s = MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=spec["P"], global_convergence_tol=spec["tol"], quiet=True,
                    engine=_engine(gmres_compat="rtol", sparse_eigsh="lanczos"), sparse_mode="device", record_history=True)
    assert snapshot.rng_digest() == gold["init"]["rng"]
    g = gold["iters"][0]
    s._update_global_diagnostics(1)
    s._adjust_global_strategy(1)
    assert s.step_population() == g["steps"]
    stepped = _rows(s.candidates, "eig")
    s._manage_candidates(1)
    assert s.engine.ctx.calls["begin"] == 1 and s.engine.lanczos_stats["converged"]
    assert snapshot.digest_rows(stepped)["ints"] == g["digest_stepped"]["ints"]
    assert snapshot.rng_digest() == g["rng"]
    rows_agree_with_arpack(A, snapshot.full_rows(stepped, limit=48), g["rows"], name)
    assert int(SolutionCandidate._candidate_id_counter) == g["next_id"]
