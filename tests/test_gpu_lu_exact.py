"""Dense LU on the device against planted factors, bit for bit (GPU box only).

The systems, the bound that makes them exact and the restated dispatch are tests/lu_cases.py; tests/test_lu_cases_host.py has
already shown on the CPU that LAPACK returns the planted ipiv, L, U and x on every case it can factor, that every case stays
within 45 significand bits, and that a wrong pivot rule or a wrong entry is seen.  Here every case demands status, ipiv and x
equal to the planted ones (np.array_equal), and that the kernel instantiations the case table promises are the ones the
dispatch takes at this device's CU count.  DESIGN section 12 maps every instantiation of csrc/lu.hip to its case."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import lu_cases as lc

pytestmark = pytest.mark.gpu

POP_X, POP_W = 0, 2
# Gaussian complement: the device's normwise backward error may be this many times LAPACK's on the same system.  Four times
# the largest ratio recorded on an MI355X, 3.11 at n = 8224 (where every case's ratio is listed).
BACKWARD_RATIO = 4 * 3.11


@pytest.fixture(scope="module")
def contexts():
    from adaptive_matrix_solver_amd import Context
    cs = {"default": Context(0), "shared": Context(0)}
    cs["shared"].set_shared_device(True)
    yield cs
    for c in cs.values():
        c.close()


def _cus(ctx):
    return ctx.device_info()["cus"]


def _check_reached(case, context, ctx):
    """The instantiations the table promises for this case are the ones the dispatch takes on this device."""
    got = lc.variants(case["n"], case["G"], _cus(ctx), context == "shared", case["nbo"] or 512)
    missing = lc.promised(case, context) - got
    assert not missing, f"{case['name']} ({context}, {_cus(ctx)} CUs) does not reach {sorted(missing)}: it runs {sorted(got)}"
    return got


def _solve_exact(ctx, A, b, x, ipiv, what, singular=None):
    """singular: {matrix index: first zero column} of the planted singular matrices of the batch."""
    singular = singular or {}
    aborts = ctx.lu_mw_aborts()
    xg, status, pg = ctx.lu_solve(A, b, want_ipiv=True)
    for g in range(A.shape[0]):
        assert status[g] == (singular[g] + 1 if g in singular else 0), (what, g, status)
        bad = np.flatnonzero(pg[g] != ipiv[g])
        assert bad.size == 0, f"{what}[{g}]: ipiv differs first at column {bad[:1]}: {pg[g][bad[:4]]} for {ipiv[g][bad[:4]]} ({bad.size} columns)"
        if g not in singular:
            bad = np.flatnonzero(xg[g] != x[g])
            assert bad.size == 0, f"{what}[{g}]: x differs first at row {bad[:1]}: {xg[g][bad[:3]]} for {x[g][bad[:3]]} ({bad.size} rows)"
    assert ctx.lu_mw_aborts() == aborts == 0, f"{what}: a multi-workgroup panel timed out; the path was not exercised"


@pytest.mark.parametrize("name", [c["name"] for c in lc.TABLE])
def test_table_case_bit_for_bit(contexts, monkeypatch, name):
    case = next(c for c in lc.TABLE if c["name"] == name)
    if case["nbo"]:
        monkeypatch.setenv("MAUS_LU_NBO", str(case["nbo"]))
    A, b, x, ipiv = lc.case_batch(case)
    for context in case["contexts"]:
        ctx = contexts[context]
        _check_reached(case, context, ctx)
        _solve_exact(ctx, A, b, x, ipiv, f"{name}/{context}")


def test_every_instantiation_is_reached_on_this_device(contexts):
    """The union over the table at this device's CU count is every reachable instantiation of csrc/lu.hip."""
    reached = set()
    for case in lc.TABLE:
        for context in case["contexts"]:
            reached |= _check_reached(case, context, contexts[context])
    assert reached == set(lc.ALL_VARIANTS), sorted(set(lc.ALL_VARIANTS) - reached)


def _family_runs(n, name):
    """(context, MAUS_LU_NBO or None) of a family: both contexts; the zero columns of a size with a single outer block also
    under an outer block of 96 columns, where they fall into the first, second and third block."""
    runs = [("default", None), ("shared", None)]
    if name.startswith("zero") and lc.ZERO_NBO[n]:
        runs += [("default", lc.ZERO_NBO[n]), ("shared", lc.ZERO_NBO[n])]
    return runs


@pytest.mark.parametrize("n,name", [(n, name) for n in lc.FAMILY_SIZES for name in lc.FAMILIES[n]])
def test_pivot_and_edge_families(contexts, monkeypatch, n, name):
    """identity / last / reverse / random interchanges, tie columns (first index wins: against the pivot row's own lane,
    wave, workgroup and the others), rule columns (|re| + |im|, not the modulus), planted zero pivots."""
    kw = lc.FAMILIES[n][name]
    A, b, x, ipiv, _, _ = lc.system(n, lc.family_seed(n, name), **kw)
    zc = kw.get("zero_cols")
    for context, nbo in _family_runs(n, name):
        if nbo:
            monkeypatch.setenv("MAUS_LU_NBO", str(nbo))
        else:
            monkeypatch.delenv("MAUS_LU_NBO", raising=False)
        _solve_exact(contexts[context], A[None], b[None], x[None], ipiv[None], f"{name}/n{n}/{context}/nbo{nbo}",
                     singular={0: min(zc)} if zc else None)


@pytest.mark.parametrize("n", lc.FAMILY_SIZES)
def test_singular_matrix_inside_a_batch(contexts, n):
    """A batch of three with the singular matrix in the middle: its first zero column is reported, its neighbours are exact."""
    names = ["ties_rules_random", "zero_two", "piv_last"]
    S = [lc.system(n, lc.family_seed(n, nm), **lc.FAMILIES[n][nm]) for nm in names]
    A, b, x, ipiv = (np.stack([s[k] for s in S]) for k in range(4))
    for context in ("default", "shared"):
        _solve_exact(contexts[context], A, b, x, ipiv, f"batch/n{n}/{context}", singular={1: min(lc.FAMILIES[n]["zero_two"]["zero_cols"])})


@pytest.mark.parametrize("n,col", [(17, 16), (33, 20), (33, 32)])
def test_zero_column_beside_pad_rows(contexts, n, col):
    """Every candidate of the column is zero, the pad rows' too: the first index wins, never a pad row."""
    A, b, x, ipiv, _, _ = lc.planted(n, 900 + n + col, pivots="random", zero_cols=[col])
    assert ipiv[col] == col
    for context in ("default", "shared"):
        _solve_exact(contexts[context], A[None], b[None], x[None], ipiv[None], f"zero_pad/n{n}/{context}", singular={0: col})


@pytest.mark.parametrize("csr", [False, True], ids=["dense", "csr"])
@pytest.mark.parametrize("rhs_mode", [0, 1])
@pytest.mark.parametrize("n", lc.FAMILY_SIZES)
def test_candidate_step_path(contexts, n, rhs_mode, csr):
    """maus_shifted_lu_solve on A_dev = H + (lambda - psi) I: build_h_kernel / build_h_csr_kernel give back the planted H
    exactly for five candidates in scattered slots with their own integer (lambda_k, psi_k), and W is the planted x.  With
    CSR the shift makes one diagonal entry of A_dev exactly zero, which is then not stored."""
    ctx = contexts["default"]
    H, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, "ties_rules_random"), **lc.FAMILIES[n]["ties_rules_random"])
    rng = np.random.default_rng(n + 10 * rhs_mode + csr)
    dg = np.diagonal(H)
    whole = np.flatnonzero((dg.real == np.rint(dg.real)) & (dg.imag == np.rint(dg.imag)) & (dg != 0))
    i0 = int(whole[len(whole) // 2])
    d = -dg[i0] if csr else complex(3, -2)                          # lambda - psi, a Gaussian integer
    A_dev = H + d * np.eye(n)
    slots = [7, 2, 11, 0, 5]
    psi = np.array([1.0, 2.0, 4.0, 7.0, 3.0])
    lam = d + psi
    if rhs_mode == 0:
        X = (rng.integers(-3, 4, (5, n)) + 1j * rng.integers(-3, 4, (5, n))).astype(np.complex128)
        B = X @ H.T
    else:
        X, B = np.tile(x, (5, 1)), np.tile(b, (5, 1))
    if csr:
        M = sp.csr_matrix(A_dev)
        M.eliminate_zeros()
        assert M[i0, i0] == 0 and i0 not in M[i0].indices
        ctx.set_matrix_csr(M)
    else:
        ctx.set_matrix(A_dev)
    ctx.pop_reserve(12)
    ctx.pop_put(POP_X, slots, B if rhs_mode == 0 else np.zeros((5, n)))
    ctx.pop_put(POP_W, slots, np.zeros((5, n)))
    ctx.set_rhs(b)
    status = ctx.shifted_lu_solve(slots, lam, psi, rhs_mode=rhs_mode, pert_mode=0)
    assert (status == 0).all(), status
    W = ctx.pop_get(POP_W, slots, n)
    for k in range(5):
        bad = np.flatnonzero(W[k] != X[k])
        assert bad.size == 0, f"candidate {k} (slot {slots[k]}): {bad.size} rows differ, first {bad[:1]}: {W[k][bad[:3]]} for {X[k][bad[:3]]}"
    assert ctx.lu_mw_aborts() == 0, "a multi-workgroup panel timed out; the path was not exercised"


# one Gaussian system per row of the case table: (table case whose shape, batch, contexts and outer block it takes)
GAUSSIAN = ["n33", "n224", "n224_nbo96", "n1024", "n1056", "n2048", "n2080", "n4128", "n8160", "n8224"]


@pytest.mark.parametrize("name", GAUSSIAN)
def test_gaussian_backward_error_against_lapack(contexts, monkeypatch, name):
    """Integer data cannot show a loss of precision: complex Gaussian systems of the same shapes, the normwise backward error
    ||b - A x||_inf / (||A||_inf ||x||_inf + ||b||_inf) in np.longdouble against LAPACK's on the same system.  The device
    differs from LAPACK by 3M products and inverted 16 x 16 unit-lower blocks; ratios seen on an MI355X: DESIGN section 12."""
    case = next(c for c in lc.TABLE if c["name"] == name)
    if case["nbo"]:
        monkeypatch.setenv("MAUS_LU_NBO", str(case["nbo"]))
    n, G = case["n"], case["G"]
    A, b = lc.gaussian(n, 5000 + n, G)
    xs = [[sla.lu_solve(sla.lu_factor(A[g], check_finite=False), b[g], check_finite=False)] for g in range(G)]
    for context in case["contexts"]:
        x, status = contexts[context].lu_solve(A, b)
        assert (status == 0).all(), status
        for g in range(G):
            xs[g].append(x[g])
    errs = np.array([lc.backward_errors(A[g], xs[g], b[g]) for g in range(G)])      # [matrix][lapack, contexts...]
    for k, context in enumerate(case["contexts"]):
        ratio = float(np.max(errs[:, k + 1] / errs[:, 0]))
        print(f"backward error {name}/{context}: device {errs[:, k + 1].max():.3e} lapack {errs[:, 0].max():.3e} ratio {ratio:.2f}")
        assert ratio <= BACKWARD_RATIO, (name, context, errs)
    assert contexts["default"].lu_mw_aborts() == 0
