"""CPU tier of the exact dense-LU tests: what tests/test_gpu_lu_exact.py demands of the device is first demanded of LAPACK
and of the case table itself (tests/lu_cases.py).

* LAPACK reproduces the planted ipiv, L, U and x bit for bit on every case small enough to factor here (n <= 2112), singular
  ones included, and on the sparse-L recipe at n = 1056.
* budget_bits <= 45 for every case of the table, the large ones included: a condition on the generator, not a measurement.
* The comparisons are sensitive: an unblocked LU with a planted wrong pivot rule gives another ipiv on the tie and rule
  cases, and one changed entry of U changes x.
* The restated dispatch reaches every reachable kernel instantiation of csrc/lu.hip over the table at 256 CUs."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import lu_cases as lc

BUDGET = 45


def _dense(L):
    return L.toarray() if sp.issparse(L) else L


def _lapack_matches(A, b, x, ipiv, L, U, singular_at=None):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # LinAlgWarning on the planted singular matrices
        lu, piv = sla.lu_factor(A, check_finite=False)
    assert np.array_equal(piv, ipiv), "ipiv"
    assert np.array_equal(np.triu(lu), U), "U"
    if singular_at is None:
        assert np.array_equal(np.tril(lu, -1), np.tril(_dense(L), -1)), "L"
        assert np.array_equal(sla.lu_solve((lu, piv), b), x), "x"
    else:
        zeros = np.flatnonzero(np.diagonal(lu) == 0)
        assert zeros.size and zeros[0] == singular_at, (zeros, singular_at)


SMALL = [c for c in lc.TABLE if c["n"] <= 2112]


@pytest.mark.parametrize("name", [c["name"] for c in SMALL])
def test_lapack_reproduces_the_table_cases(name):
    case = next(c for c in lc.TABLE if c["name"] == name)
    n, G = case["n"], case["G"]
    for g in range(G):
        kw = lc.case_kwargs(case, g)
        A, b, x, ipiv, L, U = lc.system(n, case["seed"] + 1000 * g, case["sparse"], **kw)
        _lapack_matches(A, b, x, ipiv, L, U)
        assert lc.budget_bits(L, U, x) <= BUDGET


@pytest.mark.parametrize("n", lc.FAMILY_SIZES)
def test_lapack_reproduces_the_families(n):
    for name, kw in lc.FAMILIES[n].items():
        A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, name), **kw)
        zc = kw.get("zero_cols")
        try:
            _lapack_matches(A, b, x, ipiv, L, U, singular_at=min(zc) if zc else None)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        assert lc.budget_bits(L, U, None if zc else x) <= BUDGET, name


def test_lapack_reproduces_the_sparse_recipe():
    n = 1056
    ties = lc.every(n, 37, 5)
    for piv in ("random", "last"):
        A, b, x, ipiv, L, U = lc.planted(n, 77, pivots=piv, tie_cols=ties, rule_cols=lc.every(n, 101, 50, avoid=ties), sparse_L=True)
        assert sp.issparse(L)
        off = L - sp.identity(n, format="csr")
        r, c = off.nonzero()
        outside = c < r - r % lc.BLK                               # entries to the left of the row's diagonal block
        # at most 32 per row, plus the tie / rule multipliers that were planted on top
        assert np.bincount(r[outside], minlength=n).max() <= lc.SPARSE_ROW_NNZ + len(ties) // 8 + 3
        _lapack_matches(A, b, x, ipiv, L, U)
        assert lc.budget_bits(L, U, x) <= BUDGET


@pytest.mark.parametrize("name", [c["name"] for c in lc.TABLE if c["n"] > 2112])
def test_budget_of_the_large_cases(name):
    case = next(c for c in lc.TABLE if c["name"] == name)
    A, b, x, ipiv, L, U = lc.system(case["n"], case["seed"], case["sparse"], **lc.case_kwargs(case, 0))
    assert lc.budget_bits(L, U, x) <= BUDGET
    # P A = L U on a sample of rows (the full product is what planted() computed; this checks the permutation bookkeeping)
    p = lc.final_order(ipiv)
    rows = np.random.default_rng(1).integers(0, case["n"], 8)
    assert np.array_equal(A[p[rows]], np.asarray(L[rows] @ U))
    assert np.array_equal(A @ x, b)


def test_budget_counts_what_it_should():
    """One multiplier of 2^-30 costs 30 fraction bits in L and as many again in the block inverse."""
    A, b, x, ipiv, L, U = lc.planted(64, 3, pivots="identity")
    base = lc.budget_bits(L, U, x)
    L2 = L.copy()
    L2[5, 4] = 2.0 ** -30
    assert lc.budget_bits(L2, U, x) >= base + 25
    X = lc.diag_block_inverses(L)
    for k in range(4):
        assert np.array_equal(X[k] @ L[16 * k:16 * k + 16, 16 * k:16 * k + 16], np.eye(16))


def test_wrong_pivot_rules_and_wrong_entries_are_seen():
    n = 224
    fam = lc.FAMILIES[n]
    for name in ("ties_identity", "rules_random", "ties_rules_random"):
        A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, name), **fam[name])
        got, lu = lc.numpy_lu(A, "lapack")
        assert np.array_equal(got, ipiv) and np.array_equal(np.triu(lu), U), name
        wrong = {"last": "ties" in name, "modulus": "rules" in name, "pad": True}
        for rule, differs in wrong.items():
            got, _ = lc.numpy_lu(A, rule)
            assert np.array_equal(got, ipiv) != differs, (name, rule)
    # every tie column alone separates the last-index rule, every rule column the modulus rule
    A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, "ties_identity"), **fam["ties_identity"])
    got, _ = lc.numpy_lu(A, "last")
    assert got[fam["ties_identity"]["tie_cols"][0]] != ipiv[fam["ties_identity"]["tie_cols"][0]]
    A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, "rules_identity"), **fam["rules_identity"])
    got, _ = lc.numpy_lu(A, "modulus")
    assert got[fam["rules_identity"]["rule_cols"][0]] != ipiv[fam["rules_identity"]["rule_cols"][0]]
    # one entry of U off by one changes x
    A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, "piv_random"), **fam["piv_random"])
    U2 = U.copy()
    U2[100, 200] += 1
    A2 = np.empty_like(A)
    A2[lc.final_order(ipiv)] = L @ U2
    x2 = sla.solve(A2, b)
    assert not np.array_equal(x2, x) and np.max(np.abs(x2 - x)) > 1e-6


def test_tie_rows_pair_every_way():
    """Over the tie columns of the identity family the tied rows sit in the pivot row's lane at another slot, in another
    lane of its wave, in another wave and (n > 1024) in another workgroup of the multi-workgroup panel."""
    for n in lc.FAMILY_SIZES:
        kw = lc.FAMILIES[n]["ties_identity"]
        A, b, x, ipiv, L, U = lc.system(n, lc.family_seed(n, "ties_identity"), **kw)
        seen = set()
        for j in kw["tie_cols"]:
            rows = np.flatnonzero(lc.cabs1(L[j + 1:, j]) == 1) + j + 1
            assert rows.size or j >= n - 1, j
            for r in rows:
                d = r - j
                if d in (128, 256, 512, 1024):
                    seen.add("slot")
                elif (j % 16) + d < 64:
                    seen.add("lane")
                elif d > 1024:
                    seen.add("workgroup")
                else:
                    seen.add("wave")
        assert seen >= ({"slot", "lane", "wave"} | ({"workgroup"} if n > 1100 + 37 else set())), (n, seen)


def test_the_table_reaches_every_reachable_instantiation():
    ncu = 256
    reached = set()
    for case in lc.TABLE:
        for context in case["contexts"]:
            got = lc.variants(case["n"], case["G"], ncu, context == "shared", case["nbo"] or 512)
            missing = lc.promised(case, context) - got
            assert not missing, (case["name"], context, missing)
            reached |= got
    assert reached == set(lc.ALL_VARIANTS), (set(lc.ALL_VARIANTS) - reached, reached - set(lc.ALL_VARIANTS))
    # lu_panel_ip_kernel<1,8> and <2,8>: no m, batch, CU count or context reaches them while the base panel is 16 wide
    for m in range(16, 16384 + 1, 16):
        for G in (1, 3, 64, 300):
            for mw in (False, True):
                for npad in (max(m, 32), 16384):
                    assert lc.panel_variant(m, G, ncu, mw, npad) not in lc.UNREACHABLE
    # the whole-matrix back substitution at its largest LDS request: 8160 rows, under the 152 KB the kernel is granted
    assert lc.backsolve_form(8160, 1) == {"backsolve:whole"}
    assert lc.backsolve_lds_bytes(8160, 1) == 16 * (8160 + 32 * 33 + 64) <= 152 * 1024
    assert lc.backsolve_form(8192, 1) == {"backsolve:blocked"} and lc.backsolve_form(8192, 65) == {"backsolve:whole"}
    assert lc.backsolve_form(8224, 1) == {"backsolve:blocked", "backsolve:blocked+short_top"} and 8224 % 256 == 32
    assert lc.backsolve_form(9024, 1) >= {"backsolve:blocked+short_top"} and 9024 % 256 == 64


def test_restated_plan_shapes():
    """Spot checks of the restatement against csrc/lu.hip read by hand."""
    panels, trsms, gemms = lc.factor_plan(224)
    assert panels == list(range(224, 0, -16))
    assert sorted(set(trsms)) == [1, 2, 3, 7]                       # 224 = 112 + 112, 112 = 48 + 64, 48 = 16 + 32, 64 = 32 + 32
    assert lc.trsm_blocks(96) >= {"trsm<3>"} and lc.trsm_blocks(160) >= {"trsm<5>"} and lc.trsm_blocks(192) >= {"trsm<6>"}
    assert lc.trsm_blocks(224, 96) >= {"trsm<6>", "trsm<3>", "trsm<2>"}
    assert lc.trsm_blocks(1024) == {"trsm<1>", "trsm<2>", "trsm<4>", "trsm<8>"}
    # update kernels with at most 32 rows: the last outer panels of every case
    assert any(M <= 32 for M, N, K in gemms)
    # blocked back substitution: N = 1 products are not part of the factorisation plan
    assert all(N >= 16 for M, N, K in lc.factor_plan(2048)[2])
    assert lc.panel_variant(2080, 1, 256, True, 2080) == "mw<1>" and lc.panel_variant(2080, 1, 256, False, 2080) == "ip<8,4>"
    assert lc.panel_variant(4128, 1, 256, True, 4128) == "mw<2>" and lc.panel_variant(4128, 1, 256, False, 4128) == "ip<16,2>"
    assert lc.panel_variant(1056, 3, 256, True, 1056) == "mw<1>" and lc.panel_variant(1056, 3, 256, False, 1056) == "ip<4,8>"
    assert lc.panel_variant(1056, 200, 256, True, 1056) == "ip<4,8>"          # G > CUs / 2: no room for two workgroups each
    assert lc.panel_variant(8224, 1, 256, True, 8224) == "ip<32,1>" and lc.panel_variant(8192, 1, 256, True, 8224) == "ip<16,2>"
