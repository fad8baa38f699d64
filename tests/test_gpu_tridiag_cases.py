"""The device tridiagonal eigen-solver (csrc/herm.hip: tri_bisect_kernel, tri_twisted_kernel, tri_scale_kernel,
tri_resid_kernel, tri_solve) on the adversarial table of tests/tridiag_cases.py: eigenvalues bit for bit against the NumPy
restatement and certified in 50-digit arithmetic, the three diagnostics held to what they claim about the returned (w, Z), the
verdict of engine.device_eigh's acceptance rule, the vectors Z themselves, state between calls, and the rule through the engine.

Z is read without a new export: the reduction of a real diagonal matrix has tau = 0 in every reflector, so the
back-transformation of the vectors herm_tridiag_eig left on the device subtracts exact zeros and get_eigvecs() returns
Z + 0i (test_backtransform_through_a_diagonal_matrix_is_the_identity).  No bound here comes from a device run: see
tridiag_cases.py and test_tridiag_cases_host.py."""
import numpy as np
import pytest

import tridiag_cases as tc

pytestmark = pytest.mark.gpu
EPS = tc.EPS
SIZES = sorted({c[1].shape[0] for c in tc.CASES})


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def engine():
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    eng = DeviceEngine(0, eigh_mode="device")
    yield eng
    eng.ctx.close()


def _bind_diagonal(ctx, n):
    ctx.set_matrix(np.diag(np.arange(1.0, n + 1.0)).astype(np.complex128))
    d, e = ctx.herm_tridiag()
    assert np.array_equal(d, np.arange(1.0, n + 1.0)) and not e.any()


def _scaled_eig(ctx, d, e):
    """maus_herm_tridiag_eig on the scaled matrix, as Context.herm_tridiag_eig calls it, but returning the eigenvalues before
    the final w * s (which rounds when T is subnormal): (ws, (gap, resid, tnorm of the scaled matrix))."""
    from adaptive_matrix_solver_amd._cabi import _ptr
    n, ds, es, s = ctx._scaled_tridiagonal(d, e)
    ws, diag = np.empty(n), np.empty(3)
    ctx._ck(ctx.lib.maus_herm_tridiag_eig(ctx.h, _ptr(ds), _ptr(es), n, _ptr(ws), _ptr(diag)), "maus_herm_tridiag_eig")
    return ws, tuple(float(x) for x in diag), s


def _solve(ctx, name):
    """The case on the device: the result as a tridiag_cases.Result, Z read through the diagonal matrix's back-transformation."""
    _, d, e, _ = tc.BY_NAME[name]
    n = d.shape[0]
    ws, sdiag, s = _scaled_eig(ctx, d, e)
    _bind_diagonal(ctx, n)
    w, diag = ctx.herm_tridiag_eig(d, e)
    ctx.herm_backtransform(None)
    V = ctx.get_eigvecs()
    assert not V.imag.any()
    assert np.array_equal(w, ws * s) and diag == (sdiag[0], sdiag[1], sdiag[2] * s), (name, diag, sdiag)
    return tc.Result(w, diag, np.ascontiguousarray(V.real), ws, s, sdiag[2])


@pytest.fixture(scope="module")
def solved(ctx):
    """Every case once, in table order; not to be modified."""
    out = {name: _solve(ctx, name) for name in tc.NAMES}
    for r in out.values():
        for a in (r.w, r.Z, r.ws):
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_backtransform_through_a_diagonal_matrix_is_the_identity(ctx, n):
    rng = np.random.default_rng(n)
    Z0 = rng.standard_normal((n, n))
    _bind_diagonal(ctx, n)
    ctx.herm_backtransform(Z0)
    V = ctx.get_eigvecs()
    assert np.array_equal(V.real, Z0) and not V.imag.any()


@pytest.mark.parametrize("name", tc.NAMES)
def test_eigenvalues_bit_for_bit(ctx, solved, name):
    """The bisection contains no product that feeds a sum and fp64 division is correctly rounded: the device must return the
    restatement's bits, with and without vectors, and the same ||T||."""
    _, d, e, _ = tc.BY_NAME[name]
    ref, got = tc.restated(name), solved[name]
    diff = np.flatnonzero(got.ws != ref.ws)
    assert diff.size == 0, (name, diff[:8], got.ws[diff[:8]], ref.ws[diff[:8]])
    assert np.array_equal(got.w, ref.w)
    assert np.array_equal(ctx.herm_tridiag_eigvals(d, e), got.w)
    assert got.diag[2] == ref.diag[2] and got.diag[0] == ref.diag[0]


@pytest.mark.parametrize("name", tc.NAMES)
def test_device_result_meets_every_check(solved, name):
    """Independent of the restatement: finite output, eigenvalues certified within the bar and within it of the closed forms,
    gap = min diff(w) / ||T|| exactly, resid within 16 eps of the long-double residual of the returned (w, Z), the tabled
    verdict; accepted cases: residual, norms, orthogonality eps / gap, angle to the known vectors (tridiag_cases.check_result)."""
    print(tc.check_result(name, solved[name]))


@pytest.mark.parametrize("name", tc.REJECTED)
def test_rejected_case_leaves_no_state(ctx, solved, name):
    """A rejected case, then an accepted one of another order on the same context: the accepted case's bits, vectors included
    (the n x n work arrays and the vectors left on the device are released and rebuilt)."""
    bad = _solve(ctx, name)
    assert np.array_equal(bad.w, solved[name].w) and np.isfinite(bad.Z).all()
    for other in ("clement_n40", "pair_n2"):
        good = _solve(ctx, other)
        assert good.verdict == "device"
        assert np.array_equal(good.w, solved[other].w) and np.array_equal(good.Z, solved[other].Z) and good.diag == solved[other].diag


def test_eigenvalues_do_not_depend_on_what_ran_before(ctx, solved):
    for order in (tc.NAMES[::-1], tc.NAMES[1::2] + tc.NAMES[::2]):
        for name in order:
            _, d, e, _ = tc.BY_NAME[name]
            w, diag = ctx.herm_tridiag_eig(d, e)
            assert np.array_equal(w, solved[name].w) and diag == solved[name].diag, name


# ---- through the engine -----------------------------------------------------------------------------------------------------
def _dense(d, e):
    return (np.diag(d) + np.diag(e, 1) + np.diag(e, -1)).astype(np.complex128)


def _decomposition_figures(d, e, w, V):
    """max |T V - V w| in long double from the three diagonals: no product underflows, even at 1e-310."""
    ld, cld = np.longdouble, np.clongdouble
    Vl = V.astype(cld)
    R = d.astype(ld)[:, None] * Vl - Vl * np.asarray(w).astype(ld)[None, :]
    R[1:] += e.astype(ld)[:, None] * Vl[:-1]
    R[:-1] += e.astype(ld)[:, None] * Vl[1:]
    return np.abs(R).max()


@pytest.mark.parametrize("name", [c[0] for c in tc.CASES if c[1].shape[0] >= 2])
def test_acceptance_rule_through_the_engine(engine, name):
    _, d, e, verdict = tc.BY_NAME[name]
    n = d.shape[0]
    w = engine.device_eigh(_dense(d, e))
    assert np.array_equal(engine.tridiag_de[0], d) and np.array_equal(engine.tridiag_de[1], e)   # T comes back unchanged
    assert engine.tridiag_solver == verdict, (engine.tridiag_solver, engine.tridiag_diag)
    gap, resid, tnorm = engine.tridiag_diag
    V = engine.ctx.get_eigvecs()
    assert np.isfinite(w).all() and np.isfinite(V).all()
    r = tc.restated(name)
    anorm = np.longdouble(np.abs(r.ws[[0, -1]]).max()) * np.longdouble(r.s)      # ||T||_2 of a symmetric T (certified spectrum)
    # (the floor of the certificate: the bisection's 2 pivmin, which is all of the zero matrix's w = -safmin, and the rounding
    # of w itself when T is subnormal)
    assert _decomposition_figures(d, e, w, V) <= 60 * n * EPS * anorm + tc.abs_floor(d, e)
    orth = np.abs(V.conj().T @ V - np.eye(n)).max()
    assert orth <= (max(50 * EPS / gap, 1e3 * EPS) if verdict == "device" else 1e-12), (orth, gap)
    assert np.abs(V[0].imag).max() == 0.0
    assert tc.certified(d, e, w, tc.CERT_BAR)
    # the bisection's eigenvalues under either verdict: a spectrum rejected for its gap takes only the vectors from dstemr
    # (whose own eigenvalues need 8 eps ||T|| on wilkinson21 and glued_wilkinson_n63, twice the bar)
    assert np.array_equal(w, r.w)


def test_residual_rejection_through_the_engine(engine, monkeypatch):
    """No finite input reached resid > TRIDIAG_MAX_RESID through the kernels; the branch is taken here by reporting 1e-12."""
    _, d, e, _ = tc.BY_NAME["clement_n40"]
    real = engine.ctx.herm_tridiag_eig
    calls = []

    def reports_a_residual(dd, ee):
        w, (gap, resid, tnorm) = real(dd, ee)
        calls.append(resid)
        return w, (gap, 1e-12, tnorm)
    monkeypatch.setattr(engine.ctx, "herm_tridiag_eig", reports_a_residual)
    w = engine.device_eigh(_dense(d, e))
    assert calls and calls[0] <= tc.MAX_RESID and engine.tridiag_solver == "host" and engine.tridiag_diag[1] == 1e-12
    V = engine.ctx.get_eigvecs()
    assert _decomposition_figures(d, e, w, V) <= 60 * 40 * EPS * engine.tridiag_diag[2]
    assert np.abs(V.conj().T @ V - np.eye(40)).max() <= 1e-12
    assert np.abs(w - np.arange(-39.0, 40.0, 2.0)).max() <= 64 * EPS * engine.tridiag_diag[2]      # dstemr's, as test_gpu_herm_eigh.py


# ---- rejected arguments -----------------------------------------------------------------------------------------------------
class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after a rejected argument")


@pytest.mark.parametrize("bad", ["nan_d", "inf_d", "nan_e", "inf_e", "long_e", "short_e"])
def test_bad_arguments_are_rejected_before_any_launch(ctx, monkeypatch, bad):
    d, e = np.arange(1.0, 7.0), np.ones(5)
    if bad.endswith("_d"):
        d[3] = np.nan if bad.startswith("nan") else np.inf
    elif bad in ("nan_e", "inf_e"):
        e[2] = np.nan if bad.startswith("nan") else -np.inf
    else:
        e = np.ones(6 if bad == "long_e" else 4)
    monkeypatch.setattr(ctx, "lib", _NoCalls())
    for call in (ctx.herm_tridiag_eig, ctx.herm_tridiag_eigvals):
        with pytest.raises(ValueError):
            call(d, e)


def test_vectors_of_another_order_are_not_back_transformed(ctx, solved):
    from adaptive_matrix_solver_amd._cabi import MausHipError
    _, d, e, _ = tc.BY_NAME["repeated_diagonal_n5"]
    _bind_diagonal(ctx, 8)
    ctx.herm_tridiag_eig(d, e)
    with pytest.raises(MausHipError, match="null input and no eigenvectors of T on the device"):
        ctx.herm_backtransform(None)
    good = _solve(ctx, "diagonal_n8")                               # the context is as good as before
    assert np.array_equal(good.w, solved["diagonal_n8"].w) and np.array_equal(good.Z, solved["diagonal_n8"].Z)
