"""The stages of the Hermitian reduction on the device (csrc/herm.hip), separated: maus_herm_tridiag gives (d, e),
maus_herm_backtransform(I) gives Q itself, and tests/herm_cases.py holds both to A_L = Q T Q^H, Q^H Q = I (check A, in extended
precision against LAPACK's own values on the same matrix and probes), to zhetrd's conventions (check B) and to the exact
statements of the structured cases -- at the edges of the 64-column panel, the 64 x 64 tile grid, the 1024-column strips of the
rank-128 update and the blocks of the back-transformation, and with 8 and 16 tiles per workgroup forced at the smallest orders
where a block row has two chunks (maus_herm_set_chunk), which the rule reaches only from n ~ 6600 and n ~ 9100 up.
tests/test_herm_cases_host.py shows on the CPU that the same checks pass for LAPACK and fail for seven planted faults."""
import numpy as np
import pytest

import herm_cases as hc
import scenarios

pytestmark = pytest.mark.gpu
EPS = hc.EPS


@pytest.fixture()
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


def _reduce(c, A, chunk=0):
    n = A.shape[0]
    c.herm_set_chunk(chunk)
    c.set_matrix(A)
    d, e = c.herm_tridiag()
    c.herm_backtransform(np.eye(n))
    return d.copy(), e.copy(), c.get_eigvecs()


def _fresh(A, chunk=0):
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    try:
        return _reduce(c, A, chunk)
    finally:
        c.close()


@pytest.mark.parametrize("name", hc.NAMES)
def test_case_table_on_the_device(ctx, name):
    hc.run_case(name, lambda A, chunk: _reduce(ctx, A, chunk))


def test_every_chunk_size_on_one_matrix(ctx):
    """4, 8 and 16 tiles per workgroup at n = 1100 (two chunks in the last block rows at 8 and at 16): each passes checks A and
    B; their d and e agree to 64 n eps ||A|| -- not bit for bit, the order of summation differs."""
    name = "chunk16_n1100"
    A = hc.matrix(name)
    n = A.shape[0]
    anorm = hc.probe_and_lapack(name)[0].anorm
    out = {}
    for h in (4, 8, 16):
        assert [ctx.herm_chunk_plan(n, 0, h)[1], ctx.herm_chunk_plan(n, n - 2, h)[1]] == [h, h]
        d, e, Q = _reduce(ctx, A, h)
        hc.check_b(A, d, e, Q)
        hc.check_a(name, d, e, Q)
        out[h] = (d, e)
    # the default is the rule, and the rule gives 4 here
    d0, e0, _ = _reduce(ctx, A, 0)
    assert hc.bits(d0, e0) == hc.bits(*out[4])
    for a, b in ((4, 8), (4, 16), (8, 16)):
        assert np.abs(out[a][0] - out[b][0]).max() <= 64 * n * EPS * anorm
        # the sign of e is fixed by zlarfg from Re alpha, which is far from zero for all but the rare column: compare as it is
        assert np.abs(out[a][1] - out[b][1]).max() <= 64 * n * EPS * anorm


def test_scaling_law_on_both_sides_of_the_range_edges(ctx):
    """The work copy is scaled when the largest entry lies outside [2^-400, 2^400) (herm.hip): just inside the squares are
    still safe unscaled, just outside the factor applies -- the law of `scaled` holds on either side of both edges."""
    import math
    A = hc.matrix("scaled")
    low = np.tril(A)
    ex0 = math.frexp(max(np.abs(low.real).max(), np.abs(low.imag).max()))[1] - 1
    d, e, Q = _reduce(ctx, A)
    for ex in (-402, -401, -400, 399, 400, 401):
        s = 2.0 ** (ex - ex0)                                        # the largest entry of s A lies in [2^ex, 2^(ex + 1))
        ds, es, Qs = _reduce(ctx, A * s)
        assert np.array_equal(ds, d * s) and np.array_equal(es, e * s), ex
        assert hc.bits(Qs) == hc.bits(Q), ex


def test_set_chunk_rejects_other_values(ctx):
    from adaptive_matrix_solver_amd._cabi import MausHipError
    for bad in (-1, 1, 2, 3, 5, 12, 32):
        with pytest.raises(MausHipError, match="tiles must be 0"):
            ctx.herm_set_chunk(bad)
    for ok in (4, 8, 16, 0):
        ctx.herm_set_chunk(ok)


def test_nan_in_the_lower_triangle_returns_and_leaves_no_trace(ctx):
    n = 200
    A = hc.matrix("lower_only")
    B = A.copy()
    B[150, 20] = complex(np.nan, 0.0)
    ctx.set_matrix(B)
    d, e = ctx.herm_tridiag()
    assert np.isnan(d).any() and np.isnan(e).any()
    ctx.herm_release()
    assert hc.bits(*_reduce(ctx, A)) == hc.bits(*_fresh(A))


def test_decompositions_are_reproducible_across_other_orders(ctx):
    """The per-call buffers are not cleared: a read of a slot nobody wrote would show as a difference after a decomposition of
    another order."""
    A, B = hc.matrix("random_n130"), hc.matrix("random_n321")
    first = hc.bits(*_reduce(ctx, A))
    assert hc.bits(*_reduce(ctx, A)) == first
    big = hc.bits(*_reduce(ctx, B))
    assert hc.bits(*_reduce(ctx, A)) == first
    assert hc.bits(*_reduce(ctx, B)) == big


def test_c_and_fortran_ordered_z_give_the_same_bits(ctx):
    n = 130
    A = hc.matrix("random_n130")
    Z = np.random.default_rng(8).standard_normal((n, n))
    V = []
    for z in (np.ascontiguousarray(Z), np.asfortranarray(Z)):
        ctx.set_matrix(A)
        ctx.herm_tridiag()
        ctx.herm_backtransform(z)
        V.append(ctx.get_eigvecs())
    assert hc.bits(V[0]) == hc.bits(V[1])


def test_backtransform_needs_reflectors(ctx):
    from adaptive_matrix_solver_amd._cabi import MausHipError
    n = 66
    A = hc.matrix("random_n66")
    ctx.set_matrix(A)
    ctx.herm_tridiag()
    ctx.herm_release()
    with pytest.raises(MausHipError, match="no reflectors"):
        ctx.herm_backtransform(np.eye(n))
    ctx.herm_tridiag()
    ctx.herm_backtransform(np.eye(n))
    with pytest.raises(MausHipError, match="no reflectors"):         # the reflectors are good for one back-transformation
        ctx.herm_backtransform(np.eye(n))
