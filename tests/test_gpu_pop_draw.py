"""Candidate vectors drawn on the device from NumPy's MT19937 stream (maus_pop_draw, vector_draws='device'; GPU only).

The draws themselves are held to NumPy's bits (np.array_equal with np.random.rand from the same state); everything that
passes through the norm is held to bounds derived from the arithmetic, N = vector length, u = 2^-53:
  * norm_out against sqrt(math.fsum(|v_i|^2)): a sum of 2N non-negative terms in any order is within (2N - 1) u of the exact
    sum, the root halves that and adds one rounding, the squares add one each: (N + 2) u relative;
  * a component of a UNIT row against the host's v / np.linalg.norm(v): two roots of sums of 2N non-negative terms in two
    orders ((N + 1) u each), one reciprocal and two products on either side: (2N + 8) u relative.
"""
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RAW, UNIT, NORM = 0, 1, 2
MIN_N = 1024


@pytest.fixture(scope="module")
def ctx():
    from adaptive_matrix_solver_amd import Context
    c = Context(0)
    yield c
    c.close()


def _bind(ctx, n, cap):
    import scipy.sparse as sp
    if (ctx.rows, ctx.cols) != (n, n):
        ctx.set_matrix_csr(sp.identity(n, format="csr", dtype=np.complex128))
    ctx.pop_reserve(cap)


def _set_pos(seed, pos):
    """The global stream at word `pos` of a block: 624 = freshly seeded, 1 = after one np.random.randint (a double's two words
    no longer sit at an even position), 623 = a double straddles the block."""
    np.random.seed(seed)
    if pos == 1:
        np.random.randint(0, 16)                       # a power of two: no rejection, exactly one word
    elif pos != 624:
        np.random.bytes(4 * pos)
    assert np.random.get_state()[2] == pos
    return np.random.get_state()


def _host_pairs(state, n, npairs):
    np.random.set_state(state)
    out = np.empty((npairs, n), dtype=np.complex128)
    for k in range(npairs):
        out[k] = np.random.rand(n) + 1j * np.random.rand(n)
    return out


def _fsum_norm(v):
    return math.sqrt(math.fsum((v.real * v.real).tolist() + (v.imag * v.imag).tolist()))


def _sentinel(ctx, rows, n):
    g = np.random.default_rng(7)
    S = g.standard_normal((rows, n)) + 1j * g.standard_normal((rows, n))
    ctx.pop_put(0, np.arange(rows), S)
    return S


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("pos", [624, 1, 312, 623])
@pytest.mark.parametrize("n", [MIN_N, MIN_N + 1, 4368, 4369])
def test_raw_rows_are_numpys_draws(ctx, n, pos):
    """Ordinals with gaps, slots scrambled and apart, a guard row on either side of each."""
    rows = 9
    _bind(ctx, n, rows)
    S = _sentinel(ctx, rows, n)
    state = _set_pos(100 + n, pos)
    ords, slots = np.array([0, 2, 5]), np.array([5, 1, 7])
    host = _host_pairs(state, n, 6)
    norms = ctx.pop_draw(0, n, slots, [RAW] * 3, None, state, ords)
    X = ctx.pop_get(0, np.arange(rows), n)
    for k in range(3):
        assert np.array_equal(X[slots[k]], host[ords[k]]), (k, "bits differ from np.random.rand")
        ref = _fsum_norm(host[ords[k]])
        assert abs(norms[k] - ref) <= (n + 2) * U * ref
    for r in set(range(rows)) - set(slots.tolist()):
        assert _same(X[r], S[r]), f"row {r} was touched"


@pytest.mark.parametrize("count", [1, 15, 17, 64, 130])
def test_raw_draw_counts(ctx, count):
    """130 pairs: draw indices above 256, a third hexadecimal digit of the lifting."""
    n = MIN_N
    rows = 2 * count + 1
    _bind(ctx, n, rows)
    S = _sentinel(ctx, rows, n)
    state = _set_pos(55, 312)
    host = _host_pairs(state, n, count)
    slots = (2 * np.arange(count) + 1)[::-1].copy()
    ctx.pop_draw(0, n, slots, [RAW] * count, None, state, np.arange(count))
    X = ctx.pop_get(0, np.arange(rows), n)
    assert np.array_equal(X[slots], host)
    assert _same(X[0::2], S[0::2])


def test_forced_substreams_and_batch_independence(ctx):
    """N = 65536: the same RAW bits and the same UNIT bits under the rule and under 1, 2, 5 and 64 forced sub-streams; a UNIT
    row alone, among 15 and among 64 (N = 4369)."""
    n = 65536
    _bind(ctx, n, 4)
    state = _set_pos(9, 623)
    host = _host_pairs(state, n, 4)
    unit0 = None
    for S in (0, 1, 2, 5, 64):
        ctx.pop_draw(0, n, [2, 0], [RAW, RAW], None, state, [1, 3], substreams=S)
        X = ctx.pop_get(0, [2, 0], n)
        assert np.array_equal(X, host[[1, 3]]), S
        nr = ctx.pop_draw(0, n, [1, 3], [UNIT, UNIT], [1.0, 2.5], state, [1, 3], substreams=S)
        Xu = ctx.pop_get(0, [1, 3], n)
        if unit0 is None:
            unit0 = (Xu, nr)
        assert _same(Xu, unit0[0]) and _same(nr, unit0[1]), S
    n = 4369
    _bind(ctx, n, 64)
    state = _set_pos(10, 1)
    ctx.pop_draw(0, n, [5], [UNIT], [0.7], state, [3])
    alone = ctx.pop_get(0, [5], n)[0]
    for count in (15, 64):
        sc = np.linspace(0.1, 10.0, count)
        sc[3] = 0.7
        ctx.pop_draw(0, n, np.arange(count)[::-1].copy(), [UNIT] * count, sc, state, np.arange(count))
        assert _same(ctx.pop_get(0, [count - 1 - 3], n)[0], alone), count


def test_engine_call_advances_the_host_stream(ctx):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    n, count = 4369, 5
    _bind(ctx, n, count)
    eng = DeviceEngine(ctx=ctx)
    state = _set_pos(77, 1)
    host = _host_pairs(state, n, count)                # leaves the stream where the host draws end
    end = np.random.get_state()
    nxt = np.random.rand(5)
    np.random.set_state(state)
    eng.draw_vectors(n, np.arange(count), [RAW] * count)
    got = np.random.get_state()
    assert np.array_equal(got[1], end[1]) and got[2] == end[2]
    assert np.array_equal(np.random.rand(5), nxt)
    assert np.array_equal(ctx.pop_get(0, np.arange(count), n), host)


@pytest.mark.parametrize("n", [MIN_N, 4369, 65536])
def test_unit_rows_and_norms(ctx, n, capsys):
    _bind(ctx, n, 6)
    S = _sentinel(ctx, 6, n)
    state = _set_pos(3 + n, 624)
    host = _host_pairs(state, n, 3)
    scale = np.array([1.0, 0.37, 9.25])
    norms = ctx.pop_draw(0, n, [0, 2, 4], [UNIT] * 3, scale, state, [0, 1, 2])
    X = ctx.pop_get(0, np.arange(6), n)
    norms1 = ctx.pop_draw(0, n, [0, 2, 4], [UNIT] * 3, None, state, [0, 1, 2])
    X1 = ctx.pop_get(0, np.arange(6), n)
    worst_c = worst_n = 0.0
    for k in range(3):
        ref = host[k] / np.linalg.norm(host[k])
        got = X1[2 * k]
        err = max(np.max(np.abs(got.real - ref.real) / np.abs(ref.real)), np.max(np.abs(got.imag - ref.imag) / np.abs(ref.imag)))
        fs = _fsum_norm(host[k])
        nerr = abs(norms[k] - fs) / fs
        worst_c, worst_n = max(worst_c, err), max(worst_n, nerr)
        # with a scale: the unit row times the scale, component by component, exactly
        assert _same(X[2 * k].real, X1[2 * k].real * scale[k]) and _same(X[2 * k].imag, X1[2 * k].imag * scale[k])
    with capsys.disabled():
        print(f"\n[pop_draw] n={n}: max component error {worst_c / U:.1f} u (bound {2 * n + 8}), max norm error {worst_n / U:.2f} u (bound {n + 2})")
    assert worst_c <= (2 * n + 8) * U
    assert worst_n <= (n + 2) * U
    assert _same(norms, norms1)                        # the norm before scaling
    assert _same(X[1::2], S[1::2]) and _same(X1[1::2], S[1::2])


def test_norm_kind_writes_nothing(ctx):
    n = 4369
    _bind(ctx, n, 4)
    S = _sentinel(ctx, 4, n)
    state = _set_pos(31, 312)
    np.random.set_state(state)
    np.random.rand(n); np.random.rand(n)
    scale = 0.1 + 0.5
    v_pert = (np.random.rand(n) - 0.5 + 1j * (np.random.rand(n) - 0.5)) * scale          # pair 1 of the stream
    norms = ctx.pop_draw(0, n, [-1, 2], [NORM, NORM], [scale, scale], state, [1, 1])
    ref = _fsum_norm(v_pert)
    assert abs(norms[0] - ref) <= (n + 2) * U * ref and norms[0] == norms[1]
    assert abs(norms[0] - np.linalg.norm(v_pert)) <= (2 * n + 8) * U * ref
    assert _same(ctx.pop_get(0, np.arange(4), n), S)


def test_refusals(ctx):
    from adaptive_matrix_solver_amd import _cabi
    _bind(ctx, 4369, 4)
    state = _set_pos(1, 624)
    assert ctx.pop_draw_min_len() == MIN_N
    with pytest.raises(_cabi.MausHipError):
        ctx.pop_draw(0, MIN_N - 1, [0], [RAW], None, state, [0])
    with pytest.raises(_cabi.MausHipError):
        ctx.pop_draw(0, 4370, [0], [RAW], None, state, [0])          # longer than a row
    with pytest.raises(_cabi.MausHipError):
        ctx.pop_draw(0, 4369, [0], [7], None, state, [0])
    with pytest.raises(_cabi.MausHipError):
        ctx.pop_draw(0, 4369, [4], [RAW], None, state, [0])          # slot out of range
    with pytest.raises(_cabi.MausHipError):
        ctx.pop_draw(0, 4369, [0], [RAW], None, state, [0], substreams=65)


# ---- MAUS_Solver under vector_draws='device' against 'host' ---------------------------------------------------------------
def _digests():
    import snapshot
    return snapshot.rng_digest()


class _Counting:
    """Counts pop_get / pop_put of a context while active."""
    def __init__(self, ctx):
        self.ctx, self.gets, self.puts = ctx, 0, 0

    def __enter__(self):
        c = self.ctx
        self._g, self._p = c.pop_get, c.pop_put

        def get(*a, **k):
            self.gets += 1
            return self._g(*a, **k)

        def put(*a, **k):
            self.puts += 1
            return self._p(*a, **k)
        c.pop_get, c.pop_put = get, put
        return self

    def __exit__(self, *exc):
        del self.ctx.pop_get, self.ctx.pop_put


def _make_solver(kind, mode):
    import scipy.sparse as sp
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(21); random.seed(21); SolutionCandidate._candidate_id_counter = 0
    g = np.random.default_rng(4)
    if kind == "lin":
        n = 4096
        A = sp.diags([g.standard_normal(n - 1), 4.0 + g.standard_normal(n), g.standard_normal(n - 1)], [-1, 0, 1], format="csr").astype(np.complex128)
        b = g.standard_normal(n) + 0j
        diag = {"is_sparse_init": True, "condition_number": 1e3, "is_singular": False, "is_hermitian": False, "is_complex_symmetric": False}
        return MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=b, initial_num_candidates=8, quiet=True, gmres_compat="scipy-legacy",
                           sparse_mode="device", sparse_direct="narrow", diag_info=diag, vector_draws=mode)
    n = 1024
    A = (g.standard_normal((n, n)) + 1j * g.standard_normal((n, n))) / np.sqrt(2 * n)
    diag = {"is_sparse_init": False, "condition_number": 1e3, "is_singular": False, "is_hermitian": False, "is_complex_symmetric": False}
    return MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=16, quiet=True, diag_info=diag, vector_draws=mode)


def _run(kind, mode, iters=3):
    s = _make_solver(kind, mode)
    rows = []
    for it in range(iters):
        s.loop_body(it + 1)
        rows.append(([(c.id, c.state.value, c.stuck_counter, c.local_psi_retries_needed) for c in s.candidates], _digests(),
                     [float(c.residual_k) for c in s.candidates],
                     [complex(c.lambda_k) if c.lambda_k is not None else 0j for c in s.candidates]))
    first = [c.param_history[0] for c in s.candidates[:4]]
    return s, rows, first


_RUNS = {}


def _runs(kind):
    if kind not in _RUNS:
        _RUNS[kind] = (_run(kind, "host"), _run(kind, "device"))
    return _RUNS[kind]


@pytest.mark.parametrize("kind", ["lin", "eig"])
def test_solver_loop_bodies(kind, capsys):
    (s0, rows0, _), (s1, rows1, _) = _runs(kind)
    assert s1.engine.vector_draws == "device" and s0.engine.vector_draws == "host"
    worst = 0.0
    for (b0, d0, r0, l0), (b1, d1, r1, l1) in zip(rows0, rows1):
        assert b0 == b1                                # ids in list order, states, stuck and retry counters
        assert d0 == d1                                # both RNG streams
        for x, y in zip(r0 + l0, r1 + l1):
            if np.isfinite(x) or np.isfinite(y):
                worst = max(worst, abs(x - y) / max(abs(x), 1e-300))
    with capsys.disabled():
        print(f"\n[pop_draw] {kind}: worst relative difference of residuals / lambda over three bodies {worst:.3e} (bound 1e-9)")
    assert worst <= 1e-9


@pytest.mark.parametrize("kind", ["lin", "eig"])
def test_first_history_entry_is_the_drawn_vector(kind):
    """param_history[0], read after three steps of the row, within the UNIT bound of the host's."""
    (s0, _, f0), (s1, _, f1) = _runs(kind)
    n = s0.N_diag
    for h, d in zip(f0, f1):
        assert len(h) == len(d)
        if kind == "eig":
            assert h[0] == d[0]
        vh, vd = h[-1], d[-1]
        assert np.max(np.abs(vd.real - vh.real) / np.abs(vh.real)) <= (2 * n + 8) * U
        assert np.max(np.abs(vd.imag - vh.imag) / np.abs(vh.imag)) <= (2 * n + 8) * U


def _spawn(mode):
    s = _make_solver("eig", mode)
    n = s.N_diag
    g = np.random.default_rng(12)
    v = g.standard_normal(n) + 1j * g.standard_normal(n)
    v /= np.linalg.norm(v)
    s.converged_solutions = [(0.3 + 0.1j, v)]
    s.num_distinct_converged_solutions = 1
    s.landscape_energy = 0.5
    with _Counting(s.engine.ctx) as cnt:
        s._manage_candidates(1)
    born = [c for c in s.candidates if c.id >= 16]               # the initial population holds ids 0..15
    out = ([c.id for c in born], [complex(c.lambda_k) for c in born], _digests(), cnt.gets, cnt.puts)
    return out, [np.array(c.v_k) for c in born]


def test_spawn_from_a_converged_base():
    (ids0, lam0, dig0, _, puts0), V0 = _spawn("host")
    (ids1, lam1, dig1, gets1, puts1), V1 = _spawn("device")
    n = 1024
    assert len(ids0) == 15 and ids0 == ids1 and lam0 == lam1 and dig0 == dig1
    assert puts0 >= 1 and puts1 == 0 and gets1 == 0          # no row crossed the bus under 'device'
    for a, b in zip(V0, V1):
        assert np.max(np.abs(b.real - a.real) / np.abs(a.real)) <= (2 * n + 8) * U
        assert np.max(np.abs(b.imag - a.imag) / np.abs(a.imag)) <= (2 * n + 8) * U


def test_construction_makes_no_transfers_under_device():
    from adaptive_matrix_solver_amd import _cabi
    orig_get, orig_put = _cabi.Context.pop_get, _cabi.Context.pop_put
    calls = {"get": 0, "put": 0}

    def get(self, *a, **k):
        calls["get"] += 1
        return orig_get(self, *a, **k)

    def put(self, *a, **k):
        calls["put"] += 1
        return orig_put(self, *a, **k)
    _cabi.Context.pop_get, _cabi.Context.pop_put = get, put
    try:
        s = _make_solver("lin", "device")
    finally:
        _cabi.Context.pop_get, _cabi.Context.pop_put = orig_get, orig_put
    assert calls == {"get": 0, "put": 0}
    assert all(c._dev_valid and not c._host_valid for c in s.candidates)
