"""The host side of vector_draws='device' without a GPU: a NumPy double of maus_pop_draw (a subclass of the fake context) drives
the bracket of DeviceEngine -- registration, the one draw call, the jump of the host stream, the first history entries -- and
the replay on the host of a draw whose norm test the device norms do not decide (AMS:131, AMS:546)."""
import random

import numpy as np
import pytest

import snapshot
from fake_ctx import FakeContext

N, P = 1024, 6
RAW, UNIT, NORM = 0, 1, 2


class DrawContext(FakeContext):
    """FakeContext + pop_draw as include/maus_hip.h states it, with NumPy's own draws and norm.  zero_norm = (call, draw):
    that draw of that call reports a norm of 0 (what a degenerate draw would)."""

    def __init__(self, zero_norm=None):
        super().__init__()
        self.zero_norm = zero_norm
        self.draw_calls = []
        self.puts = 0

    def pop_draw_min_len(self):
        return 1024

    def pop_put(self, which, slots, vecs):
        self.puts += 1
        return super().pop_put(which, slots, vecs)

    def pop_draw(self, which, length, slots, kinds, scale, state, ordinals, substreams=0):
        saved = np.random.get_state()
        norms = np.zeros(len(slots))
        for k, (s, kind, o) in enumerate(zip(slots, kinds, ordinals)):
            np.random.set_state(state)
            for _ in range(int(o)):
                np.random.rand(length); np.random.rand(length)
            u1, u2 = np.random.rand(length), np.random.rand(length)
            sc = 1.0 if scale is None else float(scale[k])
            if kind == NORM:
                norms[k] = np.linalg.norm((u1 - 0.5 + 1j * (u2 - 0.5)) * sc)
            else:
                v = u1 + 1j * u2
                norms[k] = np.linalg.norm(v)
                self.pop[which][s, :length] = v if kind == RAW else v * (1.0 / norms[k]) * sc
            if self.zero_norm == (len(self.draw_calls), k):
                norms[k] = 0.0
        np.random.set_state(saved)
        self.draw_calls.append((len(slots), list(kinds)))
        return norms


def _solver(kind, mode, ctx):
    from adaptive_matrix_solver_amd.engine import DeviceEngine
    from adaptive_matrix_solver_amd.solver import MAUS_Solver, ProblemType, SolutionCandidate
    np.random.seed(33); random.seed(33); SolutionCandidate._candidate_id_counter = 0
    g = np.random.default_rng(1)
    A = (g.standard_normal((N, N)) + 1j * g.standard_normal((N, N))) / np.sqrt(2 * N)
    diag = {"is_sparse_init": False, "condition_number": 1e3, "is_singular": False, "is_hermitian": False, "is_complex_symmetric": False}
    eng = DeviceEngine(ctx=ctx, vector_draws=mode)
    if kind == "lin":
        return MAUS_Solver(A, ProblemType.SOLVE_LINEAR_SYSTEM, b_vector=g.standard_normal(N) + 0j, initial_num_candidates=P, quiet=True,
                           diag_info=diag, engine=eng)
    return MAUS_Solver(A, ProblemType.EIGENVALUE, initial_num_candidates=P, quiet=True, diag_info=diag, engine=eng)


def _vec(c):
    return np.array(c.x_k if c.v_k is None else c.v_k)


@pytest.mark.parametrize("kind", ["lin", "eig"])
def test_bracket_draws_once_and_keeps_both_streams(kind):
    s0 = _solver(kind, "host", DrawContext())
    d0 = snapshot.rng_digest()
    s1 = _solver(kind, "device", DrawContext())
    assert snapshot.rng_digest() == d0
    ctx = s1.engine.ctx
    assert ctx.draw_calls == [(P, [UNIT] * P)] and ctx.puts == 0
    assert s0.engine.ctx.draw_calls == [] and s0.engine.ctx.puts >= 1
    assert [c.id for c in s0.candidates] == [c.id for c in s1.candidates]
    for a, b in zip(s0.candidates, s1.candidates):
        assert a.lambda_k == b.lambda_k and len(b.param_history) == 1 and len(b.residual_history) == 1
        assert b._dev_valid and not b._host_valid
        np.testing.assert_allclose(_vec(b), _vec(a), rtol=4e-16, atol=0)
        h = b.param_history[0]                              # through the history store
        assert len(h) == len(a.param_history[0]) and np.array_equal(h[-1], _vec(b))
        if kind == "eig":
            assert h[0] == a.param_history[0][0]


@pytest.mark.parametrize("kind", ["lin", "eig"])
def test_an_undecided_norm_test_replays_the_rest_on_the_host(kind):
    """Draw 3 of the bracket reports a norm that fails AMS:131's test: draws 3, 4 and 5 take the host path from the stream
    position draw 3 starts at -- the host's vectors bit for bit -- and the stream ends where the host's ends."""
    s0 = _solver(kind, "host", DrawContext())
    d0 = snapshot.rng_digest()
    s1 = _solver(kind, "device", DrawContext(zero_norm=(0, 3)))
    assert snapshot.rng_digest() == d0
    assert s1.engine.ctx.puts == 1                          # the three replayed rows in the bracket's one transfer
    for k, (a, b) in enumerate(zip(s0.candidates, s1.candidates)):
        assert a.id == b.id and a.lambda_k == b.lambda_k
        if k >= 3:
            assert np.array_equal(_vec(a), _vec(b)) and np.array_equal(b.param_history[0][-1], _vec(a))
        else:
            np.testing.assert_allclose(_vec(b), _vec(a), rtol=4e-16, atol=0)


def _spawn(mode, base_norm, ctx):
    s = _solver("eig", mode, ctx)
    g = np.random.default_rng(2)
    v = g.standard_normal(N) + 1j * g.standard_normal(N)
    v *= base_norm / np.linalg.norm(v)
    s.converged_solutions = [(0.25 - 0.5j, v)]
    s.num_distinct_converged_solutions = 1
    s.landscape_energy = 0.5
    s._manage_candidates(1)
    born = [c for c in s.candidates if c.id >= P]
    return s, born, snapshot.rng_digest()


def test_spawn_from_a_base_takes_the_norm_of_v_pert_from_the_device():
    s0, born0, d0 = _spawn("host", 1.0, DrawContext())
    s1, born1, d1 = _spawn("device", 1.0, DrawContext())
    assert len(born0) == 15 and [c.id for c in born0] == [c.id for c in born1] and d0 == d1
    assert [c.lambda_k for c in born0] == [c.lambda_k for c in born1]
    assert s1.engine.ctx.draw_calls[1] == (30, [NORM, UNIT] * 15) and s1.engine.ctx.puts == 0
    for a, b in zip(born0, born1):
        np.testing.assert_allclose(_vec(b), _vec(a), rtol=4e-16, atol=0)


def test_spawn_whose_bound_does_not_decide_replays_on_the_host():
    """||base|| = 1e6 >> ||v_pert||: the triangle bound says nothing, so the whole bracket is the host's."""
    s0, born0, d0 = _spawn("host", 1e6, DrawContext())
    s1, born1, d1 = _spawn("device", 1e6, DrawContext())
    assert len(born0) == 15 and [c.id for c in born0] == [c.id for c in born1] and d0 == d1
    assert s1.engine.ctx.puts == 1
    for a, b in zip(born0, born1):
        assert a.lambda_k == b.lambda_k and np.array_equal(_vec(a), _vec(b))
