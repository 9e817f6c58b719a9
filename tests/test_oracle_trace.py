"""`rollout_trace` / `rnn_rollout_trace`: the one horizon loop of the oracle planners, with what each step hands to the next.

The returns are those of `rollout_returns` / `rnn_rollout_returns` (thin wrappers: same array, bit for bit - the golden cases
of test_oracle.py pin them against the reference); the states are what stepping `predict` by hand gives, and a rollout
continued from the trace's step-k state with the remaining actions ends in the trace's last state - the property the GPU
chunk chains are tested for."""

import numpy as np
import pytest

from learning_to_adapt_amd.utils import synthetic
from oracle import LSTMStateTuple, OracleLSTMDynamics, OracleMLPDynamics, OracleRNNStackDynamics
from oracle.planner import rollout_returns, rollout_trace
from oracle.rnn_planner import repeat_hidden, rnn_rollout_returns, rnn_rollout_trace

M, N, H, DISCOUNT = 2, 5, 4, 0.9


def _inputs(obs_dim, act_dim, seed):
    rs = np.random.RandomState(seed)
    return rs, rs.randn(M, obs_dim), rs.uniform(-1, 1, (H, M * N, act_dim))


def test_mlp_trace_is_the_returns_loop_with_its_states():
    obs_dim, act_dim = 7, 3
    rs, obs0, acts = _inputs(obs_dim, act_dim, 3)
    sets = [synthetic.make_weight_set(obs_dim, act_dim, [24, 24], 10 + e) for e in range(2)]
    norms = [synthetic.make_norm(obs_dim, act_dim, -np.ones(act_dim), np.ones(act_dim), 20 + e) for e in range(2)]
    dyn = OracleMLPDynamics(obs_dim, act_dim, sets, norms, mode="mean", hidden_nonlinearity="tanh")
    reward = lambda o, a, n: n[:, 0] - o[:, 1] - 0.1 * np.sum(a * a, axis=1)  # noqa: E731
    total, states = rollout_trace(dyn, reward, obs0, acts, N, DISCOUNT)
    assert np.array_equal(total, rollout_returns(dyn, reward, obs0, acts, N, DISCOUNT))
    assert states.shape == (H, M * N, obs_dim) and states.dtype == np.float64
    state = np.repeat(obs0, N, axis=0)
    for t in range(H):
        state = dyn.predict(state, acts[t])
        assert np.array_equal(states[t], state)
    # continued from the state after step 1 (rows are their own envs now): the same last state
    _, tail = rollout_trace(dyn, reward, states[0], acts[1:], 1, DISCOUNT)
    assert np.array_equal(tail[-1], states[-1])


@pytest.mark.parametrize("cell,units", [("lstm", (12,)), ("gru", (9, 6)), ("rnn", (8,)), ("lstm", (6, 5))])
def test_rnn_trace_is_the_returns_loop_with_its_states_and_hiddens(cell, units):
    obs_dim, act_dim = 6, 2
    rs, obs0, acts = _inputs(obs_dim, act_dim, 4)
    norm = synthetic.make_norm(obs_dim, act_dim, -np.ones(act_dim), np.ones(act_dim), 5)
    if cell == "lstm" and len(units) == 1:
        dyn = OracleLSTMDynamics(obs_dim, act_dim, synthetic.make_lstm_set(obs_dim, act_dim, units[0], 6), norm)
    else:
        dyn = OracleRNNStackDynamics(obs_dim, act_dim, units, cell, synthetic.make_rnn_stack_set(obs_dim, act_dim, list(units), cell, 6),
                                     norm)
    layers = []
    for u in units:
        c, h = rs.randn(M, u).astype(np.float32), np.tanh(rs.randn(M, u)).astype(np.float32)
        layers.append(LSTMStateTuple(c, h) if cell == "lstm" else h)
    hid0 = layers if len(layers) > 1 else layers[0]
    reward = lambda o, a, n: n[:, 0] - o[:, 1] - 0.1 * np.sum(a * a, axis=1)  # noqa: E731
    total, states, hiddens = rnn_rollout_trace(dyn, reward, obs0, hid0, acts, N, DISCOUNT)
    assert np.array_equal(total, rnn_rollout_returns(dyn, reward, obs0, hid0, acts, N, DISCOUNT))
    assert states.shape == (H, M * N, obs_dim) and len(hiddens) == H
    state, hid = np.repeat(obs0, N, axis=0), repeat_hidden(hid0, N)
    flat = lambda hd: np.concatenate([np.concatenate(list(x), axis=1) if isinstance(x, LSTMStateTuple) else x  # noqa: E731
                                      for x in (list(hd) if len(units) > 1 else [hd])], axis=1)
    for t in range(H):
        state, hid = dyn.predict(state, acts[t], hid)
        assert np.array_equal(states[t], state) and np.array_equal(flat(hiddens[t]), flat(hid))
    _, tail, tail_hid = rnn_rollout_trace(dyn, reward, states[1], hiddens[1], acts[2:], 1, DISCOUNT)
    assert np.array_equal(tail[-1], states[-1]) and np.array_equal(flat(tail_hid[-1]), flat(hiddens[-1]))
