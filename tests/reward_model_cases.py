"""Shared builders of the reward-model tests (CPU and GPU): recipe weights and statistics of a reward MLP, inputs of
normalised scale, and the float64 restatement of the model's semantics that the oracle planner takes
as its ``reward_fn``."""

from collections import OrderedDict

import numpy as np

ACTS = {
    None: lambda x: x,
    "identity": lambda x: x,
    "relu": lambda x: np.maximum(x, 0.0),
    "tanh": np.tanh,
    "sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)),
    "swish": lambda x: x / (1.0 + np.exp(-x)),
}


def reward_weights(obs_dim, act_dim, hidden, seed=4000, bias_std=0.05):
    """Xavier-uniform kernels ``[in, out]`` and small random biases in fp32, as ``utils.synthetic.make_weight_set`` draws
    the dynamics models' - for the layer sizes ``[2 obs_dim + act_dim, *hidden, 1]``."""
    rs = np.random.RandomState(seed)
    sizes = [2 * obs_dim + act_dim] + list(hidden) + [1]
    params = []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        params.append(rs.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32))
        params.append((bias_std * rs.randn(fan_out)).astype(np.float32))
    return params


def reward_norm(obs_dim, act_dim, seed=5000, base=None):
    """Statistics as ``utils.synthetic.make_norm`` draws them (actions in [-1, 1]) - or those of ``base``, a dynamics
    model's dict - plus the reward's mean and standard deviation."""
    rs = np.random.RandomState(seed)
    norm = OrderedDict()
    if base is None:
        norm["obs"] = (0.1 * rs.randn(obs_dim), 1.0 + rs.rand(obs_dim))
        norm["delta"] = (0.01 * rs.randn(obs_dim), 0.1 + 0.1 * rs.rand(obs_dim))
        norm["act"] = (np.zeros(act_dim), np.full(act_dim, 2.0 / np.sqrt(12.0)))
    else:
        for key in ("obs", "delta", "act"):
            norm[key] = (np.asarray(base[key][0], dtype=np.float64), np.asarray(base[key][1], dtype=np.float64))
    norm["reward"] = (0.3 + 0.1 * rs.randn(), 1.5 + rs.rand())
    return norm


def restate(params, norm, act_name, obs, act, next_obs):
    """The model in float64 NumPy: rewards ``[rows]``.  ``norm`` None = identity.  A row with a non-finite input is NaN."""
    obs, act, next_obs = (np.asarray(v, dtype=np.float64) for v in (obs, act, next_obs))
    delta = next_obs - obs
    with np.errstate(all="ignore"):
        if norm is None:
            x = np.concatenate([obs, act, delta], axis=1)
        else:
            x = np.concatenate([(obs - norm["obs"][0]) / (norm["obs"][1] + 1e-10),
                                (act - norm["act"][0]) / (norm["act"][1] + 1e-10),
                                (delta - norm["delta"][0]) / (norm["delta"][1] + 1e-10)], axis=1)
        n_layers = len(params) // 2
        for li in range(n_layers):
            x = x @ np.asarray(params[2 * li], dtype=np.float64) + np.asarray(params[2 * li + 1], dtype=np.float64)
            if li < n_layers - 1:
                x = ACTS[act_name](x)
        z = x[:, 0]
        r = z if norm is None else z * (norm["reward"][1] + 1e-10) + norm["reward"][0]
    bad = ~(np.isfinite(obs).all(axis=1) & np.isfinite(act).all(axis=1) & np.isfinite(next_obs).all(axis=1))
    return np.where(bad, np.nan, r)


def reward_fn(params, norm, act_name):
    """``reward_fn(obs, act, next_obs)`` for ``oracle.planner.rollout_returns / rs_plan / cem_plan``."""
    return lambda obs, act, next_obs: restate(params, norm, act_name, obs, act, next_obs)


def model_reward_fn(model):
    """The restatement of an ``MLPRewardModel``'s current parameters and statistics."""
    params = [p.numpy() for p in model._params]
    return reward_fn(params, model.normalization if model.normalize_input else None, model.hidden_nonlinearity)


def inputs(seed, m, n, obs_dim, act_dim, h, norm):
    """``obs0 [m, obs]``, ``traj [h, m n, obs]``, ``actions [h, m n, act]`` in fp32, of the scale the statistics describe:
    observations around ``mu_obs``, every step adds a delta drawn around ``mu_delta``, actions uniform in [-1, 1]."""
    rs = np.random.RandomState(seed)
    obs0 = norm["obs"][0] + norm["obs"][1] * rs.randn(m, obs_dim)
    state = np.repeat(obs0, n, axis=0)
    traj = []
    for _ in range(h):
        state = state + norm["delta"][0] + norm["delta"][1] * rs.randn(m * n, obs_dim)
        traj.append(state)
    actions = rs.uniform(-1.0, 1.0, (h, m * n, act_dim))
    return obs0.astype(np.float32), np.stack(traj).astype(np.float32), actions.astype(np.float32)


def returns_f64(fn, obs0, traj, actions, n, discount):
    """Discounted returns ``[m n]`` of trajectories that are given (float64 arithmetic on the fp32 values)."""
    h = traj.shape[0]
    total = np.zeros(traj.shape[1])
    state = np.repeat(np.asarray(obs0, dtype=np.float64), n, axis=0)
    for t in range(h):
        nxt = traj[t].astype(np.float64)
        total += discount ** t * fn(state, actions[t].astype(np.float64), nxt)
        state = nxt
    return total
