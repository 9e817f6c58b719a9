"""Shared builders of the terminal-value tests (CPU and GPU): recipe weights and statistics of a value MLP, states of
normalised scale, the float64 restatement of the model's semantics, and the oracle's augmented returns

    R' = R + value_coef * discount ** h * V(s_h)

on top of ``oracle.planner.rollout_trace``."""

from collections import OrderedDict

import numpy as np

from reward_model_cases import ACTS

#          m,   n, obs, h, hidden
SHAPES = [(1, 64, 20, 3, (64,)),                    # whole tiles
          (1, 33, 17, 1, (64, 64)),                 # ragged last tile; K padded 17 -> 32; obs_dim no multiple of 4; h = 1
          (3, 70, 41, 7, (128, 64)),                # workgroups straddling env boundaries: more than one key per workgroup; unequal widths
          (2, 130, 64, 2, (512, 512, 512))]         # every limit at once
SHAPE_IDS = ["m%d_n%d_o%d_h%d_%s" % (s[:4] + ("x".join(map(str, s[4])),)) for s in SHAPES]

# The controller recipe (found on the CPU with the oracle, tests/test_value_model.py checks it again): on golden case
# RECIPE_CASE planned with horizon 3 and candidates drawn after np.random.seed(RECIPE_SEED), the oracle's winner of at least
# one env differs with and without the value term of ``recipe_value`` at coefficient RECIPE_COEF, and the top-two margin of
# every env exceeds the bar in both settings.
RECIPE_CASE = "hc_rs_ragged_n37_h3"
RECIPE_SEED = 0
RECIPE_COEF = 1.0
RECIPE_HIDDEN = (128, 64)


def value_weights(obs_dim, hidden, seed=6000, bias_std=0.05):
    """Xavier-uniform kernels ``[in, out]`` and small random biases in fp32 for the layer sizes ``[obs_dim, *hidden, 1]``."""
    rs = np.random.RandomState(seed)
    sizes = [obs_dim] + list(hidden) + [1]
    params = []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        params.append(rs.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32))
        params.append((bias_std * rs.randn(fan_out)).astype(np.float32))
    return params


def value_norm(obs_dim, seed=7000, base=None, value=None):
    """Observation statistics as ``utils.synthetic.make_norm`` draws them - or those of ``base``, a dynamics model's dict -
    plus the value's mean and standard deviation (``value``: given, else drawn)."""
    rs = np.random.RandomState(seed)
    norm = OrderedDict()
    if base is None:
        norm["obs"] = (0.1 * rs.randn(obs_dim), 1.0 + rs.rand(obs_dim))
    else:
        norm["obs"] = (np.asarray(base["obs"][0], dtype=np.float64), np.asarray(base["obs"][1], dtype=np.float64))
    norm["value"] = value if value is not None else (0.5 + 0.1 * rs.randn(), 2.0 + rs.rand())
    return norm


def restate(params, norm, act_name, obs):
    """The model in float64 NumPy: values ``[rows]``.  ``norm`` None = identity.  A row with a non-finite input is NaN."""
    obs = np.asarray(obs, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = obs if norm is None else (obs - norm["obs"][0]) / (norm["obs"][1] + 1e-10)
        n_layers = len(params) // 2
        for li in range(n_layers):
            x = x @ np.asarray(params[2 * li], dtype=np.float64) + np.asarray(params[2 * li + 1], dtype=np.float64)
            if li < n_layers - 1:
                x = ACTS[act_name](x)
        z = x[:, 0]
        v = z if norm is None else z * (norm["value"][1] + 1e-10) + norm["value"][0]
    return np.where(np.isfinite(obs).all(axis=1), v, np.nan)


def value_fn(params, norm, act_name):
    return lambda obs: restate(params, norm, act_name, obs)


def model_value_fn(model):
    """The restatement of an ``MLPValueModel``'s current parameters and statistics."""
    params = [p.numpy() for p in model._params]
    return value_fn(params, model.normalization if model.normalize_input else None, model.hidden_nonlinearity)


def states(seed, rows, obs_dim, norm):
    """fp32 ``[rows, obs_dim]`` of the scale the statistics describe."""
    rs = np.random.RandomState(seed)
    return (norm["obs"][0] + norm["obs"][1] * rs.randn(rows, obs_dim)).astype(np.float32)


def discount_pow(discount, h):
    """``discount ** h`` as the rollout carries it: float64, h multiplications from 1.0."""
    d = 1.0
    for _ in range(h):
        d *= float(discount)
    return d


def fold_f32(returns, values, discount, h, coef):
    """The kernel's fold restated in fp32: ``R + np.float32(coef * d_h) * v``, a multiply and an add; ``w == 0`` leaves R."""
    returns = np.asarray(returns, dtype=np.float32)
    w = np.float32(float(coef) * discount_pow(discount, h))
    if w == 0:
        return returns.copy()
    with np.errstate(all="ignore"):
        return (returns + (w * np.asarray(values, dtype=np.float32)).astype(np.float32)).astype(np.float32)


def augmented_returns(dyn, reward_fn, vfn, observations, actions, n, discount, coef):
    """The oracle's returns with the terminal value: ``rollout_trace``'s total plus ``coef * discount ** h * V`` of its last
    state.  Returns ``(R' [m n], R [m n], states [h, m n, obs_dim])`` in float64."""
    from oracle.planner import rollout_trace
    total, trace = rollout_trace(dyn, reward_fn, observations, actions, n, discount)
    h = actions.shape[0]
    return total + float(coef) * float(discount) ** h * vfn(trace[-1]), total, trace


def margins(returns):
    """Per env: (top - second) / max(1, |top|) of a returns table ``[m, n]``."""
    top = np.sort(returns, axis=1)
    return (top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1]))


def recipe_value(env_norm, obs_dim, act="relu"):
    """The value network of the controller recipe: recipe weights over the dynamics model's observation statistics, scaled
    so that the term is of the size of a short plan's return."""
    params = value_weights(obs_dim, RECIPE_HIDDEN, seed=6100)
    norm = value_norm(obs_dim, base=env_norm, value=(0.0, 50.0))
    return params, norm, act
