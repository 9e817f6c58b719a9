"""Shared builders and references of the policy-prior tests (CPU and GPU): recipe weights and statistics of a policy MLP, the
float64 oracle of the model and of the closed-loop proposal (the policy and the oracle's dynamics step taking turns), and the
fp32 restatement of ``l2a_policy_mlp_k``'s operation sequence:

    x   = (s - fp32(mu)) * fp32(1 / (sd + 1e-10))                     a subtract and a multiply
    y_u = bias_u + chain_u,  chain_u = fma(W[k, u], x[k], chain_u) over k in the MFMA's order: k-groups of 16 ascending, inside
          a group the four registers ii = 0 .. 3 one after the other, inside a register the four lane groups q = 0 .. 3
          (k = 16 g + 4 q + ii) - ``v_mfma_f32_16x16x4_f32`` is a k-ordered fma chain (tests/mfma_emulator.py); K is padded with
          zeros, which leave a chain unchanged
    a   = y * fp32(sd_a + 1e-10) + fp32(mu_a);  a = a + sigma * z where sigma != 0;  a = min(max(a, low), high)

every operation rounded once, on its own.  The hidden activation of the restatement is a parameter: relu is exact on the host;
the GPU tests pass the device's own ``tanhf`` (a host libm's differs in the last place)."""

from collections import OrderedDict

import numpy as np

from reward_model_cases import ACTS

F32 = np.float32


def policy_weights(obs_dim, act_dim, hidden, seed=8000, bias_std=0.05):
    """Xavier-uniform kernels ``[in, out]`` and small random biases in fp32 for the layer sizes ``[obs_dim, *hidden, act_dim]``."""
    rs = np.random.RandomState(seed)
    sizes = [obs_dim] + list(hidden) + [act_dim]
    params = []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        params.append(rs.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32))
        params.append((bias_std * rs.randn(fan_out)).astype(np.float32))
    return params


def constant_weights(obs_dim, act_dim, hidden, bias):
    """All-zero kernels, zero hidden biases and the output bias ``bias``: the policy's normalised output is ``bias`` everywhere."""
    sizes = [obs_dim] + list(hidden) + [act_dim]
    params = []
    for fan_in, fan_out in zip(sizes[:-1], sizes[1:]):
        params.append(np.zeros((fan_in, fan_out), dtype=np.float32))
        params.append(np.zeros(fan_out, dtype=np.float32))
    params[-1] = np.asarray(bias, dtype=np.float32).reshape(act_dim).copy()
    return params


def policy_norm(obs_dim, act_dim, seed=8100, base=None):
    """Observation statistics as ``utils.synthetic.make_norm`` draws them - or those of ``base``, a dynamics model's dict - plus
    the action's mean and standard deviation."""
    rs = np.random.RandomState(seed)
    norm = OrderedDict()
    if base is None:
        norm["obs"] = (0.1 * rs.randn(obs_dim), 1.0 + rs.rand(obs_dim))
    else:
        norm["obs"] = (np.asarray(base["obs"][0], dtype=np.float64), np.asarray(base["obs"][1], dtype=np.float64))
    norm["act"] = (0.05 * rs.randn(act_dim), 0.3 + 0.4 * rs.rand(act_dim))
    return norm


def states(seed, rows, obs_dim, norm):
    """fp32 ``[rows, obs_dim]`` of the scale the statistics describe."""
    rs = np.random.RandomState(seed)
    return (norm["obs"][0] + norm["obs"][1] * rs.randn(rows, obs_dim)).astype(np.float32)


# ------------------------------------------------------------------------------------------ float64
def restate64(params, norm, act_name, obs):
    """The model in float64 NumPy: actions ``[rows, act_dim]`` before noise and clip.  ``norm`` None = identity."""
    obs = np.asarray(obs, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = obs if norm is None else (obs - norm["obs"][0]) / (norm["obs"][1] + 1e-10)
        n_layers = len(params) // 2
        for li in range(n_layers):
            x = x @ np.asarray(params[2 * li], dtype=np.float64) + np.asarray(params[2 * li + 1], dtype=np.float64)
            if li < n_layers - 1:
                x = ACTS[act_name](x)
        return x if norm is None else x * (np.asarray(norm["act"][1], np.float64) + 1e-10) + np.asarray(norm["act"][0], np.float64)


def act64(params, norm, act_name, obs, sigma, low, high, z=None):
    """``l2a_policy_act`` in float64: the model, the noise where ``sigma != 0``, the clip; NaN rows for a non-finite state."""
    obs = np.asarray(obs, dtype=np.float64)
    a = restate64(params, norm, act_name, obs)
    sigma = np.asarray(sigma, dtype=np.float64)
    if z is not None and np.any(sigma != 0):
        zz = np.where(sigma != 0, np.asarray(z, dtype=np.float64).reshape(a.shape), 0.0)
        a = a + sigma * zz
    with np.errstate(all="ignore"):
        a = np.minimum(np.maximum(a, np.asarray(low, np.float64)), np.asarray(high, np.float64))
    a[~np.isfinite(obs).all(axis=1)] = np.nan
    return a


def propose64(dyn, params, norm, act_name, obs0, n_pi, h, sigma, low, high, z=None):
    """The closed-loop proposal in float64: ``dyn`` is an oracle dynamics model (``tests/oracle_backend.py``'s: ``predict(obs,
    act)`` on env-major rows), ``obs0`` ``[m, obs_dim]``, ``z`` ``[h, m, n_pi, act_dim]`` or None.  Returns ``(actions [h, m * n_pi,
    act_dim], states [h, m * n_pi, obs_dim])``; ``states[t]`` is the state AFTER step t (the last one is not needed by the proposal
    and is computed all the same)."""
    obs0 = np.asarray(obs0, dtype=np.float64)
    m = obs0.shape[0]
    state = np.repeat(obs0, n_pi, axis=0)
    acts, sts = [], []
    for t in range(h):
        zt = None if z is None else np.asarray(z[t], dtype=np.float64).reshape(m * n_pi, -1)
        a = act64(params, norm, act_name, state, sigma, low, high, zt)
        state = dyn.predict(state, a)
        acts.append(a)
        sts.append(state)
    return np.stack(acts), np.stack(sts)


# ------------------------------------------------------------------------------------------ fp32, the kernel's operations
def fma32(a, b, c):
    """One rounding of ``a * b + c`` (the product of two fp32 values is exact in float64)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def k_order(k_in):
    """The order in which an accumulator chain meets the inputs ``0 .. k_in - 1`` (the zero padding left out)."""
    out = []
    for g in range((k_in + 15) // 16):
        for ii in range(4):
            for q in range(4):
                k = 16 * g + 4 * q + ii
                if k < k_in:
                    out.append(k)
    return out


def layer_f32(x, w, b):
    """``x [rows, K] @ w [K, U] + b`` as the kernel computes it: one fma chain per element in ``k_order``, then the bias add."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F32)
    acc = np.zeros((x.shape[0], w.shape[1]), dtype=F32)
    with np.errstate(all="ignore"):
        for k in k_order(w.shape[0]):
            acc = fma32(x[:, k:k + 1], w[k:k + 1, :], acc)
        return (acc + np.asarray(b, dtype=F32)[None, :]).astype(F32)


def _host_act(name):
    if name == "relu":
        return lambda v: np.maximum(v, F32(0))
    if name in (None, "identity"):
        return lambda v: v
    return lambda v: ACTS[name](v.astype(F32)).astype(F32)


def act_f32(params, norm, act_name, obs, sigma, low, high, z=None, hidden_fn=None):
    """``l2a_policy_act`` restated operation by operation in fp32: ``[rows, act_dim]``.  ``hidden_fn``: the hidden activation on an
    fp32 array (default: the host's; relu and identity are exact)."""
    obs = np.asarray(obs, dtype=F32)
    hidden_fn = hidden_fn if hidden_fn is not None else _host_act(act_name)
    n_layers = len(params) // 2
    act_dim = params[-1].shape[0]
    with np.errstate(all="ignore"):
        if norm is None:
            mu, inv = np.zeros(obs.shape[1], F32), np.ones(obs.shape[1], F32)
            sda, mua = np.ones(act_dim, F32), np.zeros(act_dim, F32)
        else:
            mu = np.asarray(norm["obs"][0], dtype=np.float64).astype(F32)
            inv = (1.0 / (np.asarray(norm["obs"][1], dtype=np.float64) + 1e-10)).astype(F32)
            sda = (np.asarray(norm["act"][1], dtype=np.float64) + 1e-10).astype(F32)
            mua = np.asarray(norm["act"][0], dtype=np.float64).astype(F32)
        x = ((obs - mu).astype(F32) * inv).astype(F32)
        x = np.where(np.isfinite(obs), x, F32(0))        # (such a row is NaN in the end; keep the chains quiet)
        for li in range(n_layers):
            x = layer_f32(x, params[2 * li], params[2 * li + 1])
            if li < n_layers - 1:
                x = hidden_fn(x).astype(F32)
        a = ((x * sda).astype(F32) + mua).astype(F32)
        sigma = np.asarray(sigma, dtype=F32)
        if np.any(sigma != 0):
            zz = np.where(sigma != 0, np.asarray(z, dtype=F32).reshape(a.shape), F32(0))
            noisy = (a + (sigma * zz).astype(F32)).astype(F32)
            a = np.where(sigma != 0, noisy, a)
        a = np.minimum(np.maximum(a, np.asarray(low, dtype=F32)), np.asarray(high, dtype=F32)).astype(F32)
    a[~np.isfinite(obs).all(axis=1)] = np.nan
    return a


def geometry_rule(obs_dim, hidden, rows, cus, lds_per_block):
    """The documented launch rule (include/l2a.h): the smallest RT in 1 | 2 | 4 | 8 that leaves at most ``cus`` workgroups, capped by
    RT * widest / 64 <= 32 and RT * kgs KiB + 4 KiB <= lds_per_block; ``None`` when not even RT = 1 fits."""
    cus = cus if cus > 0 else 256
    tpw = max(w // 64 for w in hidden)
    kgs = max([(obs_dim + 15) // 16] + [w // 16 for w in hidden])
    tiles = (rows + 15) // 16
    best = None
    for rt in (1, 2, 4, 8):
        if rt * tpw > 32 or rt * kgs * 1024 + 4096 > lds_per_block:
            break
        best = rt
        if (tiles + rt - 1) // rt <= cus:
            break
    if best is None:
        return None
    return dict(RT=best, workgroups=(rows + 16 * best - 1) // (16 * best), lds_bytes=best * kgs * 1024)
