"""Learned reward models on the GPU: the matrix-core scorer (``l2a_score_mlp_k``) against the float64 restatement of the
model, the bits it promises (a row's reward depends on that row only), the plan step (``l2a_plan_rs_reward_model``) against
the float64 oracle, and the controller.

Measured on one MI355X (maximum over all cases of ``|got - want| / max(1, |want|)``, bar 1e-4): see the figures the tests
print, recorded in DESIGN section 4.9."""

import ctypes

import numpy as np
import pytest
import torch

import cases
import cem_ties
import reward_model_cases as rmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
from learning_to_adapt_amd.policies import MPCController

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py

#          m,   n, obs, act, h, hidden
SHAPES = [(1, 64, 20, 6, 3, (64,)),                 # a whole block
          (1, 33, 17, 5, 1, (64, 64)),              # ragged, 2 * 17 + 5 = 39 inputs (no multiple of 4), h = 1
          (3, 70, 41, 8, 7, (128, 64)),             # blocks straddling env boundaries, unequal widths, odd horizon
          (2, 130, 64, 16, 2, (512, 512, 512))]     # every limit at once
ACTS = ["relu", "tanh"]


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


_SETUPS = {}


def _setup(shape, act):
    """Reward model, statistics, inputs and the restated per-discount returns of a shape: built once, never modified."""
    key = (shape, act)
    if key not in _SETUPS:
        m, n, od, ad, h, hidden = shape
        params = rmc.reward_weights(od, ad, hidden)
        norm = rmc.reward_norm(od, ad)
        native = NativeRewardModel(od, ad, hidden, act)
        native.set_weights(params)
        native.set_norm(norm)
        obs0, traj, actions = rmc.inputs(100 + n, m, n, od, ad, h, norm)
        fn = rmc.reward_fn(params, norm, act)
        want = {d: rmc.returns_f64(fn, obs0, traj, actions, n, d) for d in (1.0, 0.9)}
        _SETUPS[key] = dict(native=native, params=params, norm=norm, obs0=obs0, traj=traj, actions=actions, fn=fn, want=want)
    return _SETUPS[key]


def _score(native, obs0, traj, actions, m, n, h, discount, cand_offset, guard=0):
    rets = torch.full((guard + m * n + guard,), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    native.score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, discount, cand_offset=cand_offset,
                            returns_out=rets[guard:guard + m * n], best_key=best)
    torch.cuda.synchronize()
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64)


def _step_rewards(native, obs0, traj, actions, n):
    """``l2a_reward_model_predict`` step by step: fp32 ``[h, rows]``."""
    state = _dev(np.repeat(obs0, n, axis=0))
    out = []
    for t in range(traj.shape[0]):
        nxt = _dev(traj[t])
        out.append(native.predict(state, _dev(actions[t]), nxt).cpu().numpy())
        state = nxt
    return np.stack(out)


def _accumulate_f32(rewards, discount):
    """``R = R + f32(disc) * r`` in fp32, ``disc`` carried in float64 by repeated multiplication."""
    R = np.zeros(rewards.shape[1], dtype=np.float32)
    disc = 1.0
    for t in range(rewards.shape[0]):
        R = R + np.float32(disc) * rewards[t]
        disc *= discount
    return R


# ------------------------------------------------------------------------------------------
# 1. the scorer against the float64 restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d_n%d_o%d_a%d_h%d_%s" % (s[:5] + ("x".join(map(str, s[5])),)))
def test_scorer_matches_the_float64_restatement(shape, discount, cand_offset, act):
    m, n, od, ad, h, hidden = shape
    s = _setup(shape, act)
    rets, keys = _score(s["native"], s["obs0"], s["traj"], s["actions"], m, n, h, discount, cand_offset, guard=8)
    assert np.all(rets[:8] == -123.5) and np.all(rets[-8:] == -123.5)          # guard rows untouched
    rets = rets[8:-8]
    want = s["want"][discount]
    assert np.isfinite(want).all() and np.std(want) > 0.01
    err = rel_err(rets, want)
    print("scorer vs float64 restatement %s %s discount %.1f: %.2e" % (shape, act, discount, err))
    assert err < RTOL
    assert np.array_equal(keys, _want_keys(rets.reshape(m, n), cand_offset))


# ------------------------------------------------------------------------------------------
# 2. bits
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d_n%d_o%d_a%d_h%d_%s" % (s[:5] + ("x".join(map(str, s[5])),)))
def test_returns_are_the_fp32_sum_of_predict_and_do_not_depend_on_the_geometry(shape, discount, cand_offset, act):
    m, n, od, ad, h, hidden = shape
    s = _setup(shape, act)
    native, obs0, traj, actions = s["native"], s["obs0"], s["traj"], s["actions"]
    rets, keys = _score(native, obs0, traj, actions, m, n, h, discount, cand_offset)
    # (a) the discounted fp32 sum of the per-row rewards of l2a_reward_model_predict
    step = _step_rewards(native, obs0, traj, actions, n)
    assert np.array_equal(rets.view(np.uint32), _accumulate_f32(step, discount).view(np.uint32))
    # (b) two shards cut at an odd candidate
    cut = (n // 2) | 1
    t4, a4 = traj.reshape(h, m, n, od), actions.reshape(h, m, n, ad)
    parts, pkeys = [], []
    for lo, hi in ((0, cut), (cut, n)):
        r, k = _score(native, obs0, t4[:, :, lo:hi].reshape(h, -1, od), a4[:, :, lo:hi].reshape(h, -1, ad), m, hi - lo, h,
                      discount, cand_offset + lo)
        parts.append(r.reshape(m, hi - lo))
        pkeys.append(k)
    both = np.concatenate(parts, axis=1)
    assert np.array_equal(both.view(np.uint32), rets.reshape(m, n).view(np.uint32))
    assert np.array_equal(np.maximum(pkeys[0], pkeys[1]), keys)
    # (c) the rows of one env permuted: the returns move with them
    perm = np.random.RandomState(7).permutation(n)
    env = m - 1
    t5, a5 = t4.copy(), a4.copy()
    t5[:, env], a5[:, env] = t4[:, env][:, perm], a4[:, env][:, perm]
    r5, _ = _score(native, obs0, t5.reshape(h, m * n, od), a5.reshape(h, m * n, ad), m, n, h, discount, cand_offset)
    want5 = rets.reshape(m, n).copy()
    want5[env] = want5[env][perm]
    assert np.array_equal(r5.reshape(m, n).view(np.uint32), want5.view(np.uint32))
    # (d) the key is the arg-max of the kernel's own returns
    assert np.array_equal(keys, _want_keys(rets.reshape(m, n), cand_offset))


@pytest.mark.parametrize("act", ACTS)
def test_ties_nan_and_keys(act):
    shape = SHAPES[2]
    m, n, od, ad, h, hidden = shape
    s = _setup(shape, act)
    native, obs0, traj, actions = s["native"], s["obs0"], s["traj"], s["actions"]
    base, _ = _score(native, obs0, traj, actions, m, n, h, 0.9, 5)
    base = base.reshape(m, n)
    # an exact tie with the best candidate of env 1, at a higher and at a lower index: the first index wins
    top = int(np.argmax(base[1]))
    for twin in ((top + 17) % n, (top - 9) % n):
        t4, a4 = traj.reshape(h, m, n, od).copy(), actions.reshape(h, m, n, ad).copy()
        t4[:, 1, twin], a4[:, 1, twin] = t4[:, 1, top], a4[:, 1, top]
        rets, keys = _score(native, obs0, t4.reshape(h, m * n, od), a4.reshape(h, m * n, ad), m, n, h, 0.9, 5)
        rets = rets.reshape(m, n)
        assert rets[1, twin].view(np.uint32) == rets[1, top].view(np.uint32) == base[1, top].view(np.uint32)
        assert _lib.key_decode(keys[1])[1] == 5 + min(top, twin)
        assert np.array_equal(keys, _want_keys(rets, 5))
    # a NaN in one row (state, action or first observation): that row wins, no other row's bits change
    for what in ("traj", "act"):
        t4, a4 = traj.reshape(h, m, n, od).copy(), actions.reshape(h, m, n, ad).copy()
        if what == "traj":
            t4[3, 2, 41, od - 1] = np.nan
        else:
            a4[h - 1, 2, 41, 0] = np.inf
        rets, keys = _score(native, obs0, t4.reshape(h, m * n, od), a4.reshape(h, m * n, ad), m, n, h, 0.9, 5)
        rets = rets.reshape(m, n)
        assert np.isnan(rets[2, 41]) and np.isnan(rets).sum() == 1
        mask = np.ones((m, n), dtype=bool)
        mask[2, 41] = False
        assert np.array_equal(rets[mask].view(np.uint32), base[mask].view(np.uint32))
        assert _lib.key_decode(keys[2])[1] == 5 + 41 and np.array_equal(keys, _want_keys(rets, 5))
    o2 = obs0.copy()
    o2[0, 3] = np.nan                       # the whole env 0 at step 0
    rets, keys = _score(native, o2, traj, actions, m, n, h, 0.9, 5)
    rets = rets.reshape(m, n)
    assert np.isnan(rets[0]).all() and np.array_equal(rets[1:].view(np.uint32), base[1:].view(np.uint32))
    assert _lib.key_decode(keys[0])[1] == 5 and np.array_equal(keys, _want_keys(rets, 5))


def test_a_minus_infinity_row():
    """A reward of -inf from finite inputs (a network that passes feature 0 on, a large reward scale): the row loses to every
    finite one, an env of nothing but such rows picks index 0, and the other rows keep their bits."""
    m, n, od, ad, h = 2, 40, 20, 6, 3
    params = [np.zeros((2 * od + ad, 64), np.float32), np.zeros(64, np.float32), np.zeros((64, 1), np.float32),
              np.zeros(1, np.float32)]
    params[0][0, 0], params[2][0, 0] = 1.0, -1.0            # z = -relu(obs[0])
    params[0][1, 1], params[2][1, 0] = 1.0, 0.5             # ... + 0.5 relu(obs[1])
    norm = rmc.reward_norm(od, ad)
    for key in ("obs", "act", "delta"):
        norm[key] = (np.zeros_like(norm[key][0]), np.ones_like(norm[key][1]))
    norm["reward"] = (0.0, 1e3)
    native = NativeRewardModel(od, ad, (64,), "relu")
    native.set_weights(params)
    native.set_norm(norm)
    obs0, traj, actions = rmc.inputs(1, m, n, od, ad, h, norm)
    base, _ = _score(native, obs0, traj, actions, m, n, h, 1.0, 0)
    assert np.isfinite(base).all()
    t4 = traj.reshape(h, m, n, od).copy()
    t4[0, 0, 7, 0] = 1e38                   # obs of step 1 of (env 0, candidate 7): r = -1e38 * 1e3 = -inf
    t4[0, 1, :, 0] = 1e38                   # every candidate of env 1
    rets, keys = _score(native, obs0, t4.reshape(h, m * n, od), actions, m, n, h, 1.0, 0)
    rets, base = rets.reshape(m, n), base.reshape(m, n)
    assert rets[0, 7] == -np.inf and np.all(rets[1] == -np.inf)
    keep = np.arange(n) != 7
    assert np.array_equal(rets[0, keep].view(np.uint32), base[0, keep].view(np.uint32))
    assert np.array_equal(keys, _want_keys(rets, 0))
    assert _lib.key_decode(keys[0])[1] == int(np.argmax(base[0, keep]) + (np.argmax(base[0, keep]) >= 7))
    assert keys[1] == _encode(-np.inf, 0)


def test_entry_points_validate():
    s = _setup(SHAPES[0], "relu")
    native, (m, n, od, ad, h, _) = s["native"], SHAPES[0]
    o, t, a = _dev(s["obs0"]), _dev(s["traj"]), _dev(s["actions"])
    with pytest.raises(_lib.L2AError, match="nothing to write"):
        native.score_trajectory(o, t, a, m, n, h, 1.0)
    fresh = NativeRewardModel(od, ad, (64,), "relu")
    rets = torch.empty((m * n,), dtype=torch.float32, device="cuda:0")
    with pytest.raises(_lib.L2AError, match="never set"):
        fresh.score_trajectory(o, t, a, m, n, h, 1.0, returns_out=rets)
    with pytest.raises(_lib.L2AError, match="width 96"):
        NativeRewardModel(od, ad, (96,), "relu")
    # keys alone
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    native.score_trajectory(o, t, a, m, n, h, 1.0, best_key=best)
    native.score_trajectory(o, t, a, m, n, h, 1.0, returns_out=rets)
    torch.cuda.synchronize()
    assert np.array_equal(best.cpu().numpy().view(np.uint64), _want_keys(rets.cpu().numpy().reshape(m, n), 0))


# ------------------------------------------------------------------------------------------
# 3. the plan step against the float64 oracle
# ------------------------------------------------------------------------------------------
PLAN_CASES = ["hc_rs_ragged_n37_h3_s0", "hc_rs_discount_s0", "ant_rs_4x256_e2_s0", "hc_rs_m2_n100_h7_e2_s0"]
_PLANS = {}


def _plan_inputs(cid, act="relu", hidden=(128, 64)):
    """Dynamics model, reward model, candidates of a golden case - built once, shared and never modified."""
    key = (cid, act, hidden)
    if key not in _PLANS:
        from oracle.planner import sample_rs_actions
        case, seed = cases.split_id(cid)
        env, model = cases.product_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        np.random.seed(seed)
        actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
        params = rmc.reward_weights(od, ad, hidden)
        norm = rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0])
        native_rm = NativeRewardModel(od, ad, hidden, act)
        native_rm.set_weights(params)
        native_rm.set_norm(norm)
        _PLANS[key] = dict(case=case, env=env, model=model, actions=actions, gold=cases.load_golden(cid),
                           dyn=cases.oracle_dynamics(case), rm=native_rm, fn=rmc.reward_fn(params, norm, act))
    return _PLANS[key]


def _plan(p, cand_offset=0, lo=None, hi=None, want_traj=True):
    case, native = p["case"], p["model"].planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    a = p["actions"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * nl, -1)
    rets = torch.full((m, nl), float("nan"), dtype=torch.float32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    traj = torch.full((h, m * nl, native.obs_dim), float("nan"), dtype=torch.float32, device=native.device) if want_traj else None
    native.plan_rs_reward_model(_dev(p["gold"]["obs0"]), _dev(a), m, nl, h, case.get("discount", 1.0), p["rm"],
                                cand_offset=cand_offset, returns_out=rets, best_key=best, traj_out=traj)
    torch.cuda.synchronize()
    assert native.ctx.launch_status_value() == 0
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64), (traj.cpu().numpy() if want_traj else None), a


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cid", PLAN_CASES)
def test_plan_step_against_the_oracle(cid, act):
    from oracle.planner import rollout_trace
    p = _plan_inputs(cid, act)
    case, gold = p["case"], p["gold"]
    m, n, h, disc = case["m"], case["n"], case["h"], case.get("discount", 1.0)
    want, states = rollout_trace(p["dyn"], p["fn"], gold["obs0"], p["actions"], n, disc)
    rets, keys, traj, a32 = _plan(p)
    err_r, err_s = rel_err(rets.reshape(-1), want), rel_err(traj, states)
    print("%s %s: returns %.2e, states %.2e against the float64 oracle" % (cid, act, err_r, err_s))
    assert err_r < RTOL and err_s < RTOL
    # the returns ARE the scorer applied to the trajectory that was written out
    again, keys2 = _score(p["rm"], gold["obs0"].astype(np.float32), traj, a32.astype(np.float32), m, n, h, disc, 0)
    assert np.array_equal(rets.reshape(-1).view(np.uint32), again.view(np.uint32)) and np.array_equal(keys, keys2)
    assert np.array_equal(keys, _want_keys(rets, 0))
    # the library's own trajectory buffer gives the same bits
    rets2, keys3, _, _ = _plan(p, want_traj=False)
    assert np.array_equal(rets2.view(np.uint32), rets.view(np.uint32)) and np.array_equal(keys3, keys)


@pytest.fixture
def _split_policy():
    ctx = _lib.Context.get(0)
    yield ctx
    ctx.set_split(0 if getattr(ctx, "split_degraded", False) else 1)


@pytest.mark.parametrize("cid", ["hc_rs_m2_n100_h7_e2_s0", "ant_rs_n300_h6_e3_s0"])
def test_plan_step_does_not_depend_on_geometry_or_sharding(cid, _split_policy):
    p = _plan_inputs(cid)
    n = p["case"]["n"]
    rets, keys, traj, _ = _plan(p)
    cut = (n // 2) | 1
    ra, ka, _, _ = _plan(p, cand_offset=0, lo=0, hi=cut, want_traj=False)
    rb, kb, _, _ = _plan(p, cand_offset=cut, lo=cut, hi=n, want_traj=False)
    both = np.concatenate([ra, rb], axis=1)
    assert np.array_equal(both.view(np.uint32), rets.view(np.uint32))
    assert np.array_equal(np.maximum(ka, kb), keys)
    _split_policy.set_split(0)
    rets0, keys0, traj0, _ = _plan(p)
    assert np.array_equal(rets0.view(np.uint32), rets.view(np.uint32)) and np.array_equal(keys0, keys)
    assert np.array_equal(traj0.view(np.uint32), traj.view(np.uint32))


def test_plan_step_refuses_a_reward_model_of_other_dimensions():
    p = _plan_inputs("hc_rs_ragged_n37_h3_s0")
    case, native = p["case"], p["model"].planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    rets = torch.empty((m, n), dtype=torch.float32, device=native.device)
    for od, ad in ((native.obs_dim + 1, native.act_dim), (native.obs_dim, native.act_dim + 1)):
        other = NativeRewardModel(od, ad, (64,), "relu")
        other.set_weights(rmc.reward_weights(od, ad, (64,)))
        with pytest.raises(_lib.L2AError, match=r"\(-1\).*the reward model is for obs_dim"):
            native.plan_rs_reward_model(_dev(p["gold"]["obs0"]), _dev(p["actions"]), m, n, h, 1.0, other, returns_out=rets)
    with pytest.raises(_lib.L2AError, match="nothing to write"):
        native.plan_rs_reward_model(_dev(p["gold"]["obs0"]), _dev(p["actions"]), m, n, h, 1.0, p["rm"])


# ------------------------------------------------------------------------------------------
# 4. through the controller
# ------------------------------------------------------------------------------------------
class _PredictOnly(object):
    """What a user's own reward model looks like to the controller: nothing but ``predict``."""

    def __init__(self, model):
        self.model, self.calls = model, 0

    def predict(self, obs, act, nxt):
        self.calls += 1
        return self.model.predict(obs, act, nxt)


def _controller(cid, act="relu", hidden=(128, 64), wrap=False, **kw):
    case, seed = cases.split_id(cid)
    env, model = cases.product_model(case)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=hidden, hidden_nonlinearity=act, init_seed=0)
    rm.set_params(rmc.reward_weights(od, ad, hidden))
    rm.set_normalization(rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0]))
    given = _PredictOnly(rm) if wrap else rm
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, reward_model=given, use_reward_model=True,
                         discount=case.get("discount", 1.0), n_candidates=case["n"], horizon=case["h"], **kw)
    return case, seed, env, model, rm, given, ctrl


@pytest.mark.parametrize("cid,act", [("hc_rs_m3_n64_h5_s0", "relu"), ("ant_rs_n300_h6_e3_s0", "tanh")])
def test_controller_random_shooting_like_the_oracle(cid, act):
    from oracle.planner import rs_plan
    case, seed, env, model, rm, _, ctrl = _controller(cid, act, rng="numpy")
    assert ctrl._native_reward_model() is rm and ctrl._fusable() and ctrl._program()
    gold = cases.load_golden(cid)
    np.random.seed(seed)
    want, best, returns, _ = rs_plan(cases.oracle_dynamics(case), rmc.model_reward_fn(rm), gold["obs0"], env.action_space.low,
                                     env.action_space.high, case["n"], case["h"], case.get("discount", 1.0))
    rng_next = np.random.uniform()
    top = np.sort(returns, axis=1)
    assert np.all((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1])) > 2 * RTOL)       # no declared near-tie
    np.random.seed(seed)
    got, info = ctrl.get_actions(gold["obs0"])
    assert np.random.uniform() == rng_next
    native = model.planner_model()
    assert info == {} and native.reward_model_plans == 1 and native.program_plans == 0
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert rel_err(ctrl.last_plan["best_return"], returns[np.arange(case["m"]), best]) < RTOL
    # the same plan through a wrapper that exposes only `predict`: the unfused loop, the same candidate
    _, _, _, model2, _, wrapped, plain = _controller(cid, act, wrap=True, rng="numpy")
    assert plain._native_reward_model() is None and not plain._fusable()
    np.random.seed(seed)
    got2, _ = plain.get_actions(gold["obs0"])
    assert wrapped.calls == case["h"] and model2.planner_model().reward_model_plans == 0
    np.testing.assert_array_equal(got2, want)


def test_controller_cem_teacher_forced_like_the_oracle():
    """Every CEM iteration on its own (``cem_mode="reference"``), started from the ORACLE's mean / std of the previous one with
    the same normal draws, so that no rank tie can decide the outcome: returns within the bar, every rank swap a witnessed
    tie, and the last iteration picks the oracle's candidate and float64 action."""
    from oracle.planner import cem_plan
    cid, iters = "hc_rs_m3_n64_h5_s0", 3
    case, seed, env, model, rm, _, ctrl = _controller(cid, rng="numpy", use_cem=True, num_cem_iters=iters, cem_mode="reference")
    gold = cases.load_golden(cid)
    m, n, h = case["m"], case["n"], case["h"]
    act_dim = env.action_space.shape[0]
    k = max(int(n * ctrl.percent_elites), 1)
    trace = []
    np.random.seed(seed)
    want, best, returns = cem_plan(cases.oracle_dynamics(case), rmc.model_reward_fn(rm), gold["obs0"], env.action_space.low,
                                   env.action_space.high, n, h, case.get("discount", 1.0), num_cem_iters=iters,
                                   percent_elites=ctrl.percent_elites, alpha=ctrl.alpha, trace=trace)
    rng_next = np.random.uniform()
    top = np.sort(returns, axis=1)
    assert np.all((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1])) > 2 * RTOL)
    clip_low = np.concatenate([env.action_space.low] * h)
    clip_high = np.concatenate([env.action_space.high] * h)
    np.random.seed(seed)
    mean, std = np.zeros((m, h * act_dim)), np.ones((m, h * act_dim))
    for it in range(iters):
        new_mean, new_std, mine, cand_a = ctrl._cem_iteration(gold["obs0"], mean, std, k, clip_low, clip_high, 0, n, 1)
        err = rel_err(mine, trace[it]["returns"])
        print("CEM iteration %d: returns %.2e against the float64 oracle" % (it, err))
        assert err < RTOL
        _, flips, _ = cem_ties.assert_flips_are_ties(mine, trace[it]["returns"], k, RTOL)
        if flips == 0:
            np.testing.assert_allclose(np.broadcast_to(new_mean, trace[it]["mean"].shape), trace[it]["mean"], rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(new_std, trace[it]["std"], rtol=1e-9, atol=1e-12)
        mean, std = trace[it]["mean"], trace[it]["std"]             # teacher forcing
    assert np.random.uniform() == rng_next
    idx = np.argmax(mine, axis=1)
    assert np.array_equal(idx, best)
    np.testing.assert_array_equal(cand_a[np.arange(m), idx], want)
    assert model.planner_model().reward_model_plans == iters
    # and the public call, both modes: it raised "needs a fusable closed-form reward" before
    for mode in ("reference", "fixed"):
        _, _, _, model2, _, _, c2 = _controller(cid, rng="numpy", use_cem=True, num_cem_iters=2, cem_mode=mode)
        np.random.seed(seed)
        got, _ = c2.get_actions(gold["obs0"])
        assert got.shape == (m, act_dim) and model2.planner_model().reward_model_plans == 2
    _, _, _, _, _, _, c3 = _controller(cid, wrap=True, rng="numpy", use_cem=True)
    with pytest.raises(_lib.L2AError, match="fusable"):
        c3.get_actions(gold["obs0"])


def test_model_predict_and_refresh():
    """``MLPRewardModel.predict`` is the reference's contract (float64 ``[rows]``) through ``l2a_reward_model_predict``, and the
    native copy follows ``set_params`` / ``set_normalization``."""
    env = cases.product_model(cases.CASES["hc_rs_m3_n64_h5"])[0]
    od, ad = 20, 6
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(256, 256), hidden_nonlinearity="swish", init_seed=0)
    rm.set_normalization(rmc.reward_norm(od, ad))
    obs0, traj, actions = rmc.inputs(9, 1, 300, od, ad, 1, rm.normalization)
    obs = np.repeat(obs0, 300, axis=0).astype(np.float64)
    for seed in (4000, 4001):
        rm.set_params(rmc.reward_weights(od, ad, (256, 256), seed=seed))
        got = rm.predict(obs, actions[0].astype(np.float64), traj[0].astype(np.float64))
        assert got.dtype == np.float64 and got.shape == (300,)
        want = rmc.model_reward_fn(rm)(obs, actions[0], traj[0])
        assert rel_err(got, want) < RTOL and np.std(want) > 0.01
    plain = MLPRewardModel(name="rew", env=env, hidden_sizes=(64,), normalize_input=False, init_seed=1)
    got = plain.predict(obs, actions[0].astype(np.float64), traj[0].astype(np.float64))
    assert rel_err(got, rmc.model_reward_fn(plain)(obs, actions[0], traj[0])) < RTOL
