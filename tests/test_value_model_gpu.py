"""Learned terminal values on the GPU: the matrix-core kernel (``l2a_value_mlp_k``) against the float64 restatement of the
model, the bits it promises (a row's value depends on that row only), the fold (``l2a_value_terminal``) bit for bit against
its fp32 restatement, the three plan entries against their two-call restatement and the float64 oracle, and the controller.

Measured on one MI355X (maximum over all cases of ``|got - want| / max(1, |want|)``, bar 1e-4): see the figures the tests
print, recorded in DESIGN section 4.14."""

import ctypes

import numpy as np
import pytest
import torch

import cases
import mppi_reference as mr
import reward_model_cases as rmc
import reward_program_cases as rpc
import value_model_cases as vmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPValueModel
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel, NativeValueModel
from learning_to_adapt_amd.envs.reward_spec import RewardSpec, reward_spec_for_env
from learning_to_adapt_amd.policies import MPCController

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
ACTS = ["relu", "tanh"]
shapes = pytest.mark.parametrize("shape", vmc.SHAPES, ids=vmc.SHAPE_IDS)


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_SETUPS = {}


def _setup(shape, act):
    """Value model, statistics, last states, incoming returns and the restated values of a shape: built once, never modified."""
    key = (shape, act)
    if key not in _SETUPS:
        m, n, od, h, hidden = shape
        params = vmc.value_weights(od, hidden)
        norm = vmc.value_norm(od)
        native = NativeValueModel(od, hidden, act)
        native.set_weights(params)
        native.set_norm(norm)
        states = vmc.states(100 + n, m * n, od, norm)
        returns = (3.0 * np.random.RandomState(200 + n).randn(m, n)).astype(np.float32)
        want_v = vmc.restate(params, norm, act, states)
        values = native.predict(_dev(states)).cpu().numpy()
        _SETUPS[key] = dict(native=native, params=params, norm=norm, states=states, returns=returns, want_v=want_v, values=values)
    return _SETUPS[key]


def _terminal(native, states, returns, m, n, h, discount, coef, cand_offset, guard=0, in_place=False, keys=True, rets=True):
    buf = torch.full((guard + m * n + guard,), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((guard + m + guard,), -77, dtype=torch.int64, device="cuda:0")
    r_in = _dev(returns)
    out = buf[guard:guard + m * n]
    if in_place:
        out.copy_(r_in.reshape(-1))
        r_in = out
    native.terminal(_dev(states), r_in, m, n, h, discount, value_coef=coef, cand_offset=cand_offset,
                    returns_out=out if rets else None, best_key=best[guard:guard + m] if keys else None)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), best.cpu().numpy()


# ------------------------------------------------------------------------------------------
# 1. predict against the float64 restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@shapes
def test_predict_matches_the_float64_restatement(shape, act):
    s = _setup(shape, act)
    assert np.isfinite(s["want_v"]).all() and np.std(s["want_v"]) > 0.01
    err = rel_err(s["values"], s["want_v"])
    print("predict vs float64 restatement %s %s: %.2e" % (shape, act, err))
    assert err < RTOL


# ------------------------------------------------------------------------------------------
# 2. bits
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@shapes
def test_a_rows_value_does_not_depend_on_its_place_or_the_geometry(shape, act):
    """The shape's rows predicted among all rows, and again inside larger batches whose row counts `l2a_value_model_geometry`
    maps to every RT the shape's widths allow on this device - shifted by 5 rows, so that every row changes its lane and tile."""
    m, n, od, h, hidden = shape
    s = _setup(shape, act)
    native, states, base = s["native"], s["states"], s["values"]
    rows, cus = m * n, _cus()
    again = native.predict(_dev(states)).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(base))                    # two identical calls
    seen = {_lib.value_model_geometry(od, hidden, rows, cus=cus)["RT"]}
    for rt in (1, 2, 4, 8):
        total = 16 * cus * (rt // 2) + 1 if rt > 1 else rows + 5
        total = max(total, rows + 5)
        g = _lib.value_model_geometry(od, hidden, total, cus=cus)
        if g["RT"] != rt:
            continue            # (the accumulator or LDS budget caps this width below rt: the CPU table shows where)
        seen.add(rt)
        big = vmc.states(300 + rt, total, od, s["norm"])
        big[5:5 + rows] = states
        got = native.predict(_dev(big)).cpu().numpy()
        assert np.array_equal(_bits(got[5:5 + rows]), _bits(base)), "RT = %d" % rt
        # a shifted sub-range of the big batch on its own
        sub = native.predict(_dev(big[3:3 + rows + 2])).cpu().numpy()
        assert np.array_equal(_bits(sub[2:2 + rows]), _bits(base))
    cap = 32 // (max(hidden) // 64)
    assert seen == {rt for rt in (1, 2, 4, 8) if rt <= cap}, seen


# ------------------------------------------------------------------------------------------
# 3. l2a_value_terminal
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("coef", [1.0, 0.5])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@shapes
def test_terminal_is_the_fp32_fold_of_predict(shape, discount, coef, cand_offset, act):
    m, n, od, h, hidden = shape
    s = _setup(shape, act)
    buf, best = _terminal(s["native"], s["states"], s["returns"], m, n, h, discount, coef, cand_offset, guard=8)
    assert np.all(buf[:8] == -123.5) and np.all(buf[-8:] == -123.5)          # guard words on both sides untouched
    assert np.all(best[:8] == -77) and np.all(best[-8:] == -77)
    rets, keys = buf[8:-8], best[8:-8].view(np.uint64)
    want = vmc.fold_f32(s["returns"].reshape(-1), s["values"], discount, h, coef)
    assert np.array_equal(_bits(rets), _bits(want))
    assert np.array_equal(keys, _want_keys(rets.reshape(m, n), cand_offset))
    # against float64
    want64 = s["returns"].reshape(-1).astype(np.float64) + coef * discount ** h * s["want_v"]
    err = rel_err(rets, want64)
    print("terminal vs float64 %s %s discount %.1f coef %.1f: %.2e" % (shape, act, discount, coef, err))
    assert err < RTOL
    # in place, and each output alone
    buf2, best2 = _terminal(s["native"], s["states"], s["returns"], m, n, h, discount, coef, cand_offset, in_place=True)
    assert np.array_equal(_bits(buf2), _bits(rets)) and np.array_equal(best2.view(np.uint64), keys)
    buf3, best3 = _terminal(s["native"], s["states"], s["returns"], m, n, h, discount, coef, cand_offset, rets=False)
    assert np.all(buf3 == -123.5) and np.array_equal(best3.view(np.uint64), keys)
    buf4, best4 = _terminal(s["native"], s["states"], s["returns"], m, n, h, discount, coef, cand_offset, keys=False)
    assert np.array_equal(_bits(buf4), _bits(rets)) and np.all(best4 == -77)


@pytest.mark.parametrize("shape", [vmc.SHAPES[0], vmc.SHAPES[2]], ids=[vmc.SHAPE_IDS[0], vmc.SHAPE_IDS[2]])
def test_terminal_ties_non_finite_rows_and_a_zero_coefficient(shape):
    m, n, od, h, hidden = shape
    s = _setup(shape, "relu")
    native = s["native"]
    states, returns = s["states"].copy(), s["returns"].copy()
    # two duplicated candidates that win: the lower index takes the key
    e = m - 1
    lo_j, hi_j = 7, n - 3
    states[e * n + hi_j] = states[e * n + lo_j]
    returns[e] = -50.0
    returns[e, lo_j] = returns[e, hi_j] = 40.0
    buf, best = _terminal(native, states, returns, m, n, h, 0.9, 1.0, 1000)
    rets = buf.reshape(m, n)
    assert _bits(rets[e, lo_j]) == _bits(rets[e, hi_j]) and int(np.argmax(rets[e])) == lo_j
    assert _lib.key_decode(best.view(np.uint64)[e])[1] == 1000 + lo_j
    assert np.array_equal(best.view(np.uint64), _want_keys(rets, 1000))
    # one final state with an inf entry: its R' is NaN and it is the key
    bad = 20
    states[bad, od - 1] = np.inf
    buf, best = _terminal(native, states, returns, m, n, h, 0.9, 1.0, 0)
    rets = buf.reshape(m, n)
    assert np.isnan(rets[0, bad]) and np.isfinite(np.delete(buf, bad)).all()
    assert _lib.key_decode(best.view(np.uint64)[0])[1] == bad and best.view(np.uint64)[0] == _encode(np.nan, bad)
    assert np.array_equal(best.view(np.uint64), _want_keys(rets, 0))
    assert np.isnan(native.predict(_dev(states)).cpu().numpy()[bad])
    # value_coef = 0: R' is R bit for bit, even on that row
    buf, best = _terminal(native, states, returns, m, n, h, 0.9, 0.0, 0)
    assert np.array_equal(_bits(buf), _bits(returns.reshape(-1)))
    assert np.array_equal(best.view(np.uint64), _want_keys(returns, 0))
    # an inf among the incoming returns follows IEEE
    returns[0, 3] = -np.inf
    buf, _ = _terminal(native, states, returns, m, n, h, 0.9, 1.0, 0)
    assert buf[3] == -np.inf


def test_entry_points_validate():
    shape = vmc.SHAPES[0]
    m, n, od, h, hidden = shape
    s = _setup(shape, "relu")
    native = s["native"]
    st, r = _dev(s["states"]), _dev(s["returns"])
    out = torch.full((m * n,), -5.0, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -7, dtype=torch.int64, device="cuda:0")
    lib, null = native.lib, ctypes.c_void_p()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731

    def call(states=st, rin=r, m_=m, n_=n, h_=h, disc=0.9, coef=1.0, off=0, ro=out, bk=best):
        return lib.l2a_value_terminal(native.handle, ptr(states) if states is not None else null, ptr(rin) if rin is not None else null,
                                      m_, n_, h_, disc, coef, off, ptr(ro) if ro is not None else null,
                                      ptr(bk) if bk is not None else null, null)

    for kw in (dict(states=None), dict(rin=None), dict(ro=None, bk=None), dict(m_=0), dict(n_=0), dict(h_=0), dict(coef=float("nan")),
               dict(coef=float("inf")), dict(disc=float("inf")), dict(disc=float("nan")), dict(off=-1), dict(off=2 ** 31 - n)):
        assert call(**kw) == _lib.L2A_EINVAL, kw
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -5.0) and np.all(best.cpu().numpy() == -7)      # nothing launched, no output touched
    assert call(off=2 ** 31 - 1 - n) == _lib.L2A_OK
    fresh = NativeValueModel(od, (64,), "relu")
    with pytest.raises(_lib.L2AError, match="never set"):
        fresh.terminal(st, r, m, n, h, 1.0, returns_out=out)
    with pytest.raises(_lib.L2AError, match="never set"):
        fresh.predict(st)
    with pytest.raises(_lib.L2AError, match="width 96"):
        NativeValueModel(od, (96,), "relu")
    with pytest.raises(_lib.L2AError, match="all four"):
        one = np.zeros(od)
        native.ctx.check(lib.l2a_value_model_set_norm(fresh.handle, one.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None,
                                                      null), "l2a_value_model_set_norm")
    # identity statistics
    fresh.set_weights(s["params"])
    fresh.set_norm(None)
    got = fresh.predict(st).cpu().numpy()
    assert rel_err(got, vmc.restate(s["params"], None, "relu", s["states"])) < RTOL


# ------------------------------------------------------------------------------------------
# 4. the plan entries
# ------------------------------------------------------------------------------------------
PLAN_CASES = ["hc_rs_m2_n100_h7_e2_s0", "ant_cem_m2_n120_h4_pb2_s1"]     # a small mean ensemble, a per-block model
_PLANS = {}


def _plan_inputs(cid, act="relu", hidden=(128, 64)):
    """Dynamics model, value model, reward model, program and candidates of a golden case - built once, never modified."""
    key = (cid, act, hidden)
    if key not in _PLANS:
        from oracle.planner import sample_rs_actions
        from oracle.rewards import make_reward
        case, seed = cases.split_id(cid)
        env, model = cases.product_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        np.random.seed(seed)
        actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
        base = cases.recipe(case)[2][0]
        v_params, v_norm = vmc.value_weights(od, hidden), vmc.value_norm(od, base=base, value=(0.5, 20.0))
        vm = NativeValueModel(od, hidden, act)
        vm.set_weights(v_params)
        vm.set_norm(v_norm)
        r_params, r_norm = rmc.reward_weights(od, ad, hidden), rmc.reward_norm(od, ad, base=base)
        rm = NativeRewardModel(od, ad, hidden, act)
        rm.set_weights(r_params)
        rm.set_norm(r_norm)
        prog = rpc.new_reward_program(od, ad, env.dt)
        spec = reward_spec_for_env(env)             # the env's own closed-form reward: the fused rollout
        assert isinstance(spec, RewardSpec)
        _PLANS[key] = dict(case=case, env=env, model=model, actions=actions, gold=cases.load_golden(cid),
                           dyn=cases.oracle_dynamics(case), vm=vm, vfn=vmc.value_fn(v_params, v_norm, act),
                           rewards=dict(spec=(spec, make_reward(case["env"], env.dt)), program=(prog, prog.evaluate),
                                        model=(rm, rmc.reward_fn(r_params, r_norm, act))))
    return _PLANS[key]


def _shard(p, lo, hi):
    case = p["case"]
    m, n, h = case["m"], case["n"], case["h"]
    return p["actions"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * (hi - lo), -1)


def _plan_value(p, kind, coef, cand_offset=0, lo=None, hi=None, keys=True, rets=True):
    case, native = p["case"], p["model"].planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    out = torch.full((m, nl), float("nan"), dtype=torch.float32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    native.plan_rs_value(_dev(p["gold"]["obs0"]), _dev(_shard(p, lo, hi)), m, nl, h, case.get("discount", 1.0), p["rewards"][kind][0],
                         p["vm"], value_coef=coef, cand_offset=cand_offset, returns_out=out if rets else None,
                         best_key=best if keys else None)
    torch.cuda.synchronize()
    assert native.ctx.launch_status_value() == 0
    return out.cpu().numpy(), best.cpu().numpy().view(np.uint64)


def _two_calls(p, kind, coef, cand_offset=0):
    """The existing plan - ``l2a_plan_rs_chunk`` with ``state_out``, or the program / reward-model plan with its trajectory - and
    ``l2a_value_terminal`` behind it."""
    case, native = p["case"], p["model"].planner_model()
    m, n, h, disc = case["m"], case["n"], case["h"], case.get("discount", 1.0)
    obs0, a = _dev(p["gold"]["obs0"]), _dev(p["actions"])
    rets = torch.full((m, n), float("nan"), dtype=torch.float32, device=native.device)
    reward = p["rewards"][kind][0]
    if kind == "spec":
        state = torch.full((m * n, native.obs_dim), float("nan"), dtype=torch.float32, device=native.device)
        null = ctypes.c_void_p()
        rc = native.lib.l2a_plan_rs_chunk(native.handle, ctypes.c_void_p(obs0.data_ptr()), 0, ctypes.c_void_p(a.data_ptr()), m, n, h, 0,
                                          float(disc), ctypes.byref(reward), cand_offset, null, ctypes.c_void_p(rets.data_ptr()),
                                          ctypes.c_void_p(state.data_ptr()), null,
                                          ctypes.c_void_p(torch.cuda.current_stream(native.device).cuda_stream))
        native.ctx.check(rc, "l2a_plan_rs_chunk")
    else:
        traj = torch.full((h, m * n, native.obs_dim), float("nan"), dtype=torch.float32, device=native.device)
        plan = native.plan_rs_program if kind == "program" else native.plan_rs_reward_model
        plan(obs0, a, m, n, h, disc, reward, cand_offset=cand_offset, returns_out=rets, traj_out=traj)
        state = traj[h - 1].contiguous()
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    plain = rets.clone()
    p["vm"].terminal(state, rets, m, n, h, disc, value_coef=coef, cand_offset=cand_offset, returns_out=rets, best_key=best)
    torch.cuda.synchronize()
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64), plain.cpu().numpy()


@pytest.mark.parametrize("coef", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["spec", "program", "model"])
@pytest.mark.parametrize("cid", PLAN_CASES)
def test_plan_entries_are_their_two_calls_and_follow_the_oracle(cid, kind, coef):
    p = _plan_inputs(cid)
    case, gold = p["case"], p["gold"]
    m, n, h, disc = case["m"], case["n"], case["h"], case.get("discount", 1.0)
    rets, keys = _plan_value(p, kind, coef)
    want_r, want_k, plain = _two_calls(p, kind, coef)
    assert np.array_equal(_bits(rets), _bits(want_r)) and np.array_equal(keys, want_k)
    assert np.array_equal(keys, _want_keys(rets, 0))
    assert not np.array_equal(_bits(rets), _bits(plain))                # the term is there
    aug, total, _ = vmc.augmented_returns(p["dyn"], p["rewards"][kind][1], p["vfn"], gold["obs0"], p["actions"], n, disc, coef)
    err = rel_err(rets.reshape(-1), aug)
    print("%s %s coef %.1f: plan with a terminal value against the float64 oracle %.2e (term std %.3f, return std %.3f)"
          % (cid, kind, coef, err, np.std(aug - total), np.std(total)))
    assert err < RTOL and np.std(aug - total) > 0.01
    # each output alone
    r2, _ = _plan_value(p, kind, coef, keys=False)
    _, k2 = _plan_value(p, kind, coef, rets=False)
    assert np.array_equal(_bits(r2), _bits(rets)) and np.array_equal(k2, keys)


@pytest.mark.parametrize("kind", ["spec", "program", "model"])
@pytest.mark.parametrize("cid", PLAN_CASES)
def test_two_shards_combine_to_the_unsharded_plan(cid, kind):
    p = _plan_inputs(cid)
    n = p["case"]["n"]
    rets, keys = _plan_value(p, kind, 1.0)
    ra, ka = _plan_value(p, kind, 1.0, cand_offset=0, lo=0, hi=n // 2)
    rb, kb = _plan_value(p, kind, 1.0, cand_offset=n // 2, lo=n // 2, hi=n)
    assert np.array_equal(_bits(np.concatenate([ra, rb], axis=1)), _bits(rets))
    assert np.array_equal(np.maximum(ka, kb), keys)


def test_plan_entries_refuse_a_value_model_of_another_obs_dim_and_bad_arguments():
    p = _plan_inputs(PLAN_CASES[0])
    case, native = p["case"], p["model"].planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    obs0, a = _dev(p["gold"]["obs0"]), _dev(p["actions"])
    rets = torch.full((m, n), -5.0, dtype=torch.float32, device=native.device)
    other = NativeValueModel(native.obs_dim + 1, (64,), "relu")
    other.set_weights(vmc.value_weights(native.obs_dim + 1, (64,)))
    for kind in ("spec", "program", "model"):
        reward = p["rewards"][kind][0]
        with pytest.raises(_lib.L2AError, match=r"\(-1\).*the value model is for obs_dim"):
            native.plan_rs_value(obs0, a, m, n, h, 1.0, reward, other, returns_out=rets)
        with pytest.raises(_lib.L2AError, match="nothing to write"):
            native.plan_rs_value(obs0, a, m, n, h, 1.0, reward, p["vm"])
        with pytest.raises(_lib.L2AError, match="must be finite"):
            native.plan_rs_value(obs0, a, m, n, h, 1.0, reward, p["vm"], value_coef=float("nan"), returns_out=rets)
        with pytest.raises(_lib.L2AError, match="too many candidates"):
            native.plan_rs_value(obs0, a, m, n, h, 1.0, reward, p["vm"], cand_offset=-1, returns_out=rets)
    torch.cuda.synchronize()
    assert np.all(rets.cpu().numpy() == -5.0)


# ------------------------------------------------------------------------------------------
# 5. through the controller
# ------------------------------------------------------------------------------------------
def _controller(coef=vmc.RECIPE_COEF, with_value=True, **kw):
    """The controller recipe of value_model_cases.py: an h = 3 plan whose oracle winner the value term changes."""
    from oracle.rewards import make_reward
    case = dict(cases.CASES[vmc.RECIPE_CASE])
    env, model = cases.product_model(case)
    od = env.observation_space.shape[0]
    params, norm, act = vmc.recipe_value(cases.recipe(case)[2][0], od)
    vm = MLPValueModel(name="val", env=env, hidden_sizes=vmc.RECIPE_HIDDEN, hidden_nonlinearity=act, init_seed=0)
    vm.set_params(params)
    vm.set_normalization(norm)
    if with_value:
        kw.update(value_model=vm, terminal_value_coef=coef)
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0),
                         n_candidates=case["n"], horizon=case["h"], **kw)
    oracle = dict(dyn=cases.oracle_dynamics(case), rf=make_reward(case["env"], env.dt), vfn=vmc.model_value_fn(vm),
                  coef=coef if with_value else 0.0, disc=case.get("discount", 1.0))
    return case, env, model, ctrl, oracle, cases.load_golden(vmc.RECIPE_CASE + "_s0")["obs0"]


def _spy(ctrl, log):
    """Record every rollout's candidates and - asked for or not - its returns table."""
    rollout = ctrl._rollout

    def spy(observations, seq, n_it, cand_offset, want_returns, **kw):
        best, rets = rollout(observations, seq, n_it, cand_offset, True, **kw)
        log.append(dict(seq=seq.cpu().numpy().copy(), n=n_it, returns=rets.cpu().numpy().copy()))
        return best, (rets if want_returns else None)

    ctrl._rollout = spy


def _oracle_table(oracle, obs, snap):
    m = len(obs)
    aug = vmc.augmented_returns(oracle["dyn"], oracle["rf"], oracle["vfn"], obs, snap["seq"].astype(np.float64), snap["n"],
                                oracle["disc"], oracle["coef"])[0]
    return aug.reshape(m, snap["n"])


def _check_tables(oracle, obs, log, what):
    """Every rollout's returns within the bar of the oracle's augmented returns; the last one's table and its decided envs."""
    worst = 0.0
    for snap in log:
        want = _oracle_table(oracle, obs, snap)
        worst = max(worst, rel_err(snap["returns"], want))
    print("\n[value] %s: %d rollouts, returns against the oracle's augmented returns %.2e" % (what, len(log), worst))
    assert worst < RTOL, what
    decided = vmc.margins(want) > 2 * RTOL
    return want, decided


@pytest.mark.parametrize("with_value", [True, False], ids=["value", "plain"])
def test_controller_random_shooting_parity_rng_follows_the_oracle_in_both_settings(with_value):
    from oracle.planner import sample_rs_actions
    case, env, model, ctrl, oracle, obs = _controller(with_value=with_value, rng="numpy")
    m, n, h = case["m"], case["n"], case["h"]
    np.random.seed(vmc.RECIPE_SEED)
    actions = sample_rs_actions(env.action_space.low, env.action_space.high, n, m, h)
    rng_next = np.random.uniform()
    aug, total, _ = vmc.augmented_returns(oracle["dyn"], oracle["rf"], oracle["vfn"], obs, actions, n, oracle["disc"], vmc.RECIPE_COEF)
    aug, total = aug.reshape(m, n), total.reshape(m, n)
    assert np.any(np.argmax(aug, axis=1) != np.argmax(total, axis=1))          # the recipe: the term changes a winner
    want = aug if with_value else total
    assert np.all(vmc.margins(want) > 2 * RTOL)                                 # no case skipped: every env is decided
    best = np.argmax(want, axis=1)
    np.random.seed(vmc.RECIPE_SEED)
    got, info = ctrl.get_actions(obs)
    assert np.random.uniform() == rng_next and info == {}
    native = model.planner_model()
    assert native.value_plans == (1 if with_value else 0) and ctrl._program() == with_value
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, actions[0].reshape(m, n, -1)[np.arange(m), best])
    assert rel_err(ctrl.last_plan["best_return"], want[np.arange(m), best]) < RTOL


def test_controller_random_shooting_device_rng():
    case, env, model, ctrl, oracle, obs = _controller(rng="device")
    m, n = case["m"], case["n"]
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    got, _ = ctrl.get_actions(obs)
    assert len(log) == 1 and model.planner_model().value_plans == 1
    want, decided = _check_tables(oracle, obs, log, "RS, device rng")
    assert decided.sum() * 10 >= 9 * m
    best = np.argmax(want, axis=1)
    first = log[0]["seq"][0].reshape(m, n, -1)
    for i in np.nonzero(decided)[0]:
        assert ctrl.last_plan["best_index"][i] == best[i]
        np.testing.assert_array_equal(got[i], first[i, best[i]].astype(np.float64))


@pytest.mark.parametrize("cem_mode", ["fixed", "reference"])
def test_controller_device_cem(cem_mode):
    case, env, model, ctrl, oracle, obs = _controller(rng="device", use_cem=True, num_cem_iters=2, cem_mode=cem_mode)
    m, n = case["m"], case["n"]
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    got, _ = ctrl.get_actions(obs)
    assert len(log) == 2 and model.planner_model().value_plans == 2
    want, decided = _check_tables(oracle, obs, log, "device CEM, %s" % cem_mode)
    assert decided.sum() * 10 >= 9 * m
    best = np.argmax(want, axis=1)
    for i in np.nonzero(decided)[0]:
        assert ctrl.last_plan["best_index"][i] == best[i]
    assert rel_err(ctrl.last_plan["best_return"][decided], want[np.arange(m), best][decided]) < RTOL
    if cem_mode == "fixed":             # the executed action is the winning candidate's (clipped) first action
        first = log[-1]["seq"][0].reshape(m, n, -1)
        for i in np.nonzero(decided)[0]:
            np.testing.assert_array_equal(got[i], first[i, best[i]].astype(np.float64))


def test_controller_mppi():
    case, env, model, ctrl, oracle, obs = _controller(rng="device", use_mppi=True, mppi_iters=1)
    m, n, h = case["m"], case["n"], case["h"]
    ad = ctrl.action_space.shape[0]
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    action, _ = ctrl.get_actions(obs)
    assert len(log) == 1 and model.planner_model().value_plans == 1
    want, decided = _check_tables(oracle, obs, log, "MPPI")
    assert decided.sum() * 10 >= 9 * m
    plan = ctrl.last_plan
    assert np.array_equal(_bits(plan["returns"]), _bits(log[-1]["returns"]))
    for i in np.nonzero(decided)[0]:
        assert plan["best_index"][i] == int(np.argmax(want[i]))
    # the executed action is the planner's unchanged rule applied to R': the reward-weighted mean of its own samples, within the
    # derived bound of tests/mppi_reference.py (the first step starts from a zero mean)
    assert np.array_equal(action, plan["mppi_mean"][:, :ad].astype(np.float64))
    a_clip = ctrl._bufs["mppi_a_clip"].cpu().numpy()
    ref = mr.result_row(np.zeros((m, h * ad), dtype=np.float32), a_clip, plan["returns"], ctrl.mppi_kappa, ad)
    bound, _ = mr.update_bounds(n, ctrl.mppi_kappa, float(np.max(np.abs(a_clip))), mr.sum_chain(n))
    assert np.array_equal(plan["best_index"], ref["index"])
    assert float(np.max(np.abs(plan["mppi_mean"].astype(np.float64) - ref["mean"]))) <= bound


def test_controller_icem():
    case, env, model, ctrl, oracle, obs = _controller(rng="device", use_icem=True, icem_iters=2)
    m = case["m"]
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    action, _ = ctrl.get_actions(obs)
    assert len(log) == 2 and model.planner_model().value_plans == 2
    want, decided = _check_tables(oracle, obs, log, "iCEM")
    assert decided.sum() * 10 >= 9 * m
    plan, snap = ctrl.last_plan, log[-1]
    first = snap["seq"][0].reshape(m, snap["n"], -1)
    for i in np.nonzero(decided)[0]:
        j = int(np.argmax(want[i]))
        assert plan["best_index"][i] == j
        np.testing.assert_array_equal(action[i], first[i, j].astype(np.float64))      # iCEM executes its best candidate's first action


def test_controller_with_a_reward_program_and_with_a_reward_model():
    """The other two reward kinds route to their own entries and score R' too."""
    from learning_to_adapt_amd.dynamics import MLPRewardModel
    case = dict(cases.CASES[vmc.RECIPE_CASE])
    gold = cases.load_golden(vmc.RECIPE_CASE + "_s0")
    for kind in ("program", "model"):
        env, model = cases.product_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        base = cases.recipe(case)[2][0]
        params, norm, act = vmc.recipe_value(base, od)
        vm = MLPValueModel(name="val", env=env, hidden_sizes=vmc.RECIPE_HIDDEN, hidden_nonlinearity=act, init_seed=0)
        vm.set_params(params)
        vm.set_normalization(norm)
        kw = {}
        if kind == "program":
            env = rpc.program_env(case["env"])
            rf = env.reward
        else:
            rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(64,), init_seed=0)
            rm.set_params(rmc.reward_weights(od, ad, (64,)))
            rm.set_normalization(rmc.reward_norm(od, ad, base=base))
            rf = rmc.model_reward_fn(rm)
            kw = dict(reward_model=rm, use_reward_model=True)
        ctrl = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=case["n"], horizon=case["h"], rng="device",
                             value_model=vm, terminal_value_coef=0.5, **kw)
        oracle = dict(dyn=cases.oracle_dynamics(case), rf=rf, vfn=vmc.model_value_fn(vm), coef=0.5, disc=1.0)
        log = []
        _spy(ctrl, log)
        torch.manual_seed(7)
        ctrl.get_actions(gold["obs0"])
        native = model.planner_model()
        assert native.value_plans == 1 and native.program_plans == (kind == "program") and native.reward_model_plans == (kind == "model")
        _check_tables(oracle, gold["obs0"], log, "RS with a reward %s" % kind)


def test_model_predict_and_refresh():
    """``MLPValueModel.predict`` (float64 ``[rows]``) goes through ``l2a_value_model_predict``, and the native copy follows
    ``set_params`` / ``set_normalization``."""
    env = cases.product_model(cases.CASES["hc_rs_m3_n64_h5"])[0]
    od = 20
    vm = MLPValueModel(name="val", env=env, hidden_sizes=(256, 256), hidden_nonlinearity="swish", init_seed=0)
    vm.set_normalization(vmc.value_norm(od))
    obs = vmc.states(9, 300, od, vm.normalization).astype(np.float64)
    for seed in (6000, 6001):
        vm.set_params(vmc.value_weights(od, (256, 256), seed=seed))
        got = vm.predict(obs)
        assert got.dtype == np.float64 and got.shape == (300,)
        want = vmc.model_value_fn(vm)(obs)
        assert rel_err(got, want) < RTOL and np.std(want) > 0.01
    plain = MLPValueModel(name="val", env=env, hidden_sizes=(64,), normalize_input=False, init_seed=1)
    assert rel_err(plain.predict(obs), vmc.model_value_fn(plain)(obs)) < RTOL
