"""Termination programs on the GPU: ``l2a_score_term_k`` bit for bit against its float32 restatement, its bit-equalities with
the existing scorers where no guard fires, the plan step (``l2a_plan_rs_term``) against the float64 oracle, its independence
of launch geometry and sharding, and the controller's routing."""

import ctypes

import numpy as np
import pytest
import torch

import cases
import reward_model_cases as rmc
import reward_program_cases as rpc
import termination_cases as tc
import termination_reference as tref
import value_model_cases as vmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel, MLPValueModel
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel, NativeValueModel
from learning_to_adapt_amd.envs import RewardProgram
from learning_to_adapt_amd.envs.reward_spec import RewardSpec, reward_spec_for_env
from learning_to_adapt_amd.policies import MPCController

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # returns against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
INF = float("inf")


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _ctx():
    return _lib.Context.get(0)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


def _score(term, obs0, traj, actions, m, n, h, discount, cand_offset=0, program=None, step_rewards=None, values=None, coef=1.0,
           guard=0, keys=True, rets=True, steps=True):
    """The kernel alone, with ``guard`` untouched elements in front of and behind the returns and the step counts."""
    r = torch.full((guard + m * n + guard,), -123.5, dtype=torch.float32, device="cuda:0")
    s = torch.full((guard + m * n + guard,), -77, dtype=torch.int32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    _ctx().score_trajectory_term(_dev(obs0) if program is not None else None, _dev(traj),
                                 _dev(actions) if program is not None else None, m, n, h, discount, term, program=program,
                                 step_rewards=None if step_rewards is None else _dev(step_rewards),
                                 terminal_values=None if values is None else _dev(values), value_coef=coef, cand_offset=cand_offset,
                                 returns_out=r[guard:guard + m * n] if rets else None,
                                 steps_alive_out=s[guard:guard + m * n] if steps else None, best_key=best if keys else None)
    torch.cuda.synchronize()
    return r.cpu().numpy(), s.cpu().numpy(), best.cpu().numpy().view(np.uint64)


_REFS = {}


def _kernel_case(shape, discount, terminal_reward):
    """Inputs, program, guards and the restatement's outputs of a kernel case - computed once, never modified."""
    key = (shape, discount, terminal_reward)
    if key not in _REFS:
        m, n, od, ad, h = shape
        guards = tc.kernel_guards(od)
        term = tc.program_of(guards, terminal_reward)
        prog = rpc.every_kind_program(od, ad)
        obs0, traj, actions = tc.kernel_inputs(10 + n, m, n, od, ad, h)
        want, steps = term.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, discount, program=prog)
        _REFS[key] = dict(term=term, prog=prog, guards=guards, obs0=obs0, traj=traj, actions=actions, want=want, steps=steps)
    return _REFS[key]


# ------------------------------------------------------------------------------------------
# 1. the kernel alone, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terminal_reward", [0.0, -3.5])
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("shape", tc.KERNEL_SHAPES, ids=tc.KERNEL_IDS)
def test_kernel_matches_the_fp32_restatement(shape, discount, cand_offset, terminal_reward):
    m, n, od, ad, h = shape
    c = _kernel_case(shape, discount, terminal_reward)
    want, steps = c["want"], c["steps"]
    alive = tc.survived(c["guards"], c["traj"], steps)
    assert np.isfinite(want).all() and (steps == 1).any() and alive.any()       # dead at step 0, survivors ...
    if h > 1:
        assert ((steps == h) & ~alive).any()                                    # ... dead at the last step ...
    if h > 2:
        assert ((steps > 1) & (steps < h)).any()                                # ... and at a middle step
    args = (c["term"], c["obs0"], c["traj"], c["actions"], m, n, h, discount, cand_offset)
    r, s, keys = _score(*args, program=c["prog"], guard=5)
    assert np.array_equal(_bits(r[5:-5]), _bits(want)) and np.array_equal(s[5:-5], steps)
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), cand_offset))
    assert (r[:5] == -123.5).all() and (r[-5:] == -123.5).all() and (s[:5] == -77).all() and (s[-5:] == -77).all()
    if cand_offset == 0:            # each output alone
        _, _, k2 = _score(*args, program=c["prog"], rets=False, steps=False)
        r2, s2, _ = _score(*args, program=c["prog"], keys=False, steps=False)
        assert np.array_equal(k2, keys) and np.array_equal(_bits(r2), _bits(want)) and (s2 == -77).all()


# ------------------------------------------------------------------------------------------
# 2. guards that never fire: l2a_score_trajectory's bits
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tc.KERNEL_SHAPES, ids=tc.KERNEL_IDS)
def test_never_firing_guards_give_score_trajectorys_bits(shape):
    m, n, od, ad, h = shape
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = tc.kernel_inputs(10 + n, m, n, od, ad, h)
    term = tc.program_of(tc.never_guards(od), -3.5)
    rets = torch.full((m * n,), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    _ctx().score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, 0.9, prog, cand_offset=7, returns_out=rets, best_key=best)
    r, s, keys = _score(term, obs0, traj, actions, m, n, h, 0.9, 7, program=prog)
    assert np.array_equal(_bits(r), _bits(rets.cpu().numpy())) and np.array_equal(keys, best.cpu().numpy().view(np.uint64))
    assert (s == h).all()


# ------------------------------------------------------------------------------------------
# 3. NaN and ties
# ------------------------------------------------------------------------------------------
def test_nan_and_ties():
    m, n, od, ad, h = 2, 70, 17, 5, 4
    prog = rpc.every_kind_program(od, ad)
    guards = tc.kernel_guards(od)
    term = tc.program_of(guards, -3.5)
    obs0, traj, actions = tc.kernel_inputs(3, m, n, od, ad, h)
    traj[:, :, 1] = np.clip(traj[:, :, 1], -7.0, 7.0)           # nothing dies by itself ...
    traj[:, :, od - 4:od - 1] = np.minimum(traj[:, :, od - 4:od - 1], 8.0)
    traj[1, 5, 1] = 9.0                                         # ... row 5 dies at step 1, and what follows is NaN
    traj[2:, 5, :] = np.nan
    actions[2:, 5, :] = np.nan
    traj[0, 9, od - 3] = np.nan                                 # a NaN in a guarded element terminates row 9 at step 0
    traj[2, 11, 0] = np.nan                                     # a NaN outside the guards of a living row reaches R
    traj[:, 21] = traj[:, 20]                                   # two identical candidates
    actions[:, 21] = actions[:, 20]
    want, steps = term.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, 0.9, program=prog)
    assert steps[5] == 2 and np.isfinite(want[5]) and steps[9] == 1 and np.isfinite(want[9])
    assert np.isnan(want[11]) and steps[11] == h and _bits(want[20:21]) == _bits(want[21:22])
    r, s, keys = _score(term, obs0, traj, actions, m, n, h, 0.9, 0, program=prog)
    assert np.array_equal(_bits(r), _bits(want)) and np.array_equal(s, steps)
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), 0))
    assert _lib.key_decode(keys[0])[1] == 11                    # NaN sorts highest
    # the tie decides an env: env 1's best row gets a twin beside it, the lower index of the two wins
    finite = traj.copy()
    finite[2, 11, 0] = 1.0
    j = int(np.argmax(want.reshape(m, n)[1]))
    twin = j + 1 if j < n - 1 else j - 1
    twin_a = actions.copy()
    finite[:, n + twin] = finite[:, n + j]
    twin_a[:, n + twin] = twin_a[:, n + j]
    w2, _ = term.returns_f32(np.repeat(obs0, n, axis=0), finite, twin_a, 0.9, program=prog)
    assert np.isfinite(w2).all() and w2[n + twin] == w2[n + j] == w2.reshape(m, n)[1].max()
    _, _, k2 = _score(term, obs0, finite, twin_a, m, n, h, 0.9, 0, program=prog)
    assert np.array_equal(k2, _want_keys(w2.reshape(m, n), 0)) and _lib.key_decode(k2[1])[1] == min(j, twin)
    # all rows dead at step 0
    dead = tc.program_of([(0, 1, 100.0, INF)], -3.5)
    w3, s3 = dead.returns_f32(np.repeat(obs0, n, axis=0), finite, actions, 0.9, program=prog)
    r3, st3, k3 = _score(dead, obs0, finite, actions, m, n, h, 0.9, 0, program=prog)
    assert (s3 == 1).all() and np.array_equal(st3, s3) and np.array_equal(_bits(r3), _bits(w3))
    assert np.array_equal(k3, _want_keys(w3.reshape(m, n), 0))


def test_entry_refusals_touch_nothing():
    m, n, od, ad, h = 1, 33, 17, 5, 2
    prog = rpc.every_kind_program(od, ad)
    term = tc.program_of(tc.kernel_guards(od))
    obs0, traj, actions = tc.kernel_inputs(3, m, n, od, ad, h)
    given = np.zeros((h, m * n), dtype=np.float32)
    with pytest.raises(_lib.L2AError, match="exactly one"):
        _score(term, obs0, traj, actions, m, n, h, 0.9, program=prog, step_rewards=given)
    with pytest.raises(_lib.L2AError, match="exactly one"):
        _score(term, obs0, traj, actions, m, n, h, 0.9)
    with pytest.raises(_lib.L2AError, match="nothing to write"):
        _score(term, obs0, traj, actions, m, n, h, 0.9, program=prog, keys=False, rets=False, steps=False)
    with pytest.raises(_lib.L2AError, match="range outside the observation"):
        _score(tc.program_of([(od - 1, 2, 0.0, 1.0)]), obs0, traj, actions, m, n, h, 0.9, program=prog)
    with pytest.raises(_lib.L2AError, match="finite"):
        _score(term, obs0, traj, actions, m, n, h, float("nan"), program=prog)
    with pytest.raises(_lib.L2AError, match="too many"):
        _score(term, obs0, traj, actions, m, n, h, 0.9, cand_offset=2 ** 31 - 10, program=prog)


# ------------------------------------------------------------------------------------------
# 4. step_rewards mode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terminal_reward", [0.0, -3.5])
@pytest.mark.parametrize("shape", tc.KERNEL_SHAPES, ids=tc.KERNEL_IDS)
def test_step_rewards_mode_matches_the_restatement(shape, terminal_reward):
    m, n, od, ad, h = shape
    c = _kernel_case(shape, 0.9, terminal_reward)
    given = np.random.RandomState(n).randn(h, m * n).astype(np.float32)
    dead_later = c["steps"] < h
    poisoned = given.copy()
    for row in np.nonzero(dead_later)[0]:
        poisoned[c["steps"][row]:, row] = np.nan                # rewards behind a row's terminal step are not looked at
    want, steps = c["term"].returns_f32(None, c["traj"], None, 0.9, step_rewards=given)
    assert np.array_equal(steps, c["steps"]) and np.isfinite(want).all()
    r, s, keys = _score(c["term"], None, c["traj"], None, m, n, h, 0.9, 1000, step_rewards=poisoned, guard=3)
    assert np.array_equal(_bits(r[3:-3]), _bits(want)) and np.array_equal(s[3:-3], steps)
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), 1000))
    assert (r[:3] == -123.5).all() and (r[-3:] == -123.5).all()


_PLANS = {}


def _plan_inputs(cid, hidden=(64,), act="relu"):
    """Dynamics model, reward model, value model, programs and the oracle's side of a plan case - built once, never modified."""
    if cid not in _PLANS:
        p = dict(tc.plan_case(cid))
        case = p["case"]
        env, model = cases.product_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        base = cases.recipe(case)[2][0]
        r_params, r_norm = rmc.reward_weights(od, ad, hidden), rmc.reward_norm(od, ad, base=base)
        rm = NativeRewardModel(od, ad, hidden, act)
        rm.set_weights(r_params)
        rm.set_norm(r_norm)
        v_params, v_norm = vmc.value_weights(od, (128, 64)), vmc.value_norm(od, base=base, value=(0.5, 20.0))
        vm = NativeValueModel(od, (128, 64), act)
        vm.set_weights(v_params)
        vm.set_norm(v_norm)
        prog = rpc.new_reward_program(od, ad, env.dt)
        spec = reward_spec_for_env(env)
        assert isinstance(spec, RewardSpec)
        p.update(model=model, native=model.planner_model(), rm=rm, vm=vm, vfn=vmc.value_fn(v_params, v_norm, act),
                 term=tc.program_of(p["guards"], -3.5), never=tc.program_of(tc.never_guards(od), -3.5),
                 rewards=dict(spec=(spec, p["reward_fn"]), program=(prog, prog.evaluate),
                              model=(rm, rmc.reward_fn(r_params, r_norm, act))))
        _PLANS[cid] = p
    return _PLANS[cid]


def _plan(p, kind, term, vm=None, coef=1.0, cand_offset=0, lo=None, hi=None, traj=False):
    case, native = p["case"], p["native"]
    m, n, h = case["m"], case["n"], case["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    a = p["actions"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * nl, -1)
    out = torch.full((m, nl), float("nan"), dtype=torch.float32, device=native.device)
    steps = torch.full((m, nl), -77, dtype=torch.int32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    tr = torch.full((h, m * nl, native.obs_dim), float("nan"), dtype=torch.float32, device=native.device) if traj else None
    native.plan_rs_term(_dev(p["obs0"]), _dev(a), m, nl, h, p["discount"], p["rewards"][kind][0], term, value_model=vm,
                        value_coef=coef, cand_offset=cand_offset, returns_out=out, steps_alive_out=steps, best_key=best, traj_out=tr)
    torch.cuda.synchronize()
    assert native.ctx.launch_status_value() == 0
    return out.cpu().numpy(), steps.cpu().numpy(), best.cpu().numpy().view(np.uint64), tr


def test_model_rewards_with_never_firing_guards_are_plan_rs_reward_models_bits():
    """The per-step rewards produced as ``l2a_plan_rs_term`` produces them - one h = 1 scoring call, one predict over the other
    steps - summed by the new kernel under guards that never fire: ``l2a_plan_rs_reward_model``'s returns and keys."""
    p = _plan_inputs("hc_rs_m2_n100_h7_e2_s0")
    case, native, rm = p["case"], p["native"], p["rm"]
    m, n, h, disc = case["m"], case["n"], case["h"], 0.9
    obs0, a = _dev(p["obs0"]), _dev(p["actions"])
    traj = torch.empty((h, m * n, native.obs_dim), dtype=torch.float32, device=native.device)
    want = torch.empty((m, n), dtype=torch.float32, device=native.device)
    want_k = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    native.plan_rs_reward_model(obs0, a, m, n, h, disc, rm, cand_offset=5, returns_out=want, best_key=want_k, traj_out=traj)
    rewards = torch.empty((h, m * n), dtype=torch.float32, device=native.device)
    rm.score_trajectory(obs0, traj[:1], a[:1], m, n, 1, 1.0, cand_offset=5, returns_out=rewards[0])
    rm.predict(traj[:h - 1].reshape(-1, native.obs_dim), a[1:].reshape(-1, native.act_dim), traj[1:].reshape(-1, native.obs_dim),
               out=rewards[1:].reshape(-1))
    torch.cuda.synchronize()
    r, s, keys = _score(p["never"], None, traj.cpu().numpy(), None, m, n, h, disc, 5, step_rewards=rewards.cpu().numpy())
    assert np.array_equal(_bits(r), _bits(want.cpu().numpy().reshape(-1))) and (s == h).all()
    assert np.array_equal(keys, want_k.cpu().numpy().view(np.uint64))
    # and the plan entry itself
    orig = p["discount"]
    try:
        p["discount"] = disc
        r2, s2, k2, _ = _plan(p, "model", p["never"], cand_offset=5)
    finally:
        p["discount"] = orig
    assert np.array_equal(_bits(r2), _bits(want.cpu().numpy())) and np.array_equal(k2, keys) and (s2 == h).all()


# ------------------------------------------------------------------------------------------
# 5. terminal values
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [tc.KERNEL_SHAPES[2], tc.KERNEL_SHAPES[4]], ids=[tc.KERNEL_IDS[2], tc.KERNEL_IDS[4]])
def test_terminal_values_reach_the_survivors_only(shape):
    m, n, od, ad, h = shape
    c = _kernel_case(shape, 0.9, -3.5)
    values = (10.0 * np.random.RandomState(4).randn(m * n)).astype(np.float32)
    want, steps = c["term"].returns_f32(np.repeat(c["obs0"], n, axis=0), c["traj"], c["actions"], 0.9, program=c["prog"],
                                        terminal_values=values, value_coef=0.5)
    alive = tc.survived(c["guards"], c["traj"], steps)
    assert np.array_equal(_bits(want[~alive]), _bits(c["want"][~alive])) and not np.any(_bits(want[alive]) == _bits(c["want"][alive]))
    args = (c["term"], c["obs0"], c["traj"], c["actions"], m, n, h, 0.9, 0)
    r, s, keys = _score(*args, program=c["prog"], values=values, coef=0.5)
    assert np.array_equal(_bits(r), _bits(want)) and np.array_equal(s, steps)
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), 0))
    poison = np.where(alive, values, np.nan).astype(np.float32)     # a dead row's value is not looked at
    r1, _, k1 = _score(*args, program=c["prog"], values=poison, coef=0.5)
    assert np.array_equal(_bits(r1), _bits(want)) and np.array_equal(k1, keys)
    r0, _, k0 = _score(*args, program=c["prog"], values=np.full_like(values, np.nan), coef=0.0)     # w == 0 leaves R
    assert np.array_equal(_bits(r0), _bits(c["want"])) and np.array_equal(k0, _want_keys(c["want"].reshape(m, n), 0))


@pytest.mark.parametrize("kind", ["program", "model"])
def test_never_firing_guards_with_a_value_are_plan_rs_values_bits(kind):
    p = _plan_inputs("hc_rs_m2_n100_h7_e2_s0")
    case, native = p["case"], p["native"]
    m, n, h = case["m"], case["n"], case["h"]
    want = torch.empty((m, n), dtype=torch.float32, device=native.device)
    want_k = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    native.plan_rs_value(_dev(p["obs0"]), _dev(p["actions"]), m, n, h, p["discount"], p["rewards"][kind][0], p["vm"], value_coef=0.5,
                         cand_offset=3, returns_out=want, best_key=want_k)
    r, s, keys, _ = _plan(p, kind, p["never"], vm=p["vm"], coef=0.5, cand_offset=3)
    assert np.array_equal(_bits(r), _bits(want.cpu().numpy())) and np.array_equal(keys, want_k.cpu().numpy().view(np.uint64))
    assert (s == h).all()
    plain, _, _, _ = _plan(p, kind, p["never"], cand_offset=3)
    assert not np.array_equal(_bits(plain), _bits(r))               # the term is there


# ------------------------------------------------------------------------------------------
# 6. the plan step against the float64 oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spec", "program", "model"])
@pytest.mark.parametrize("cid", tc.PLAN_CASES)
def test_plan_follows_the_oracle(cid, kind):
    p = _plan_inputs(cid)
    case = p["case"]
    m, n, h = case["m"], case["n"], case["h"]
    tv = p["vfn"](p["trace"][-1])
    want, steps, ambiguous, alive = tc.plan_want(p, p["rewards"][kind][1], terminal_reward=-3.5, terminal_values=tv, value_coef=0.5)
    assert ambiguous.mean() <= 0.01 and (steps < h).mean() >= 0.20 and alive.mean() >= 0.20
    r, s, keys, traj = _plan(p, kind, p["term"], vm=p["vm"], coef=0.5, traj=True)
    clear = ~ambiguous
    err = rel_err(r.reshape(-1)[clear], want[clear])
    print("%s %s: %d of %d rows ambiguous, %.0f %% terminate early, %.0f %% survive; returns against the float64 oracle %.2e; "
          "trajectory %.2e" % (cid, kind, ambiguous.sum(), m * n, 100 * (steps < h).mean(), 100 * alive.mean(), err,
                               rel_err(traj.cpu().numpy(), p["trace"])))
    assert np.array_equal(s.reshape(-1)[clear], steps[clear])
    assert err < RTOL
    assert np.array_equal(keys, _want_keys(r, 0))                   # the key's index is the arg-max of the GPU's own row
    plain, s2, _, _ = _plan(p, kind, p["term"])                     # without the value: the dead rows' bits do not move
    dead = s.reshape(-1) < h
    assert np.array_equal(s2, s) and np.array_equal(_bits(plain.reshape(-1)[dead]), _bits(r.reshape(-1)[dead]))


# ------------------------------------------------------------------------------------------
# 7. launch geometry and shards
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["program", "model"])
def test_chain_and_single_launch_give_equal_bits(kind):
    p = _plan_inputs("hc_rs_m2_n100_h7_e2_s0")
    ctx = p["native"].ctx
    outs = []
    try:
        for policy in (0, 2):
            ctx.set_micro(policy)
            outs.append(_plan(p, kind, p["term"], vm=p["vm"], coef=0.5))
    finally:
        ctx.set_micro(1)
    (r0, s0, k0, _), (r2, s2, k2, _) = outs
    assert np.array_equal(_bits(r0), _bits(r2)) and np.array_equal(s0, s2) and np.array_equal(k0, k2)


@pytest.mark.parametrize("kind", ["spec", "model"])
@pytest.mark.parametrize("cid", ["hc_rs_ragged_n37_h3_s0", "ant_rs_n300_h6_e3_s0"])
def test_two_shards_combine_to_the_unsharded_plan(cid, kind):
    p = _plan_inputs(cid)
    n = p["case"]["n"]
    cut = n // 2 + 1
    r, s, keys, _ = _plan(p, kind, p["term"], vm=p["vm"], coef=0.5)
    ra, sa, ka, _ = _plan(p, kind, p["term"], vm=p["vm"], coef=0.5, cand_offset=0, lo=0, hi=cut)
    rb, sb, kb, _ = _plan(p, kind, p["term"], vm=p["vm"], coef=0.5, cand_offset=cut, lo=cut, hi=n)
    assert np.array_equal(_bits(np.concatenate([ra, rb], axis=1)), _bits(r))
    assert np.array_equal(np.concatenate([sa, sb], axis=1), s) and np.array_equal(np.maximum(ka, kb), keys)


# ------------------------------------------------------------------------------------------
# 8. through the controller
# ------------------------------------------------------------------------------------------
CTRL_CASE = "hc_rs_m2_n100_h7_e2_s0"


def _controller(with_term=True, **kw):
    p = _plan_inputs(CTRL_CASE)
    case = p["case"]
    env, model = cases.product_model(case)
    if with_term:
        kw.update(termination=p["term"])
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=p["discount"], n_candidates=case["n"],
                         horizon=case["h"], **kw)
    return p, case, env, model, ctrl


def _spy(ctrl, log):
    """Record every rollout's candidates and - asked for or not - its returns table."""
    rollout = ctrl._rollout

    def spy(observations, seq, n_it, cand_offset, want_returns, **kw):
        best, rets = rollout(observations, seq, n_it, cand_offset, True, **kw)
        log.append(dict(seq=seq.clone(), n=n_it, returns=rets.cpu().numpy().copy(), best=best.cpu().numpy().view(np.uint64).copy()))
        return best, (rets if want_returns else None)

    ctrl._rollout = spy


def _entry_table(p, model, snap, m, h):
    """``plan_rs_term`` on a rollout's own candidates."""
    native = model.planner_model()
    out = torch.empty((m, snap["n"]), dtype=torch.float32, device=native.device)
    steps = torch.empty((m, snap["n"]), dtype=torch.int32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    native.plan_rs_term(_dev(p["obs0"]), snap["seq"], m, snap["n"], h, p["discount"], p["rewards"]["spec"][0], p["term"],
                        returns_out=out, steps_alive_out=steps, best_key=best)
    torch.cuda.synchronize()
    return out.cpu().numpy(), steps.cpu().numpy(), best.cpu().numpy().view(np.uint64)


def test_controller_random_shooting_is_plan_rs_term_on_the_drawn_candidates():
    p, case, env, model, ctrl = _controller(rng="numpy")
    m, n, h = case["m"], case["n"], case["h"]
    np.random.seed(0)
    got, info = ctrl.get_actions(p["obs0"])
    native = model.planner_model()
    assert info == {} and native.term_plans == 1 and native.program_plans == 0 and ctrl._program()
    r, s, keys, _ = _plan(p, "spec", p["term"])                     # the case's candidates are this seed's draw
    best = np.array([_lib.key_decode(k)[1] for k in keys])
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, p["actions"][0].reshape(m, n, -1)[np.arange(m), best])
    assert np.array_equal(_bits(ctrl.last_plan["best_return"]), _bits(r[np.arange(m), best]))
    diag = ctrl.termination_diagnostics()
    assert np.array_equal(diag["index"], best) and np.array_equal(diag["steps_alive"], s[np.arange(m), best])
    np.testing.assert_allclose(diag["terminated"], (s < h).mean(axis=1))
    assert 0.0 < diag["terminated"].mean() < 1.0


@pytest.mark.parametrize("planner", ["cem", "mppi", "icem"])
def test_controller_iterating_planners_score_the_entrys_returns(planner):
    kw = dict(cem=dict(use_cem=True, num_cem_iters=1, cem_mode="fixed"), mppi=dict(use_mppi=True, mppi_iters=1),
              icem=dict(use_icem=True, icem_iters=1))[planner]
    p, case, env, model, ctrl = _controller(rng="device", **kw)
    m, h = case["m"], case["h"]
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    action, _ = ctrl.get_actions(p["obs0"])
    native = model.planner_model()
    assert len(log) == 1 and native.term_plans == 1 and np.isfinite(action).all()
    want, steps, keys = _entry_table(p, model, log[0], m, h)
    assert np.array_equal(_bits(log[0]["returns"]), _bits(want)) and np.array_equal(log[0]["best"], keys)
    assert (steps < h).any()
    if planner != "cem":
        assert np.array_equal(_bits(ctrl.last_plan["returns"]), _bits(want))


@pytest.mark.parametrize("which", ["spec", "program"])
def test_controller_without_termination_calls_none_of_the_new_entries(which):
    """No termination anywhere: the entries of the parent commit's path are called, with their bits."""
    p = _plan_inputs(CTRL_CASE)
    case = p["case"]
    m, n, h = case["m"], case["n"], case["h"]
    env, model = cases.product_model(case)
    if which == "program":
        env = rpc.program_env(case["env"], p["rewards"]["program"][0])
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=p["discount"], n_candidates=n, horizon=h, rng="device",
                         native_step=False)
    assert ctrl._termination is None and ctrl._program() == (which == "program")
    log = []
    _spy(ctrl, log)
    torch.manual_seed(5)
    ctrl.get_actions(p["obs0"])
    native = model.planner_model()
    assert native.term_plans == 0 and ctrl.termination_diagnostics() is None and len(log) == 1
    assert native.program_plans == (1 if which == "program" else 0)
    want = torch.empty((m, n), dtype=torch.float32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    plan = native.plan_rs_program if which == "program" else native.plan_rs
    plan(_dev(p["obs0"]), log[0]["seq"], m, n, h, p["discount"], p["rewards"][which][0], returns_out=want, best_key=best)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(log[0]["returns"]), _bits(want.cpu().numpy()))
    assert np.array_equal(log[0]["best"], best.cpu().numpy().view(np.uint64))
