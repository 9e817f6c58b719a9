"""Reward programs on the GPU: the trajectory-scoring kernel bit for bit against its float32 restatement, the plan
step (``l2a_plan_rs_program``) against the float64 oracle, its independence of launch geometry and sharding, and the
controller's routing."""

import ctypes

import numpy as np
import pytest
import torch

import cases
import cem_ties
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs import RewardProgram

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # returns against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _ctx():
    return _lib.Context.get(0)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


def _inputs(seed, m, n, od, ad, h):
    """Random inputs of magnitude 0.1 .. 10 with random signs (away from subnormals)."""
    rs = np.random.RandomState(seed)

    def draw(*shape):
        return (rs.uniform(0.1, 10.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
    return draw(m, od), draw(h, m * n, od), draw(h, m * n, ad)


def _score(prog, obs0, traj, actions, m, n, h, discount, cand_offset, guard=0):
    rets = torch.full((guard + m * n + guard,), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    _ctx().score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, discount, prog, cand_offset=cand_offset,
                            returns_out=rets[guard:guard + m * n], best_key=best)
    torch.cuda.synchronize()
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64)


SCORE_SHAPES = [(1, 64, 20, 6, 3),          # whole block
                (1, 33, 17, 5, 1),          # ragged block, odd dims, h = 1
                (3, 70, 41, 8, 4),          # blocks straddling env boundaries
                (2, 130, 64, 16, 2)]        # the dimension limits of the matrix-core rollout kernels


# ------------------------------------------------------------------------------------------
# 1. the score kernel alone, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("m,n,od,ad,h", SCORE_SHAPES)
def test_score_kernel_is_bit_identical_to_its_restatement(m, n, od, ad, h, discount, cand_offset):
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = _inputs(10 + n, m, n, od, ad, h)
    want = prog.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, discount)
    rets, keys = _score(prog, obs0, traj, actions, m, n, h, discount, cand_offset)
    assert np.isfinite(want).all()
    assert np.array_equal(rets.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), cand_offset))


def test_score_kernel_unaligned_steps_and_keys_only():
    """A step of an odd number of odd rows starts off a 16-byte boundary (dword staging of whole blocks), and a call may
    ask for the keys alone or the returns alone."""
    m, n, od, ad, h = 1, 129, 17, 5, 3
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = _inputs(5, m, n, od, ad, h)
    want = prog.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, 0.9)
    rets, keys = _score(prog, obs0, traj, actions, m, n, h, 0.9, 7)
    assert np.array_equal(rets.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), 7))
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    _ctx().score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, 0.9, prog, cand_offset=7, best_key=best)
    torch.cuda.synchronize()
    assert np.array_equal(best.cpu().numpy().view(np.uint64), keys)
    with pytest.raises(_lib.L2AError):
        _ctx().score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, 0.9, prog)
    bad = RewardProgram().linear("obs", od, 1.0)
    with pytest.raises(_lib.L2AError, match="range"):
        _ctx().score_trajectory(_dev(obs0), _dev(traj), _dev(actions), m, n, h, 0.9, bad, best_key=best)


# ------------------------------------------------------------------------------------------
# 2. ties and non-finite returns
# ------------------------------------------------------------------------------------------
def test_score_kernel_ties_nan_and_guards():
    m, n, od, ad, h = 1, 64, 20, 6, 3
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = _inputs(3, m, n, od, ad, h)
    base = prog.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, 1.0)
    top = int(np.argmax(base))
    # two identical candidates: the lower index wins
    twin = (top + 17) % n
    traj2, act2 = traj.copy(), actions.copy()
    traj2[:, twin], act2[:, twin] = traj[:, top], actions[:, top]
    rets, keys = _score(prog, obs0, traj2, act2, m, n, h, 1.0, 0, guard=8)
    assert np.all(rets[:8] == -123.5) and np.all(rets[-8:] == -123.5)          # guard rows untouched
    assert rets[8 + twin] == rets[8 + top] == base[top]
    assert _lib.key_decode(keys[0])[1] == min(top, twin)
    # one candidate's trajectory holds a NaN: it wins, as np.argmax has it
    traj3 = traj.copy()
    traj3[1, 41, 3] = np.nan
    want = prog.returns_f32(np.repeat(obs0, n, axis=0), traj3, actions, 1.0)
    rets, keys = _score(prog, obs0, traj3, actions, m, n, h, 1.0, 0)
    assert np.isnan(want[41]) and int(np.argmax(want)) == 41
    assert np.array_equal(np.isnan(rets), np.isnan(want)) and _lib.key_decode(keys[0])[1] == 41
    assert np.array_equal(keys, _want_keys(want.reshape(m, n), 0))
    # all returns -inf: index 0
    act4 = actions.copy()
    act4[0, :, 2] = np.inf
    rets, keys = _score(prog, obs0, traj, act4, m, n, h, 1.0, 0)
    assert np.all(rets == -np.inf) and _lib.key_decode(keys[0])[1] == 0
    assert keys[0] == _encode(-np.inf, 0)


# ------------------------------------------------------------------------------------------
# 3. the plan step against the float64 oracle
# ------------------------------------------------------------------------------------------
PLAN_CASES = ["hc_rs_ragged_n37_h3_s0", "hc_rs_discount_s0", "ant_rs_4x256_e2_s0", "ant_rs_n300_h6_e3_s0"]
_PLANS = {}


def _plan_inputs(cid):
    """Model, candidates and the oracle's trace of a golden case - computed once, shared and never modified."""
    if cid not in _PLANS:
        from oracle.planner import sample_rs_actions
        case, seed = cases.split_id(cid)
        env, model = cases.product_model(case)
        np.random.seed(seed)
        actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
        _PLANS[cid] = dict(case=case, env=env, model=model, actions=actions, gold=cases.load_golden(cid),
                           dyn=cases.oracle_dynamics(case))
    return _PLANS[cid]


def _plan_program(p, prog, cand_offset=0, lo=None, hi=None, want_traj=True):
    case, native = p["case"], p["model"].planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    a = p["actions"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * nl, -1)
    rets = torch.full((m, nl), float("nan"), dtype=torch.float32, device=native.device)
    best = torch.full((m,), -1, dtype=torch.int64, device=native.device)
    traj = torch.full((h, m * nl, native.obs_dim), float("nan"), dtype=torch.float32, device=native.device) if want_traj else None
    native.plan_rs_program(_dev(p["gold"]["obs0"]), _dev(a), m, nl, h, case.get("discount", 1.0), prog, cand_offset=cand_offset,
                           returns_out=rets, best_key=best, traj_out=traj)
    torch.cuda.synchronize()
    assert native.ctx.launch_status_value() == 0
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64), (traj.cpu().numpy() if want_traj else None), a


@pytest.mark.parametrize("cid", PLAN_CASES)
def test_plan_step_with_the_cases_own_reward(cid):
    p = _plan_inputs(cid)
    case, env, gold = p["case"], p["env"], p["gold"]
    prog = RewardProgram.from_spec(env.reward_spec, env.observation_space.shape[0], env.action_space.shape[0])
    rets, keys, _, _ = _plan_program(p, prog)
    err = rel_err(rets, gold["returns"])
    print("%s: returns against the golden table %.2e" % (cid, err))
    assert err < RTOL
    for i in range(case["m"]):
        ret, idx = _lib.key_decode(keys[i])
        assert idx == int(gold["best"][i]) == int(np.argmax(rets[i]))
        assert np.float32(ret) == rets[i, idx]


@pytest.mark.parametrize("cid", PLAN_CASES)
def test_plan_step_with_a_new_reward(cid):
    from oracle.planner import rollout_trace
    p = _plan_inputs(cid)
    case, env, gold = p["case"], p["env"], p["gold"]
    m, n, h, disc = case["m"], case["n"], case["h"], case.get("discount", 1.0)
    prog = rpc.new_reward_program(env.observation_space.shape[0], env.action_space.shape[0], env.dt)
    want, states = rollout_trace(p["dyn"], prog.evaluate, gold["obs0"], p["actions"], n, disc)
    rets, keys, traj, a32 = _plan_program(p, prog)
    err_r, err_s = rel_err(rets.reshape(-1), want), rel_err(traj, states)
    print("%s: returns %.2e, states %.2e against the float64 oracle" % (cid, err_r, err_s))
    assert err_r < RTOL and err_s < RTOL
    # the returns ARE the fixed fp32 arithmetic applied to the trajectory that was written out
    again = prog.returns_f32(np.repeat(gold["obs0"].astype(np.float32), n, axis=0), traj, a32.astype(np.float32), disc)
    assert np.array_equal(rets.reshape(-1).view(np.uint32), again.view(np.uint32))
    assert np.array_equal(keys, _want_keys(rets, 0))
    # the library's own trajectory buffer gives the same bits
    rets2, keys2, _, _ = _plan_program(p, prog, want_traj=False)
    assert np.array_equal(rets2.view(np.uint32), rets.view(np.uint32)) and np.array_equal(keys2, keys)


# ------------------------------------------------------------------------------------------
# 4. geometry independence
# ------------------------------------------------------------------------------------------
@pytest.fixture
def _split_policy():
    ctx = _ctx()
    yield ctx
    ctx.set_split(0 if getattr(ctx, "split_degraded", False) else 1)


@pytest.mark.parametrize("cid", ["hc_rs_m2_n100_h7_e2_s0", "ant_rs_n300_h6_e3_s0"])
def test_plan_step_does_not_depend_on_the_launch_geometry(cid, _split_policy):
    p = _plan_inputs(cid)
    env = p["env"]
    prog = rpc.new_reward_program(env.observation_space.shape[0], env.action_space.shape[0], env.dt)
    rets, keys, traj, _ = _plan_program(p, prog)
    _split_policy.set_split(0)
    rets0, keys0, traj0, _ = _plan_program(p, prog)
    assert np.array_equal(rets0.view(np.uint32), rets.view(np.uint32)) and np.array_equal(keys0, keys)
    assert np.array_equal(traj0.view(np.uint32), traj.view(np.uint32))


@pytest.mark.parametrize("cid", ["hc_rs_m2_n100_h7_e2_s0", "ant_rs_n300_h6_e3_s0"])
def test_two_shards_combine_to_the_unsharded_plan(cid):
    p = _plan_inputs(cid)
    env, n = p["env"], p["case"]["n"]
    prog = rpc.new_reward_program(env.observation_space.shape[0], env.action_space.shape[0], env.dt)
    rets, keys, _, _ = _plan_program(p, prog, want_traj=False)
    ra, ka, _, _ = _plan_program(p, prog, cand_offset=0, lo=0, hi=n // 2, want_traj=False)
    rb, kb, _, _ = _plan_program(p, prog, cand_offset=n // 2, lo=n // 2, hi=n, want_traj=False)
    both = np.concatenate([ra, rb], axis=1)
    assert np.array_equal(both.view(np.uint32), rets.view(np.uint32))
    assert np.array_equal(np.maximum(ka, kb), keys)


# ------------------------------------------------------------------------------------------
# 5. through the controller
# ------------------------------------------------------------------------------------------
def _controller(cid, program=True, **kw):
    case, seed = cases.split_id(cid)
    env, model = cases.product_model(case)
    if program:
        env = rpc.program_env(case["env"])
    kw.setdefault("use_cem", False)
    from learning_to_adapt_amd.policies import MPCController
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0),
                         n_candidates=case["n"], horizon=case["h"], **kw)
    return case, seed, env, model, ctrl


@pytest.mark.parametrize("cid", ["hc_rs_m3_n64_h5_s0", "ant_rs_n300_h6_e3_s0"])
def test_controller_plans_a_program_env_like_the_oracle(cid):
    from oracle.planner import rs_plan
    case, seed, env, model, ctrl = _controller(cid, rng="numpy")
    gold = cases.load_golden(cid)
    np.random.seed(seed)
    want, best, returns, _ = rs_plan(cases.oracle_dynamics(case), env.reward, gold["obs0"], env.action_space.low,
                                     env.action_space.high, case["n"], case["h"], case.get("discount", 1.0))
    state = np.random.get_state()
    top = np.sort(returns, axis=1)
    assert np.all((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1])) > 2 * RTOL)       # no declared near-tie
    np.random.seed(seed)
    got, info = ctrl.get_actions(gold["obs0"])
    after = np.random.get_state()
    assert info == {} and model.planner_model().program_plans == 1
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert rel_err(ctrl.last_plan["best_return"], returns[np.arange(case["m"]), best]) < RTOL
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_controller_cem_on_a_program_env():
    from oracle.planner import cem_plan
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, ctrl = _controller(cid, rng="numpy", use_cem=True, num_cem_iters=1)
    gold = cases.load_golden(cid)
    m, n = case["m"], case["n"]
    np.random.seed(seed)
    want, best, returns = cem_plan(cases.oracle_dynamics(case), env.reward, gold["obs0"], env.action_space.low,
                                   env.action_space.high, n, case["h"], case.get("discount", 1.0), num_cem_iters=1)
    np.random.seed(seed)
    got, _ = ctrl.get_actions(gold["obs0"])                 # raised L2AError before reward programs
    assert model.planner_model().program_plans >= 1
    mine = ctrl.last_plan["cem_trace"][0]["returns"]
    assert rel_err(mine, returns) < RTOL
    cem_ties.assert_flips_are_ties(mine, returns, max(int(n * 0.1), 1), RTOL)      # every rank swap has a witness pair
    idx = np.asarray(ctrl.last_plan["best_index"])
    for i in range(m):
        if idx[i] == best[i]:
            np.testing.assert_array_equal(got[i], want[i])
        else:       # a witnessed tie at the very top
            assert abs(returns[i, idx[i]] - returns[i, best[i]]) <= 2 * RTOL * max(1.0, abs(returns[i, best[i]]))


def test_a_reward_spec_env_keeps_its_old_path():
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, ctrl = _controller(cid, program=False, rng="numpy")
    gold = cases.load_golden(cid)
    np.random.seed(seed)
    got, _ = ctrl.get_actions(gold["obs0"])
    assert model.planner_model().program_plans == 0 and not ctrl._program()
    assert np.array_equal(ctrl.last_plan["best_index"], gold["best"])
    np.testing.assert_array_equal(got, gold["chosen"])
    assert rel_err(ctrl.last_plan["best_return"], gold["returns"][np.arange(case["m"]), gold["best"]]) < RTOL
