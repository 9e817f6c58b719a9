"""``MPCController(policy_model=...)`` on the GPU: random shooting, CEM (fixed mode) and MPPI pick the policy's proposal where it
is the best candidate by construction, the rows the proposal does not own keep their bits, the proposal composes with every
scoring path behind ``_rollout``, and a relaunch proposes again."""

import numpy as np
import pytest
import torch

import cases
import policy_reference as pr
import reward_model_cases as rmc
import termination_cases as tc
import value_model_cases as vmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPPolicyModel, MLPRewardModel, MLPValueModel
from learning_to_adapt_amd.envs import RewardProgram
from learning_to_adapt_amd.policies import MPCController

pytestmark = pytest.mark.gpu

CASE = dict(env="half_cheetah", mode="single", hidden=[128, 128], E=1)
ENS_CASE = dict(env="half_cheetah", mode="mean", hidden=[128, 128], E=2)
A_BIAS = np.array([0.8, -1.0, 0.4, 0.0, -0.3, 1.1])                  # the policy's normalised output


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _constant_policy(env, norms, hidden=(64,)):
    """A policy with zero kernels: its action is ``a* = fp32(b * fp32(sd_a + 1e-10)) + fp32(mu_a)`` in every state."""
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    pm = MLPPolicyModel(name="pol", env=env, hidden_sizes=hidden, init_seed=0)
    pm.set_params(pr.constant_weights(od, ad, hidden, A_BIAS))
    norm = pr.policy_norm(od, ad, base=norms[0])
    pm.set_normalization(norm)
    sd = (np.asarray(norm["act"][1]) + 1e-10).astype(np.float32)
    a_star = (A_BIAS.astype(np.float32) * sd).astype(np.float32) + np.asarray(norm["act"][0]).astype(np.float32)
    assert np.all(np.abs(a_star) < 0.95)                              # inside the action box: the clip does not move it
    return pm, a_star


def _setup(case=CASE, program=True):
    env, model = cases.product_model(case)
    _, _, norms = cases.recipe(case)
    pm, a_star = _constant_policy(env, norms)
    if program:
        env.reward_spec = RewardProgram().sqsum("act", 0, env.action_space.shape[0], -1.0, target=a_star.astype(np.float64))
    obs = pr.states(5, 2, env.observation_space.shape[0], pm.normalization).astype(np.float64)
    return env, model, norms, pm, a_star, obs


def _controller(env, model, pm=None, n=64, h=4, **kw):
    if pm is not None:
        kw.update(policy_model=pm)
    return MPCController(name="policy", env=env, dynamics_model=model, n_candidates=n, horizon=h, rng="device", native_step=False, **kw)


PLANNERS = {"rs": dict(), "cem": dict(use_cem=True, cem_mode="fixed", num_cem_iters=2, percent_elites=0.1),
            "mppi": dict(use_mppi=True, mppi_kappa=1000.0, mppi_iters=2)}


@pytest.mark.parametrize("planner", list(PLANNERS))
def test_the_policys_proposal_wins_where_it_is_the_best_candidate(planner):
    """Reward ``-|a - a*|^2`` and a policy that plays ``a*``: its rows score 0, every sampled row less."""
    env, model, norms, pm, a_star, obs = _setup()
    n_pi = 3
    torch.manual_seed(123)
    ctrl = _controller(env, model, pm, policy_candidates=n_pi, **PLANNERS[planner])
    native = model.planner_model()
    before = native.policy_proposals
    act, _ = ctrl.get_actions(obs)
    plan = ctrl.last_plan
    assert plan["policy_candidates"] == n_pi and np.all(plan["best_index"] < n_pi), plan["best_index"]
    np.testing.assert_allclose(act, np.broadcast_to(a_star.astype(np.float64), act.shape), rtol=0, atol=2.0 ** -22)
    np.testing.assert_allclose(plan["best_return"], 0.0, atol=1e-10)
    iters = {"rs": 1, "cem": 2, "mppi": 2}[planner]
    assert native.policy_proposals == before + iters and ctrl._pol_calls == iters
    if planner == "rs":
        return
    # the same seed without a policy: the refit / updated mean lies farther from a* than with it
    torch.manual_seed(123)
    plain = _controller(env, model, None, **PLANNERS[planner])
    plain.get_actions(obs)
    key = "cem_mean" if planner == "cem" else "mppi_mean"
    target = np.tile(a_star.astype(np.float64), 4)
    with_pi = np.linalg.norm(plan[key] - target, axis=1)
    without = np.linalg.norm(plain.last_plan[key] - target, axis=1)
    print("%s: |mean - a*| with the policy %s, without %s" % (planner, with_pi, without))
    assert np.all(with_pi < without)
    assert "policy_candidates" not in plain.last_plan and native.policy_proposals == before + iters


def test_rs_rows_beyond_the_proposal_keep_their_bits():
    env, model, norms, pm, a_star, obs = _setup()
    n, n_pi = 64, 5
    tables, cands = [], []
    for policy in (pm, None):
        torch.manual_seed(321)
        ctrl = _controller(env, model, policy, n=n, policy_candidates=n_pi if policy is not None else None)
        ctrl.get_actions(obs)
        a_dev = ctrl._bufs["a_dev"]
        _, rets = ctrl._rollout(obs, a_dev, n, 0, want_returns=True)
        tables.append(rets.cpu().numpy().copy())
        cands.append(a_dev.cpu().numpy().reshape(4, 2, n, -1).copy())
    assert np.array_equal(_bits(cands[0][:, :, n_pi:]), _bits(cands[1][:, :, n_pi:]))
    assert np.array_equal(_bits(tables[0][:, n_pi:]), _bits(tables[1][:, n_pi:]))
    assert not np.array_equal(_bits(cands[0][:, :, :n_pi]), _bits(cands[1][:, :, :n_pi]))
    assert np.all(cands[0][:, :, :n_pi] == a_star) and np.all(tables[0][:, :n_pi] == 0.0)


def _value_model(env, norms):
    od = env.observation_space.shape[0]
    vm = MLPValueModel(name="val", env=env, hidden_sizes=(64, 64), init_seed=0)
    vm.set_params(vmc.value_weights(od, (64, 64)))
    vm.set_normalization(vmc.value_norm(od, base=norms[0]))
    return vm


def _reward_model(env, norms):
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(128, 64), init_seed=0)
    rm.set_params(rmc.reward_weights(od, ad, (128, 64)))
    rm.set_normalization(rmc.reward_norm(od, ad, base=norms[0]))
    return rm


@pytest.mark.parametrize("path", ["fused", "value_model", "termination", "reward_model", "particles", "particles_ts1"])
def test_the_proposal_composes_with_every_scoring_path(path):
    """m = 2, n = 64, h = 4, a policy with weights (its rows differ from step to step) and noise: the score table's policy rows
    are the same controller's scores of those action rows fed in by hand."""
    case = ENS_CASE if path.startswith("particles") else CASE
    env, model = cases.product_model(case)
    _, _, norms = cases.recipe(case)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    pm = MLPPolicyModel(name="pol", env=env, hidden_sizes=(64, 64), init_seed=0)
    pm.set_params(pr.policy_weights(od, ad, (64, 64)))
    pm.set_normalization(pr.policy_norm(od, ad, base=norms[0]))
    kw = {"fused": dict(),            # the env's closed-form RewardSpec in the rollout kernel (`l2a_plan_rs`)
          "value_model": dict(value_model=_value_model(env, norms), terminal_value_coef=0.5),
          "termination": dict(termination=tc.program_of(tc.kernel_guards(od))),
          "reward_model": dict(reward_model=_reward_model(env, norms), use_reward_model=True),
          "particles": dict(ensemble_planning="particles", risk_coef=0.5),
          "particles_ts1": dict(ensemble_planning="particles", particle_sampling="ts1")}[path]
    m, n, h, n_pi = 2, 64, 4, 6
    obs = pr.states(6, m, od, pm.normalization).astype(np.float64)
    torch.manual_seed(7)
    ctrl = _controller(env, model, pm, n=n, h=h, policy_candidates=n_pi, policy_noise=0.05, **kw)
    native = model.planner_model()
    before = native.policy_proposals
    act, _ = ctrl.get_actions(obs)
    assert native.policy_proposals == before + 1 and act.shape == (m, ad) and np.isfinite(act).all()
    a_dev = ctrl._bufs["a_dev"]
    rows = a_dev.reshape(h, m, n, ad)[:, :, :n_pi].contiguous().reshape(h, m * n_pi, ad)
    assert float(rows.std()) > 0.01                       # (a real policy: the rows are not one constant)
    if path == "particles_ts1":
        # every `_rollout` call takes the next permutation slots, and a candidate's slot depends on its place in the launch:
        # pin the stream position, and compare the proposal rows inside a launch of the same width
        ctrl._ts1_calls = 0
        _, table = ctrl._rollout(obs, a_dev, n, 0, want_returns=True)
        table = table.cpu().numpy().copy()
        by_hand = a_dev.clone()
        by_hand.reshape(h, m, n, ad)[:, :, n_pi:] = 0.0
        ctrl._ts1_calls = 0
        _, again = ctrl._rollout(obs, by_hand, n, 0, want_returns=True)
        assert np.array_equal(_bits(table[:, :n_pi]), _bits(again.cpu().numpy()[:, :n_pi]))
        return
    _, table = ctrl._rollout(obs, a_dev, n, 0, want_returns=True)
    table = table.cpu().numpy().copy()
    _, small = ctrl._rollout(obs, rows, n_pi, 0, want_returns=True)
    assert np.array_equal(_bits(table[:, :n_pi]), _bits(small.cpu().numpy()))
    assert np.isfinite(table).all()


@pytest.fixture
def _fresh_split_state():
    """The context's tile-split state as a fresh process has it, before and after (as tests/test_gpu_parity.py restores it)."""
    ctx = _lib.Context.get(0)

    def fresh():
        ctx.set_spin_limit(0)
        ctx.set_split(1)
        ctx.split_degraded = False
        ctx.launch_status_value()
    fresh()
    yield ctx
    fresh()


@pytest.mark.parametrize("planner", list(PLANNERS))
def test_a_relaunch_proposes_again(planner, _fresh_split_state):
    ctx = _fresh_split_state
    env, model, norms, pm, a_star, obs = _setup()
    torch.manual_seed(55)
    ctrl = _controller(env, model, pm, policy_candidates=4, **PLANNERS[planner])
    native = model.planner_model()
    first, _ = ctrl.get_actions(obs)
    calls = ctrl._pol_calls
    assert native.policy_proposals == calls == {"rs": 1, "cem": 2, "mppi": 2}[planner]
    # a launch flagged invalid: the step repeats itself unsplit, proposal included
    ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
    second, _ = ctrl.get_actions(obs)
    assert ctx.split_degraded is True
    assert ctrl._pol_calls == 3 * calls and native.policy_proposals == 3 * calls, "the flagged step did not propose again"
    assert np.all(ctrl.last_plan["best_index"] < 4)
    np.testing.assert_allclose(second, first, rtol=0, atol=2.0 ** -22)
    # force_unsplit, then plan again
    ctrl._force_unsplit()
    third, _ = ctrl.get_actions(obs)
    assert ctrl._pol_calls == 4 * calls and native.policy_proposals == 4 * calls
    assert np.all(ctrl.last_plan["best_index"] < 4)
    np.testing.assert_allclose(third, first, rtol=0, atol=2.0 ** -22)
