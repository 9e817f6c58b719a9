"""Particle plans without a GPU: the C entry points' declarations, the two restatements of ``tests/particle_reference.py`` against
each other and against E single-member oracle rollouts, the oracle's choices of the risk recipes, and every argument check of
``MPCController(ensemble_planning=..., risk_coef=...)``.

Two kinds of test live here.  The declaration, keyword and argument tests (``test_entry_points_...``, ``test_scorer_refuses_...``,
``test_defaults_...``, ``test_particles_keyword_...``, ``test_particles_argument_errors``, ``test_recurrent_controller_...``) exercise
the product and fail without the feature.  The others - fp32 against float64, the edge rows, per-block = E single rollouts, the
risk recipes - touch ``tests/particle_reference.py`` and the oracle only: they pin the REFERENCE the GPU tests judge the product
by, pass on any commit that has that file, and are no coverage of the product."""

import ctypes
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import cases
import particle_reference as pr
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs.synthetic_env import SyntheticEnv
from learning_to_adapt_amd.utils import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("l2a_particle_score", "l2a_plan_rs_particles", "l2a_plan_rs_particles_program", "l2a_plan_rs_particles_reward_model")


def _case(E=3, mode="mean", planner="rs", hidden=(128, 128)):
    return dict(env="half_cheetah", mode=mode, hidden=hidden, E=E, n=50, h=7, planner=planner)


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    lib = _lib.load()
    c = ctypes
    vp, i32, f32 = c.c_void_p, c.c_int, c.c_float
    tail = [f32, i32, vp, vp, vp, vp, vp]
    want = {
        "l2a_particle_score": [vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, vp],
        "l2a_plan_rs_particles": [vp, vp, vp, i32, i32, i32, c.c_double, None] + tail,
        "l2a_plan_rs_particles_program": [vp, vp, vp, i32, i32, i32, c.c_double, None] + tail,
        "l2a_plan_rs_particles_reward_model": [vp, vp, vp, vp, i32, i32, i32, c.c_double] + tail,
    }
    for name in SYMBOLS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl, name + " is not declared in include/l2a.h"
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)                     # the library exports it
        assert fn.restype is i32
        assert len(fn.argtypes) == len(want[name]) == decl.group(1).count(",") + 1, name
        for got, exp in zip(fn.argtypes, want[name]):
            assert exp is None or got is exp, name
    tails = [re.search(r"\bint %s\(([^;]*)\);" % n, text).group(1).split("float lambda")[1] for n in SYMBOLS[1:]]
    assert len(set(re.sub(r"\s+", " ", t) for t in tails)) == 1, "the three plan entries do not share their tail"


def test_scorer_refuses_without_a_context():
    lib = _lib.load()
    assert lib.l2a_particle_score(None, None, 1, 1, 1, ctypes.c_float(0.0), 0, None, None, None, None) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_particles(None, None, None, 1, 1, 1, 1.0, None, ctypes.c_float(0.0), 0, None, None, None, None,
                                     None) == _lib.L2A_EINVAL


@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0, 4.0, -2.0])
def test_fp32_restatement_agrees_with_float64(lam):
    rs = np.random.RandomState(int(lam * 10) + 100)
    worst = 0.0
    for E in (1, 2, 3, 5, 8):
        for scale, offset in ((3.0, 0.0), (1e-3, 50.0), (1e4, -2e4)):
            R = pr.random_table(rs, 3, E, 257, scale, offset)
            s32, d32 = pr.score_f32(R, lam)
            s64, d64, _ = pr.score64(R, lam)
            bound = pr.score_bound(R, lam)
            worst = max(worst, float(np.max(np.abs(s32.astype(np.float64) - s64) / bound)))
            assert np.all(np.abs(s32.astype(np.float64) - s64) <= bound), (E, scale, offset)
            assert np.all(np.abs(d32.astype(np.float64) - d64) <= pr.score_bound(R, 0.0)), (E, scale, offset)
    print("particle score fp32 vs float64, lambda=%g: worst error / bound %.3f" % (lam, worst))


def test_fp32_restatement_edge_rows():
    R = np.array([[[1.0, 2.0, np.nan, np.inf, -np.inf, np.inf, 5.0],
                   [1.0, 2.0, 0.0, 1.0, 1.0, -np.inf, 5.0],
                   [1.0, 2.0, 0.0, 1.0, 1.0, 0.0, 5.0]]], dtype=np.float32)
    s0, d0 = pr.score_f32(R, 0.0)
    assert s0[0, 0] == 1.0 and d0[0, 0] == 0.0 and d0[0, 6] == 0.0            # identical members: spread exactly 0
    assert np.isnan(s0[0, 2]) and s0[0, 3] == np.inf and s0[0, 4] == -np.inf and np.isnan(s0[0, 5])
    assert np.isnan(d0[0, 3]) and np.isnan(d0[0, 4])
    s1, _ = pr.score_f32(R, 1.0)
    assert s1[0, 0] == 1.0 and np.isnan(s1[0, 3]) and np.isnan(s1[0, 4])
    assert pr.argmax_nan_first(s0[0]) == 2 and pr.argmax_nan_first(s1[0]) == 2
    _, idx = _lib.key_decode(int(pr.keys(s0, cand_offset=7)[0]))
    assert idx == 7 + 2
    ties = np.array([[[1.0, 3.0, 3.0, 2.0]]], dtype=np.float32)
    assert _lib.key_decode(int(pr.keys(pr.score_f32(ties, 0.0)[0])[0]))[1] == 1     # lowest index wins


def test_per_block_restatement_is_e_single_member_rollouts():
    from oracle import OracleMLPDynamics, planner
    env = SyntheticEnv("half_cheetah")
    E, m, n, h = 3, 2, 9, 4
    sets, norms = synthetic.make_members(env, (32, 32), E)
    np.random.seed(5)
    obs = synthetic.make_obs0(m, 20)
    actions = planner.sample_rs_actions(env.action_space.low, env.action_space.high, n, m, h)
    got = pr.member_returns64(env, sets, norms, obs, actions, n, discount=0.9)
    for e in range(E):
        one = OracleMLPDynamics(20, 6, [sets[e]], [norms[e]], mode="single")
        want = planner.rollout_returns(one, env.reward, obs, actions, n, 0.9).reshape(m, n)
        assert np.array_equal(got[:, e], want), e


@pytest.mark.parametrize("E,seed,want", pr.RISK_RECIPES)
def test_oracle_choices_of_the_risk_recipes(E, seed, want):
    """The candidates the GPU test holds the controller to.  Their margins decide that test: a GPU score within the bar,
    (1 + lambda) 1e-4 max |R|, of the oracle's cannot change the winner when the best two lie more than twice that apart."""
    from oracle import planner
    env = SyntheticEnv("half_cheetah")
    sets, norms = synthetic.make_members(env, (128, 128), E)
    np.random.seed(seed)
    obs = synthetic.make_obs0(1, 20)
    actions = planner.sample_rs_actions(env.action_space.low, env.action_space.high, 50, 1, 7)
    R = pr.member_returns64(env, sets, norms, obs, actions, 50)
    scale = np.max(np.abs(R))
    for lam, idx in zip(pr.RISK_LAMBDAS, want):
        score = pr.score64(R, lam)[0][0]
        order = np.argsort(-score)
        assert order[0] == idx, (lam, order[:3])
        margin = (score[order[0]] - score[order[1]]) / scale
        print("risk recipe E=%d seed=%d lambda=%g: candidate %d, margin %.2e of max |R|" % (E, seed, lam, idx, margin))
        assert margin > 2 * (1 + lam) * 1e-4, (lam, margin)


# ------------------------------------------------------------------------------------------------------ controller arguments
def test_defaults_change_nothing():
    from learning_to_adapt_amd.policies import MPCController, RNNMPCController
    params = inspect.signature(MPCController.__init__).parameters
    assert params["ensemble_planning"].default == "mean" and params["risk_coef"].default == 0.0
    assert inspect.signature(RNNMPCController.__init__).parameters["ensemble_planning"].default == "mean"
    ctrl = cases.product_controller(_case())
    assert ctrl.ensemble_planning == "mean" and ctrl.risk_coef == 0.0 and not ctrl._program()
    assert ctrl.particle_diagnostics() is None


def test_particles_keyword_and_pickle():
    ctrl = cases.product_controller(_case(E=2), ensemble_planning="particles", risk_coef=1.5)
    assert ctrl.ensemble_planning == "particles" and ctrl.risk_coef == 1.5
    assert ctrl._program()                  # every path around `_rollout` declines: blocking launch, pipelines, C controllers
    assert ctrl.native_step is True         # (the default C step steps aside silently)
    back = pickle.loads(pickle.dumps(ctrl))
    assert back.ensemble_planning == "particles" and back.risk_coef == 1.5
    assert cases.product_controller(_case(planner="cem"), ensemble_planning="particles")._program()
    assert cases.product_controller(_case(), rng="device", use_mppi=True, ensemble_planning="particles")._program()


def test_particles_argument_errors():
    with pytest.raises(_lib.L2AError, match="ensemble"):
        cases.product_controller(_case(E=1, mode="single"), ensemble_planning="particles")
    with pytest.raises(_lib.L2AError, match="ensemble"):
        cases.product_controller(_case(E=2, mode="per_block"), ensemble_planning="particles")
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="risk_coef"):
            cases.product_controller(_case(), ensemble_planning="particles", risk_coef=bad)
        with pytest.raises(ValueError, match="risk_coef"):
            cases.product_controller(_case(), risk_coef=bad)
    with pytest.raises(ValueError, match="ensemble_planning"):
        cases.product_controller(_case(), ensemble_planning="ts1")
    with pytest.raises(_lib.L2AError, match="native_cem_step"):
        cases.product_controller(_case(planner="cem"), rng="device", ensemble_planning="particles", native_cem_step=True)
    with pytest.raises(_lib.L2AError, match="native_mppi_step"):
        cases.product_controller(_case(), rng="device", use_mppi=True, ensemble_planning="particles", native_mppi_step=True)
    cases.product_controller(_case(planner="cem"), rng="device", native_cem_step=True)       # (fine without particles)


def test_recurrent_controller_refuses_particles():
    name = cases.rnn_case_ids()[0]
    case, _ = cases.split_id(name)
    with pytest.raises(_lib.L2AError, match="ensemble"):
        cases.product_rnn_controller(dict(case, planner="rnn_rs"), ensemble_planning="particles")
    assert cases.product_rnn_controller(dict(case, planner="rnn_rs")).ensemble_planning == "mean"
