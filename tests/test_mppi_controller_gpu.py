"""The reward-weighted (MPPI) planner through the controllers on the GPU: ``MPCController(use_mppi=True, rng="device")`` and
``RNNMPCController(use_mppi=True, rng="device")`` on the small golden-case models (one MLP, one 5-member mean ensemble, one LSTM).

Every step is judged in two halves, as CEM's refit is: the returns against the float64 oracle rolled on the product's OWN candidates
(the project's bar, 1e-4 relative), and the update (action, mean, effective sample size) against ``mppi_reference`` on the
product's own returns, within ``mppi_reference.update_bounds``.  The samples are checked bit for bit where the normals are
injected and within the Philox bound of ``tests/test_mppi_kernels_gpu.py`` where the device draws them."""

import numpy as np
import pytest
import torch

import cases
import mppi_reference as mr
from learning_to_adapt_amd import _lib
from oracle import LSTMStateTuple, make_reward
from oracle.planner import rollout_returns
from oracle.rnn_planner import rnn_rollout_returns
from test_cem_kernels_gpu import PHILOX_ATOL

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # returns against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
MODELS = {"mlp": dict(cases.CASES["hc_rs_m3_n64_h5"]),
          "ens5": dict(cases.CASES["c2_hc_rs_n2000_h30_e5"], n=96, h=6),        # the 5-member mean ensemble on a small plan
          "long": dict(cases.CASES["hc_rs_m3_n64_h5"], h=90)}   # l2a_mppi_sample_k walks this horizon in two passes (85 + 5 at A = 6)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _obs(which):
    case = MODELS[which]
    return cases.load_golden("%s_s%d" % (case["name"], case["seeds"][0]))["obs0"]


def _controller(which, **kw):
    case = MODELS[which]
    return case, cases.product_controller(case, rng="device", use_mppi=True, **kw)


def _inject(ctrl, zs):
    it = iter(zs)
    ctrl._mppi_normal_device = lambda shape, device: torch.from_numpy(np.ascontiguousarray(next(it), dtype=np.float32)).to(device)


def _samples(ctrl):
    """The product's own samples and candidates of the last iteration."""
    return ctrl._bufs["mppi_a_clip"].cpu().numpy(), ctrl._bufs["mppi_seq"].cpu().numpy()


def _oracle_returns(case, obs, seq):
    env, _, _ = cases.recipe(case)
    dyn = cases.oracle_dynamics(case)
    rets = rollout_returns(dyn, make_reward(case["env"], env.dt), obs, seq.astype(np.float64), case["n"], case.get("discount", 1.0))
    return rets.reshape(len(obs), case["n"])


def _check_update(ctrl, action, mean_before, a_clip, kappa, what):
    """Action, mean, ESS, index and counts of the last step against the reference on the product's own samples and returns."""
    plan = ctrl.last_plan
    n, ad = a_clip.shape[0], action.shape[1]
    ref = mr.result_row(mean_before, a_clip, plan["returns"], kappa, ad)
    bound, rel = mr.update_bounds(n, kappa, float(np.max(np.abs(a_clip))), mr.sum_chain(n))
    assert action.dtype == np.float64 and np.array_equal(action, plan["mppi_mean"][:, :ad].astype(np.float64)), what
    assert np.array_equal(plan["best_index"], ref["index"]) and np.array_equal(plan["mppi_valid"], ref["valid"]), what
    assert np.array_equal(_bits(plan["best_return"]), _bits(ref["rmax"])), what
    err = float(np.max(np.abs(plan["mppi_mean"].astype(np.float64) - ref["mean"])))
    ess = float(np.max(np.abs(plan["mppi_ess"].astype(np.float64) - ref["ess"]) / ref["ess"]))
    print("\n[mppi] %s: mean error / bound %.3f, ESS error / bound %.3f, ESS %s of %d" % (what, err / bound, ess / rel, plan["mppi_ess"], n))
    assert err <= bound and ess <= rel, what


def _sample_bound(mean_shifted, z64, sigma, beta, h):
    """``PHILOX_ATOL sigma_k + 4 2^-24 (|mu'| + U / beta)`` (tests/test_mppi_kernels_gpu.py)."""
    sig = np.tile(sigma.astype(np.float64), h)
    U = float(np.max(np.abs(z64 * sig)))
    return PHILOX_ATOL * sig[None, None] + 4 * 2.0 ** -24 * (np.abs(mean_shifted)[None] + U / float(np.float32(beta)))


# ------------------------------------------------------------------------------------------------- injected normals, one step
@pytest.mark.parametrize("which", ["mlp", "ens5", "long"])
def test_single_step_with_injected_normals(which):
    case, ctrl = _controller(which)
    obs = _obs(which)
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    z = np.random.RandomState(3).randn(n, m, D).astype(np.float32)
    _inject(ctrl, [z])
    action, info = ctrl.get_actions(obs)
    assert info == {} and action.shape == (m, ad)
    a_clip, seq = _samples(ctrl)
    sigma = ctrl._mppi_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    _, want_a, want_seq = mr.sample_f32(np.zeros((m, D), dtype=np.float32), -np.ones(m, dtype=np.int32), z, sigma, ctrl.mppi_beta, low,
                                        high, n, m, h, ad)
    assert np.array_equal(_bits(a_clip), _bits(want_a)) and np.array_equal(_bits(seq), _bits(want_seq))
    err = rel_err(ctrl.last_plan["returns"], _oracle_returns(case, obs, seq))
    print("\n[mppi] %s: returns against the float64 oracle %.2e" % (which, err))
    assert err < RTOL
    _check_update(ctrl, action, np.zeros((m, D), dtype=np.float32), a_clip, ctrl.mppi_kappa, which)
    assert np.all(action >= low) and np.all(action <= high)
    assert ctrl._bufs["mppi_calls"] == 1


# ----------------------------------------------------------------------------------------------------- three consecutive steps
def _replay_steps(which, steps):
    seed = 1234
    torch.manual_seed(seed)
    case, ctrl = _controller(which, mppi_kappa=0.5)
    obs = _obs(which)
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    sigma = ctrl._mppi_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    mean = np.zeros((m, D), dtype=np.float32)
    rs = np.random.RandomState(0)
    means = []
    for s in range(steps):
        action, _ = ctrl.get_actions(obs)
        a_clip, seq = _samples(ctrl)
        z64 = mr.philox_normal(seed, mr.philox_indices(s * n * m * D, n * m * D)).reshape(n, m, D)
        shift = np.full(m, -1 if s == 0 else 1, dtype=np.int32)
        shifted, want_a, _ = mr.sample(mean, shift, z64, sigma, ctrl.mppi_beta, low, high, n, m, h, ad)
        bound = _sample_bound(shifted, z64, sigma, ctrl.mppi_beta, h)
        r = float(np.max(np.abs(a_clip.astype(np.float64) - want_a) / bound))
        print("\n[mppi] step %d: sample error / bound %.3f" % (s, r))
        assert r <= 1.0, "step %d does not sample the shifted mean at offset %d" % (s, s * n * m * D)
        assert np.array_equal(_bits(seq), _bits(a_clip).reshape(-1)[mr.seq_index(n, m, h, ad)])
        err = rel_err(ctrl.last_plan["returns"], _oracle_returns(case, obs, seq))
        print("[mppi] %s step %d: returns against the float64 oracle %.2e" % (which, s, err))
        assert err < RTOL
        _check_update(ctrl, action, shifted.astype(np.float32), a_clip, 0.5, "%s step %d" % (which, s))
        mean = ctrl.last_plan["mppi_mean"]
        means.append(mean.copy())
        obs = obs + 0.01 * rs.randn(*obs.shape)
    assert ctrl._bufs["mppi_calls"] == steps
    return means


def test_three_steps_replayed_with_the_philox_normals():
    """Step ``s`` draws at offset ``s n m D`` under ``torch.initial_seed()`` and samples around the previous step's mean moved on
    one step."""
    _replay_steps("mlp", 3)


def test_two_steps_replayed_with_the_philox_normals_over_several_passes():
    """The same at h = 90: step 1 samples around step 0's mean shifted ACROSS the pass boundary - the last step of the first pass
    (t = 84) takes the mean of t = 85 -, draws its second pass at element index ``t0 * A`` onwards and hands the rollout a
    candidate tensor stored in two passes; the update then refits a mean of 540 elements per env."""
    case = MODELS["long"]
    tc = 512 // 6
    assert case["h"] > tc
    mean = _replay_steps("long", 2)[0]
    assert mean.shape == (case["m"], case["h"] * 6)
    # the step-0 mean that step 1 shifted is not constant over the boundary: a clamp at the pass end would have shown
    assert np.all(np.abs(mean[:, (tc - 1) * 6:tc * 6] - mean[:, tc * 6:(tc + 1) * 6]).max(axis=1) > 0)


# ------------------------------------------------------------------------------------------------------------------------ reset
def test_reset_zeroes_only_the_marked_envs_start():
    case, ctrl = _controller("mlp")
    obs = _obs("mlp")
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    assert m == 3
    zs = [np.random.RandomState(20 + s).randn(n, m, D).astype(np.float32) for s in range(3)]
    _inject(ctrl, zs)
    ctrl.get_actions(obs)
    ctrl.get_actions(obs)
    mean = ctrl.last_plan["mppi_mean"]
    assert np.all(np.abs(mean).max(axis=1) > 0)
    ctrl.reset(dones=[False, True, False])
    ctrl.get_actions(obs)
    a_clip, _ = _samples(ctrl)
    sigma = ctrl._mppi_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    shift = np.array([1, -1, 1], dtype=np.int32)
    shifted, want_a, _ = mr.sample_f32(mean, shift, zs[2], sigma, ctrl.mppi_beta, low, high, n, m, h, ad)
    assert np.all(shifted[1] == 0) and np.any(shifted[0] != 0) and np.any(shifted[2] != 0)
    assert np.array_equal(_bits(a_clip), _bits(want_a))
    unmarked = mr.sample_f32(mean, np.ones(m, dtype=np.int32), zs[2], sigma, ctrl.mppi_beta, low, high, n, m, h, ad)[1]
    assert not np.array_equal(a_clip[:, 1], unmarked[:, 1])


# ---------------------------------------------------------------------------------------------------------------------- seeding
def test_same_seed_same_actions_other_seed_other_actions():
    obs = _obs("mlp")

    def three(seed):
        torch.manual_seed(seed)
        _, ctrl = _controller("mlp")
        return np.stack([ctrl.get_actions(obs)[0] for _ in range(3)])

    a, b, c = three(5), three(5), three(6)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])
    assert not np.array_equal(a[0], a[1])                   # the stream moves on from step to step


# ------------------------------------------------------------------------------------------------------------------- iterations
def test_second_iteration_samples_around_the_firsts_mean_unshifted():
    case, ctrl = _controller("mlp", mppi_iters=2)
    obs = _obs("mlp")
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    zs = [np.random.RandomState(40 + s).randn(n, m, D).astype(np.float32) for s in range(2)]
    _inject(ctrl, zs)
    log = []
    rollout = ctrl._rollout

    def spy(*args, **kw):
        out = rollout(*args, **kw)
        log.append((ctrl._bufs["mppi_a_clip"].cpu().numpy().copy(), out[1].cpu().numpy().copy()))
        return out

    ctrl._rollout = spy
    action, _ = ctrl.get_actions(obs)
    assert len(log) == 2 and ctrl._bufs["mppi_calls"] == 2
    sigma = ctrl._mppi_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    zero = np.zeros((m, D), dtype=np.float32)
    want_a0 = mr.sample_f32(zero, -np.ones(m, dtype=np.int32), zs[0], sigma, ctrl.mppi_beta, low, high, n, m, h, ad)[1]
    assert np.array_equal(_bits(log[0][0]), _bits(want_a0))
    mean1 = mr.update(zero, log[0][0], log[0][1], ctrl.mppi_kappa)[0]               # float64
    kept, want_a1, _ = mr.sample(mean1, np.zeros(m, dtype=np.int32), zs[1], sigma, ctrl.mppi_beta, low, high, n, m, h, ad)
    assert np.array_equal(kept, mean1)
    # the product's fp32 mean is within the update's bound of mean1; adding the filtered noise and clipping does not widen that,
    # and rounds a few more times (the Philox term of the sample bound is not needed: the normals are injected)
    mean_bound, _ = mr.update_bounds(n, ctrl.mppi_kappa, float(np.max(np.abs(log[0][0]))), mr.sum_chain(n))
    U = float(np.max(np.abs(zs[1].astype(np.float64) * np.tile(sigma.astype(np.float64), h))))
    bound = mean_bound + 4 * 2.0 ** -24 * (np.abs(mean1)[None] + U / float(np.float32(ctrl.mppi_beta)))
    r = float(np.max(np.abs(log[1][0].astype(np.float64) - want_a1) / bound))
    print("\n[mppi] second iteration: sample error / bound %.3f" % r)
    assert r <= 1.0
    moved = mr.sample(mean1, np.ones(m, dtype=np.int32), zs[1], sigma, ctrl.mppi_beta, low, high, n, m, h, ad)[1]
    assert np.max(np.abs(moved - want_a1)) > 100 * float(np.max(bound))            # (a shifted second iteration would show)
    assert np.array_equal(_bits(ctrl.last_plan["returns"]), _bits(log[1][1]))
    _check_update(ctrl, action, mean1.astype(np.float32), log[1][0], ctrl.mppi_kappa, "iteration 2")


# --------------------------------------------------------------------------------------------------------------- reward sources
def test_reward_program_routes_through_the_program_plan():
    from test_reward_program_gpu import _controller as program_controller
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, ctrl = program_controller(cid, rng="device", use_mppi=True)
    obs = cases.load_golden(cid)["obs0"]
    torch.manual_seed(seed)
    action, _ = ctrl.get_actions(obs)
    assert model.planner_model().program_plans == 1
    _, seq = _samples(ctrl)
    want = rollout_returns(cases.oracle_dynamics(case), env.reward, obs, seq.astype(np.float64), case["n"], case.get("discount", 1.0))
    assert rel_err(ctrl.last_plan["returns"], want.reshape(case["m"], case["n"])) < RTOL
    assert action.shape == (case["m"], 6) and np.isfinite(action).all()


def test_reward_model_routes_through_the_reward_model_plan():
    import reward_model_cases as rmc
    from test_reward_model_gpu import _controller as model_controller
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, rm, _, ctrl = model_controller(cid, rng="device", use_mppi=True)
    obs = cases.load_golden(cid)["obs0"]
    torch.manual_seed(seed)
    action, _ = ctrl.get_actions(obs)
    native = model.planner_model()
    assert native.reward_model_plans == 1 and native.program_plans == 0
    _, seq = _samples(ctrl)
    want = rollout_returns(cases.oracle_dynamics(case), rmc.model_reward_fn(rm), obs, seq.astype(np.float64), case["n"],
                           case.get("discount", 1.0))
    assert rel_err(ctrl.last_plan["returns"], want.reshape(case["m"], case["n"])) < RTOL
    assert action.shape == (case["m"], 6) and np.isfinite(action).all()


# -------------------------------------------------------------------------------------------------------------------- recurrent
def test_recurrent_single_step_and_state_advance():
    cid = "hc_rnn_rs_m2_n64_h4_reset_s0"
    case, _ = cases.split_id(cid)
    case = dict(case)
    ctrl = cases.product_rnn_controller(case, rng="device", use_mppi=True)
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    rs = np.random.RandomState(5)
    hid = LSTMStateTuple(rs.randn(m, case["units"]).astype(np.float32), np.tanh(rs.randn(m, case["units"])).astype(np.float32))
    ctrl._hidden_state = hid
    obs = cases.load_golden(cid)["obs"][0]
    z = np.random.RandomState(6).randn(n, m, D).astype(np.float32)
    _inject(ctrl, [z])
    action, _ = ctrl.get_actions(obs)
    a_clip, seq = _samples(ctrl)
    sigma = ctrl._mppi_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    zero = np.zeros((m, D), dtype=np.float32)
    want_a = mr.sample_f32(zero, -np.ones(m, dtype=np.int32), z, sigma, ctrl.mppi_beta, low, high, n, m, h, ad)[1]
    assert np.array_equal(_bits(a_clip), _bits(want_a))
    env, _, _ = cases.rnn_recipe(case)
    want = rnn_rollout_returns(cases.oracle_rnn_dynamics(case), make_reward(case["env"], env.dt), obs, hid, seq.astype(np.float64), n,
                               case.get("discount", 1.0)).reshape(m, n)
    err = rel_err(ctrl.last_plan["returns"], want)
    print("\n[mppi] recurrent: returns against the float64 oracle %.2e" % err)
    assert err < RTOL
    _check_update(ctrl, action, zero, a_clip, ctrl.mppi_kappa, "recurrent")
    # the controller's own state: the advance kernel's result for the returned action
    native = ctrl.dynamics_model.planner_model()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(native.device)  # noqa: E731
    c1, h1 = native.advance(dev(obs), dev(action), dev(hid.c), dev(hid.h))
    assert np.array_equal(_bits(ctrl._hidden_state.c), _bits(c1.cpu().numpy()))
    assert np.array_equal(_bits(ctrl._hidden_state.h), _bits(h1.cpu().numpy()))


# ----------------------------------------------------------------------------------------------------------------- out of scope
def test_out_of_scope_combinations_raise():
    case, ctrl = _controller("mlp", native_cem_step=True)
    with pytest.raises(_lib.L2AError, match="one C controller call"):
        ctrl.get_actions(_obs("mlp"))
    case, ctrl = _controller("mlp")
    ctrl.rng = "numpy"
    with pytest.raises(_lib.L2AError, match="NumPy normals"):
        ctrl.get_actions(_obs("mlp"))
    case, ctrl = _controller("mlp")
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl.get_actions(_obs("mlp"))
