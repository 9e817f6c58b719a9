"""Policy priors without a GPU: the host-only check and geometry function of the policy kernel, the argument checks of the entries
that need no device, ``MLPPolicyModel`` (cloning fit, predict, pickling), the references the GPU tests lean on
(``tests/policy_reference.py``) and the controller's constructor errors and routing decisions."""

import ctypes
import pickle

import numpy as np
import pytest
import torch

import cases
import policy_reference as pr
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPPolicyModel
from learning_to_adapt_amd.envs import SyntheticEnv
from learning_to_adapt_amd.policies import MPCController, RNNMPCController

SYMBOLS = ("l2a_policy_model_check", "l2a_policy_model_geometry", "l2a_policy_model_create", "l2a_policy_model_destroy",
           "l2a_policy_model_set_weights", "l2a_policy_model_set_norm", "l2a_policy_act", "l2a_policy_propose")


def _hid(hidden):
    return (ctypes.c_int * max(len(hidden), 1))(*hidden)


# ------------------------------------------------------------------------------------------
# 1. l2a_policy_model_check and the entries' checks that need no GPU
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs,act,hidden,code,word", [
    (20, 0, (64,), 1, "act_dim 0"),
    (20, 17, (64,), 1, "act_dim 17"),
    (20, 6, (96,), 1, "width 96"),
    (20, 6, (64, 64, 64, 64), 1, "4 hidden layers"),
    (20, 6, (64,), 5, "activation 5"),
    (20, 6, (64,), -1, "activation -1"),
    (0, 6, (64,), 1, "obs_dim 0"),
    (65, 6, (64,), 1, "obs_dim 65"),
    (20, 6, (), 1, "0 hidden layers"),
    (20, 6, (576,), 1, "width 576"),
])
def test_check_rejects(obs, act, hidden, code, word):
    lib = _lib.load()
    assert lib.l2a_policy_model_check(obs, act, len(hidden), _hid(hidden), code) == _lib.L2A_EINVAL
    assert word in lib.l2a_last_error(None).decode()
    assert word in _lib.policy_model_check(obs, act, hidden, code)


@pytest.mark.parametrize("obs,act,hidden,code", [(1, 1, (64,), 0), (64, 16, (512, 512, 512), 4), (17, 6, (64, 128), 2),
                                                 (20, 6, (256, 256), "relu"), (41, 9, (512, 64, 128), "tanh")])
def test_check_accepts(obs, act, hidden, code):
    assert _lib.policy_model_check(obs, act, hidden, code) is None


def test_new_symbols_are_exported_and_refuse_null_handles():
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    null = ctypes.c_void_p()
    assert lib.l2a_policy_model_check(20, 6, 1, None, 1) == _lib.L2A_EINVAL
    assert "null hidden sizes" in lib.l2a_last_error(None).decode()
    assert lib.l2a_policy_act(null, null, 1, null, 0, 0, null, null, null, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_policy_propose(null, null, null, 1, 1, 1, 1, 0, null, 0, 0, null, null, null, null, null, 1, null) == _lib.L2A_EINVAL
    assert lib.l2a_policy_model_set_weights(null, None, null) == _lib.L2A_EINVAL
    assert lib.l2a_policy_model_set_norm(null, None, None, None, None, null) == _lib.L2A_EINVAL
    out = ctypes.c_void_p()
    assert lib.l2a_policy_model_create(null, 20, 6, 1, _hid((64,)), 1, ctypes.byref(out)) == _lib.L2A_EINVAL and not out.value
    lib.l2a_policy_model_destroy(null)         # a no-op


# ------------------------------------------------------------------------------------------
# 2. the geometry function against the documented rule
# ------------------------------------------------------------------------------------------
#                 hidden,         rows, cus,  RT, workgroups
GEOMETRY_TABLE = [((256, 256),       1, 256,   1,    1),
                  ((256, 256),    4096, 256,   1,  256),      # exactly one row tile per CU ...
                  ((256, 256),    4097, 256,   2,  129),      # ... and one row more
                  ((256, 256),    8192, 256,   2,  256),
                  ((256, 256),    8193, 256,   4,  129),
                  ((256, 256),   16385, 256,   8,  129),
                  ((512,),       16385, 256,   4,  257),      # width 512: 8 accumulator tiles per wave, RT <= 4
                  ((64,),           64,   4,   1,    4),
                  ((64,),           65,   4,   2,    3),
                  ((512, 64, 128), 500,   4,   4,    8)]


@pytest.mark.parametrize("hidden,rows,cus,rt,wgs", GEOMETRY_TABLE)
def test_every_table_row_takes_its_geometry(hidden, rows, cus, rt, wgs):
    g = _lib.policy_model_geometry(20, 6, hidden, rows, cus=cus)
    assert g == dict(RT=rt, workgroups=wgs, lds_bytes=rt * max(2, max(hidden) // 16) * 1024)
    assert g == pr.geometry_rule(20, hidden, rows, cus, 160 * 1024)


@pytest.mark.parametrize("hidden", [(64,), (256, 256), (512, 512, 512), (320, 64)])
def test_geometry_is_the_documented_rule_over_a_sweep(hidden):
    seen = set()
    for lds in (160 * 1024, 64 * 1024, 40 * 1024):
        for cus in (1, 8, 256, 0):
            for rows in (1, 15, 16, 17, 16 * 8, 16 * 8 + 1, 2000, 4096, 4097, 70000, (1 << 30) - 1):
                want = pr.geometry_rule(64, hidden, rows, cus, lds)
                if want is None:
                    with pytest.raises(_lib.L2AError, match="no launch geometry fits"):
                        _lib.policy_model_geometry(64, 16, hidden, rows, cus=cus, lds_per_block=lds)
                    continue
                assert _lib.policy_model_geometry(64, 16, hidden, rows, cus=cus, lds_per_block=lds) == want
                seen.add(want["RT"])
    assert len(seen) >= 2


def test_geometry_refusals():
    lib = _lib.load()
    out = (ctypes.c_int * 8)()
    assert lib.l2a_policy_model_geometry(20, 6, 1, _hid((512,)), 100, 4, 16 * 1024, out) == _lib.L2A_EINVAL      # no RT fits this LDS
    assert "no launch geometry fits" in lib.l2a_last_error(None).decode()
    assert pr.geometry_rule(20, (512,), 100, 4, 16 * 1024) is None
    assert lib.l2a_policy_model_geometry(20, 6, 1, _hid((64,)), 0, 4, 160 * 1024, out) == _lib.L2A_EINVAL
    assert lib.l2a_policy_model_geometry(20, 6, 1, _hid((64,)), 100, 4, 160 * 1024, None) == _lib.L2A_EINVAL
    assert lib.l2a_policy_model_geometry(20, 17, 1, _hid((64,)), 100, 4, 160 * 1024, out) == _lib.L2A_EINVAL
    with pytest.raises(_lib.L2AError, match="width 96"):
        _lib.policy_model_geometry(20, 6, (96,), 100)


@pytest.mark.parametrize("hidden", [(64,), (256, 64), (512, 512, 512)])
@pytest.mark.parametrize("obs", [1, 17, 64])
def test_value_and_policy_kernels_share_one_geometry_rule(hidden, obs):
    """``l2a_value_model_geometry`` and ``l2a_policy_model_geometry`` go through one ``choose_rt``: the same network and row count
    give the same (RT, workgroups, LDS bytes), whatever the policy's ``act_dim``."""
    for rows in (1, 16, 17, 16 * 256, 16 * 256 * 8 + 1):
        for cus in (256, 1):
            for lds in (65536, 163840):
                v = _lib.value_model_geometry(obs, hidden, rows, cus=cus, lds_per_block=lds)
                p = _lib.policy_model_geometry(obs, 6, hidden, rows, cus=cus, lds_per_block=lds)
                assert v == p and set(v) == {"RT", "workgroups", "lds_bytes"}, (rows, cus, lds, v, p)
                assert v["workgroups"] == (rows + 16 * v["RT"] - 1) // (16 * v["RT"])


@pytest.mark.parametrize("hidden,code,word", [
    ((0,), 1, "hidden width 0 "), ((32,), 1, "hidden width 32 "), ((96,), 1, "hidden width 96 "), ((576,), 1, "hidden width 576 "),
    ((64, 96), 1, "hidden width 96 "), ((), 1, "0 hidden layers"), ((64, 64, 64, 64), 1, "4 hidden layers"),
    ((64,), -1, "unknown activation -1"), ((64,), 5, "unknown activation 5"), ((64,), 100, "unknown activation 100")])
def test_the_three_model_checks_reject_the_same_networks_with_the_same_words(hidden, code, word):
    """The reward, value and policy model checks are one function behind three prefixes."""
    msgs = {"reward model: ": _lib.reward_model_check(20, 6, hidden, code),
            "value model: ": _lib.value_model_check(20, hidden, code),
            "policy model: ": _lib.policy_model_check(20, 6, hidden, code)}
    tails = set()
    for prefix, msg in msgs.items():
        assert msg is not None and msg.startswith(prefix), (prefix, msg)
        tails.add(msg[len(prefix):])
    assert len(tails) == 1 and tails.pop().startswith(word), msgs


# ------------------------------------------------------------------------------------------
# 3. MLPPolicyModel
# ------------------------------------------------------------------------------------------
def _policy(env, hidden=(64, 64), act="relu", base=None, params=None):
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    pm = MLPPolicyModel(name="pol", env=env, hidden_sizes=hidden, hidden_nonlinearity=act, init_seed=0)
    pm.set_params(params if params is not None else pr.policy_weights(od, ad, hidden))
    pm.set_normalization(pr.policy_norm(od, ad, base=base))
    return pm


def test_fit_lowers_the_cloning_loss_on_a_linear_target():
    env = SyntheticEnv("half_cheetah")
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    rs = np.random.RandomState(3)
    mix = 0.3 * rs.randn(od, ad)
    obs, obs_t = rs.randn(1500, od), rs.randn(300, od)
    act, act_t = obs @ mix + 0.1, obs_t @ mix + 0.1
    model = MLPPolicyModel(name="pol", env=env, hidden_sizes=(64,), init_seed=1, batch_size=250)
    np.random.seed(0)
    torch.manual_seed(0)
    model.fit(obs, act, epochs=0)                            # statistics only
    assert set(model.normalization) == {"obs", "act"} and model.normalization["act"][0].shape == (ad,)
    before = float(np.mean((model.predict(obs_t) - act_t) ** 2))
    stats = model.fit(obs, act, epochs=20, compute_normalization=False)
    after = float(np.mean((model.predict(obs_t) - act_t) ** 2))
    print("held-out cloning MSE: %.4f before, %.4f after the fit (action variance %.4f)" % (before, after, np.var(act_t)))
    assert after < 0.5 * before and after < np.var(act_t)
    assert np.isfinite(stats["TrainLoss"]) and np.isfinite(stats["ValidLoss"])


@pytest.mark.parametrize("hidden,act", [((64,), "relu"), ((64, 128), "tanh"), ((128, 64, 64), "swish")])
def test_predict_is_the_reference_helper(hidden, act):
    env = SyntheticEnv("half_cheetah")
    model = _policy(env, hidden, act)
    obs = pr.states(5, 40, 20, model.normalization).astype(np.float64)
    want = pr.restate64([p.numpy() for p in model._params], model.normalization, act, obs)
    got = model.predict(obs)
    assert got.dtype == np.float64 and got.shape == (40, 6)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    plain = MLPPolicyModel(name="pol", env=env, hidden_sizes=hidden, hidden_nonlinearity=act, normalize_input=False, init_seed=0)
    np.testing.assert_allclose(plain.predict(obs), pr.restate64([p.numpy() for p in plain._params], None, act, obs), rtol=1e-12, atol=1e-12)


def test_model_pickles_with_its_weights_and_statistics():
    env = SyntheticEnv("half_cheetah")
    model = _policy(env, (64,), "tanh")
    twin = pickle.loads(pickle.dumps(model))
    assert twin.hidden_sizes == (64,) and twin.hidden_nonlinearity == "tanh" and twin._native is None
    for a, b in zip(model.get_param_values().items(), twin.get_param_values().items()):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for key in ("obs", "act"):
        assert np.array_equal(model.normalization[key][0], twin.normalization[key][0])
        assert np.array_equal(model.normalization[key][1], twin.normalization[key][1])
    assert list(model.get_param_values()) == ["hidden_0/kernel", "hidden_0/bias", "output/kernel", "output/bias"]
    assert model.get_param_values()["output/kernel"].shape == (64, 6)
    obs = pr.states(6, 9, 20, model.normalization).astype(np.float64)
    assert np.array_equal(model.predict(obs), twin.predict(obs))
    assert model.native_eligible() is None
    assert "width 96" in MLPPolicyModel(name="pol", env=env, hidden_sizes=(96,)).native_eligible()
    with pytest.raises(ValueError):
        MLPPolicyModel(name="pol", env=env, hidden_nonlinearity="gelu")


# ------------------------------------------------------------------------------------------
# 4. the references
# ------------------------------------------------------------------------------------------
def test_k_order_is_a_permutation_in_the_mfma_order():
    assert pr.k_order(16) == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]
    assert pr.k_order(6) == [0, 4, 1, 5, 2, 3]
    for k_in in (1, 17, 20, 41, 64, 512):
        order = pr.k_order(k_in)
        assert sorted(order) == list(range(k_in))
        assert [k // 16 for k in order] == sorted(k // 16 for k in order)        # k-groups ascending


def test_the_fp32_restatement_stays_close_to_the_float64_oracle_and_rounds_per_operation():
    od, ad, hidden = 17, 6, (64, 64)
    params, norm = pr.policy_weights(od, ad, hidden), pr.policy_norm(od, ad)
    obs = pr.states(7, 33, od, norm)
    rs = np.random.RandomState(1)
    z = rs.randn(33, ad).astype(np.float32)
    sigma = np.array([0.1, 0.0, 0.2, 0.0, 0.05, 0.3], dtype=np.float32)
    low, high = np.full(ad, -0.4, np.float32), np.full(ad, 0.4, np.float32)
    got = pr.act_f32(params, norm, "relu", obs, sigma, low, high, z)
    want = pr.act64(params, norm, "relu", obs, sigma, low, high, z)
    assert got.dtype == np.float32 and np.max(np.abs(got - want)) < 1e-5
    assert np.any(got == low) and np.any(got == high) and np.any((got > low) & (got < high))
    # sigma == 0: z is not looked at, even where it is NaN
    z_nan = z.copy()
    z_nan[:, sigma == 0] = np.nan
    assert np.array_equal(pr.act_f32(params, norm, "relu", obs, sigma, low, high, z_nan).view(np.uint32), got.view(np.uint32))
    assert np.array_equal(pr.act_f32(params, norm, "relu", obs, 0 * sigma, low, high, None).view(np.uint32),
                          pr.act_f32(params, norm, "relu", obs, 0 * sigma, low, high, np.full_like(z, np.nan)).view(np.uint32))
    # a non-finite state: that row is NaN, the others keep their bits
    bad = obs.copy()
    bad[3, od - 1] = np.inf
    bad[7, 0] = np.nan
    got_bad = pr.act_f32(params, norm, "relu", bad, sigma, low, high, z)
    assert np.isnan(got_bad[[3, 7]]).all()
    keep = np.delete(np.arange(33), [3, 7])
    assert np.array_equal(got_bad[keep].view(np.uint32), got[keep].view(np.uint32))
    assert np.isnan(pr.act64(params, norm, "relu", bad, sigma, low, high, z)[[3, 7]]).all()
    # one fma per chain step: a layer of one input is bias + fl(w x), and k_order is what separates it from a plain dot product
    x = rs.randn(5, 40).astype(np.float32)
    w = rs.randn(40, 3).astype(np.float32)
    b = rs.randn(3).astype(np.float32)
    chain = np.zeros((5, 3), dtype=np.float32)
    for k in pr.k_order(40):
        chain = pr.fma32(x[:, k:k + 1], w[k:k + 1], chain)
    assert np.array_equal(pr.layer_f32(x, w, b), chain + b)


@pytest.mark.parametrize("mode,m", [("mean", 2), ("per_block", 3)])
def test_the_oracle_against_a_closed_form(mode, m):
    """All-zero kernels and bias b: a = clip(mu_a + sd_a b) at every step, whatever the dynamics do in between."""
    case = dict(env="half_cheetah", mode=mode, hidden=[32, 32], E=2 if mode == "mean" else m)
    env, _, norms = cases.recipe(case)
    dyn = cases.oracle_dynamics(case, mlp_dtype=np.float64)
    od, ad = 20, 6
    norm = pr.policy_norm(od, ad, base=norms[0])
    b = np.linspace(-3.0, 3.0, ad)
    params = pr.constant_weights(od, ad, (64,), b)
    low, high = np.full(ad, -1.0), np.full(ad, 1.0)
    obs0 = pr.states(2, m, od, norm).astype(np.float64)
    acts, sts = pr.propose64(dyn, params, norm, "relu", obs0, 4, 3, np.zeros(ad), low, high)
    raw = norm["act"][0] + (norm["act"][1] + 1e-10) * b.astype(np.float32)
    want = np.clip(raw, low, high)
    assert acts.shape == (3, m * 4, ad) and sts.shape == (3, m * 4, od)
    np.testing.assert_allclose(acts, np.broadcast_to(want, acts.shape), rtol=1e-12, atol=1e-12)
    assert np.any(want == 1.0) or np.any(want == -1.0)
    # the states are the oracle's own rollout of those actions
    from oracle.planner import rollout_trace
    _, trace = rollout_trace(dyn, lambda s, a, n: np.zeros(len(s)), obs0, acts, 4, 1.0)
    assert np.array_equal(trace, sts)
    # with noise, element (t, i, j, k) reads z[t, i, j, k]
    z = np.random.RandomState(4).randn(3, m, 4, ad)
    sig = np.full(ad, 0.01)
    noisy, _ = pr.propose64(dyn, params, norm, "relu", obs0, 4, 3, sig, low, high, z)
    np.testing.assert_allclose(noisy, np.clip(raw + sig * z.reshape(3, m * 4, ad), low, high), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------
# 5. the controller: constructor errors and routing decisions
# ------------------------------------------------------------------------------------------
def _kw():
    case = cases.CASES["hc_rs_m3_n64_h5"]
    env, model = cases.product_model(case)
    return env, model, dict(name="policy", env=env, dynamics_model=model, n_candidates=case["n"], horizon=case["h"])


def test_constructor_errors():
    env, model, kw = _kw()
    pm = _policy(env)
    with pytest.raises(_lib.L2AError, match="rng='device'.*host copy of the candidates"):
        MPCController(policy_model=pm, **kw)
    with pytest.raises(_lib.L2AError, match="use_icem is not built: the kept elites and the added mean own candidate slots"):
        MPCController(policy_model=pm, rng="device", use_icem=True, **kw)
    with pytest.raises(_lib.L2AError, match="needs cem_mode='fixed'"):
        MPCController(policy_model=pm, rng="device", use_cem=True, cem_mode="reference", **kw)
    for key in ("native_cem_step", "native_mppi_step", "native_icem_step"):
        with pytest.raises(_lib.L2AError, match="plans through the Python loop: the C controller steps"):
            MPCController(policy_model=pm, rng="device", use_cem=(key == "native_cem_step"), cem_mode="fixed",
                          use_mppi=(key == "native_mppi_step"), **dict(kw, **{key: True}))
    with pytest.raises(_lib.L2AError, match="not eligible.*no host fallback.*width 96"):
        MPCController(policy_model=_policy(env, hidden=(96,)), rng="device", **kw)

    class Plain(object):
        def predict(self, obs):
            return np.zeros((len(obs), 6))

    with pytest.raises(_lib.L2AError, match="no host fallback"):
        MPCController(policy_model=Plain(), rng="device", **kw)
    with pytest.raises(_lib.L2AError, match="policy_candidates 65 exceeds n_candidates 64"):
        MPCController(policy_model=pm, rng="device", policy_candidates=65, **kw)
    with pytest.raises(ValueError, match="policy_candidates must be at least 1"):
        MPCController(policy_model=pm, rng="device", policy_candidates=0, **kw)
    with pytest.raises(ValueError, match="policy_noise"):
        MPCController(policy_model=pm, rng="device", policy_noise=-0.1, **kw)
    with pytest.raises(ValueError, match="policy_noise"):
        MPCController(policy_model=pm, rng="device", policy_noise=[0.1, 0.2], **kw)

    class Custom(SyntheticEnv):         # a reward the library does not know, and no reward model: not a fusable plan
        def reward(self, obs, act, nxt):
            return np.zeros(len(obs))

    custom = Custom("half_cheetah")
    custom.reward_spec = None
    with pytest.raises(_lib.L2AError, match="needs a plan the library scores"):
        MPCController(name="policy", env=custom, dynamics_model=model, policy_model=pm, rng="device")
    # the recurrent controller does not take the keyword
    rnn_case = cases.CASES[cases.rnn_case_ids()[0].rsplit("_s", 1)[0]]
    renv, rnn_model = cases.product_rnn_model(rnn_case)
    with pytest.raises(TypeError):
        RNNMPCController(name="policy", env=renv, dynamics_model=rnn_model, policy_model=pm)


def test_n_pi_from_the_fraction_and_the_noise_vector():
    env, model, kw = _kw()
    pm = _policy(env)
    assert MPCController(policy_model=pm, rng="device", **kw)._n_pi == 3                      # round(0.05 * 64)
    assert MPCController(policy_model=pm, rng="device", policy_fraction=0.001, **kw)._n_pi == 1
    assert MPCController(policy_model=pm, rng="device", policy_fraction=0.5, **kw)._n_pi == 32
    assert MPCController(policy_model=pm, rng="device", policy_fraction=1.0, **kw)._n_pi == 64
    assert MPCController(policy_model=pm, rng="device", policy_candidates=24, policy_fraction=0.5, **kw)._n_pi == 24
    ctrl = MPCController(policy_model=pm, rng="device", policy_noise=0.25, **kw)
    assert ctrl._policy_sigma.dtype == np.float32 and np.array_equal(ctrl._policy_sigma, np.full(6, 0.25, np.float32))
    per_dim = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
    assert np.array_equal(MPCController(policy_model=pm, rng="device", policy_noise=per_dim, **kw)._policy_sigma,
                          np.asarray(per_dim, np.float32))
    assert np.array_equal(MPCController(policy_model=pm, rng="device", **kw)._policy_sigma, np.zeros(6, np.float32))


class _Chunked(object):
    """Stands in for a native model that offers the horizon-chunked entry."""
    def plan_rs_chunk(self, *a, **k):
        raise AssertionError("not called")


def test_the_l2a_reward_paths_decline_with_a_policy_and_are_unchanged_without_one():
    env, model, kw = _kw()
    kw = dict(kw, horizon=10)           # (long enough for both pipelines to apply)
    model.planner_model = lambda: _Chunked()
    plain = MPCController(**kw)
    assert plain.policy_model is None and not plain._program()
    assert plain._can_pipeline(10, 64) and plain._can_pipeline_cem(1, 1, 64)
    assert "policy_model" in plain.__dict__ and not hasattr(plain, "_n_pi")
    for planner in (dict(), dict(use_cem=True, cem_mode="fixed"), dict(use_mppi=True)):
        ctrl = MPCController(policy_model=_policy(env), rng="device", **dict(kw, **planner))
        assert ctrl._program() and ctrl._fusable()
        assert not ctrl._can_pipeline(10, 64) and not ctrl._can_pipeline_cem(1, 1, 64)
        assert ctrl._native_rs_step(np.zeros((3, 20)), 3) is None


def test_policy_fill_refuses_more_than_one_rank():
    env, model, kw = _kw()
    ctrl = MPCController(policy_model=_policy(env), rng="device", **kw)
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="not sharded at the controller level"):
        ctrl._policy_fill(torch.zeros((3, 20)), None, None, 32, 0)
