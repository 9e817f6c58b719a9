"""Terminal values without a GPU: the host-only check and geometry function of the value kernel, the argument checks of the
entries that need no device, ``MLPValueModel`` (targets, fit, pickling), the float64 restatement the GPU tests lean on, the
controller's constructor errors and its routing with the native calls stubbed by the oracle."""

import ctypes
import pickle

import numpy as np
import pytest
import torch

import cases
import oracle_backend
import value_model_cases as vmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPValueModel
from learning_to_adapt_amd.envs import SyntheticEnv
from learning_to_adapt_amd.policies import MPCController, RNNMPCController

RTOL = 1e-4         # the bar of tests/test_gpu_parity.py


def _hid(hidden):
    return (ctypes.c_int * max(len(hidden), 1))(*hidden)


# ------------------------------------------------------------------------------------------
# 1. l2a_value_model_check and the entries' checks that need no GPU
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs,hidden,code,word", [
    (0, (64,), 1, "obs_dim 0"),
    (65, (64,), 1, "obs_dim 65"),
    (20, (), 1, "0 hidden layers"),
    (20, (64, 64, 64, 64), 1, "4 hidden layers"),
    (20, (32,), 1, "width 32"),
    (20, (96,), 1, "width 96"),
    (20, (576,), 1, "width 576"),
    (20, (64, 100), 1, "width 100"),
    (20, (64,), -1, "activation -1"),
    (20, (64,), 5, "activation 5"),
])
def test_check_rejects(obs, hidden, code, word):
    lib = _lib.load()
    assert lib.l2a_value_model_check(obs, len(hidden), _hid(hidden), code) == _lib.L2A_EINVAL
    assert word in lib.l2a_last_error(None).decode()
    assert word in _lib.value_model_check(obs, hidden, code)


@pytest.mark.parametrize("obs,hidden,code", [(1, (64,), 0), (64, (512, 512, 512), 4), (17, (64, 128), 2), (20, (256, 256), "relu")])
def test_check_accepts(obs, hidden, code):
    assert _lib.value_model_check(obs, hidden, code) is None


def test_check_refuses_null_hidden_sizes():
    lib = _lib.load()
    assert lib.l2a_value_model_check(20, 1, None, 1) == _lib.L2A_EINVAL
    assert "null hidden sizes" in lib.l2a_last_error(None).decode()


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("l2a_value_model_check", "l2a_value_model_geometry", "l2a_value_model_create", "l2a_value_model_destroy",
                 "l2a_value_model_set_weights", "l2a_value_model_set_norm", "l2a_value_model_predict", "l2a_value_terminal",
                 "l2a_plan_rs_value", "l2a_plan_rs_program_value", "l2a_plan_rs_reward_model_value"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS


def test_entries_refuse_null_handles_without_a_device():
    """What can be refused before any handle is looked at: every entry returns L2A_EINVAL for a NULL model or value model."""
    lib = _lib.load()
    null = ctypes.c_void_p()
    assert lib.l2a_value_terminal(null, null, null, 1, 1, 1, 1.0, 1.0, 0, null, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_value_model_predict(null, null, 1, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_value_model_set_weights(null, None, null) == _lib.L2A_EINVAL
    assert lib.l2a_value_model_set_norm(null, None, None, None, None, null) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_value(null, null, null, null, 1, 1, 1, 1.0, None, 1.0, 0, null, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_program_value(null, null, null, null, 1, 1, 1, 1.0, None, 1.0, 0, null, null, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_reward_model_value(null, null, null, null, null, 1, 1, 1, 1.0, 1.0, 0, null, null, null, null) == _lib.L2A_EINVAL
    out = ctypes.c_void_p()
    assert lib.l2a_value_model_create(null, 20, 1, _hid((64,)), 1, ctypes.byref(out)) == _lib.L2A_EINVAL and not out.value
    lib.l2a_value_model_destroy(null)          # a no-op


# ------------------------------------------------------------------------------------------
# 2. the geometry function
# ------------------------------------------------------------------------------------------
#                 hidden,         rows, cus,  RT, workgroups
GEOMETRY_TABLE = [((256, 256),       1, 256,   1,    1),
                  ((256, 256),    2000, 256,   1,  125),      # config 2: m n = 2000 rows, latency-sized
                  ((256, 256),    4096, 256,   1,  256),      # exactly one row tile per CU
                  ((256, 256),    4097, 256,   2,  129),
                  ((256, 256),    8193, 256,   4,  129),
                  ((256, 256),   16385, 256,   8,  129),
                  ((256, 256),  100000, 256,   8,  782),      # the cap: more than one round
                  ((512,),       16385, 256,   4,  257),      # width 512: 8 accumulator tiles per wave, RT <= 4
                  ((512, 64),     8193, 256,   4,  129),
                  ((320,),       16385, 256,   4,  257),      # TPW = 5: 8 x 5 > 32
                  ((64,),           33,   4,   1,    3),
                  ((64,),           65,   4,   2,    3),
                  ((64,),          500,   4,   8,    4),
                  ((128, 64),      210,   8,   2,    7)]


@pytest.mark.parametrize("hidden,rows,cus,rt,wgs", GEOMETRY_TABLE)
def test_every_table_row_takes_its_geometry(hidden, rows, cus, rt, wgs):
    g = _lib.value_model_geometry(20, hidden, rows, cus=cus)
    kgs = max(2, max(hidden) // 16)
    assert g == dict(RT=rt, workgroups=wgs, lds_bytes=rt * kgs * 1024)


def test_the_table_reaches_every_rt():
    assert {row[3] for row in GEOMETRY_TABLE} == {1, 2, 4, 8}


@pytest.mark.parametrize("hidden", [(64,), (256, 256), (512, 512, 512), (320, 64)])
def test_geometry_properties_over_a_sweep(hidden):
    tpw = max(hidden) // 64
    for cus in (1, 8, 256, 0):
        for rows in (1, 15, 16, 17, 255, 2000, 4097, 70000, (1 << 30) - 1):
            g = _lib.value_model_geometry(64, hidden, rows, cus=cus)
            rt, tiles = g["RT"], (rows + 15) // 16
            assert rt in (1, 2, 4, 8) and rt * tpw <= 32 and g["lds_bytes"] + 4096 <= 160 * 1024
            assert g["workgroups"] == (rows + 16 * rt - 1) // (16 * rt)
            if rt > 1:                       # a smaller RT would have left more workgroups than CUs
                assert (tiles + rt // 2 - 1) // (rt // 2) > (cus or 256)
            if g["workgroups"] > (cus or 256):      # only the budgets stop RT from growing
                assert rt == 8 or 2 * rt * tpw > 32 or 2 * g["lds_bytes"] + 4096 > 160 * 1024


def test_geometry_with_a_small_lds_and_its_refusals():
    lib = _lib.load()
    assert _lib.value_model_geometry(20, (512,), 100000, cus=4, lds_per_block=64 * 1024)["RT"] == 1
    out = (ctypes.c_int * 8)()
    assert lib.l2a_value_model_geometry(20, 1, _hid((512,)), 100, 4, 16 * 1024, out) == _lib.L2A_EINVAL
    assert "no launch geometry fits" in lib.l2a_last_error(None).decode()
    assert lib.l2a_value_model_geometry(20, 1, _hid((64,)), 0, 4, 160 * 1024, out) == _lib.L2A_EINVAL
    assert lib.l2a_value_model_geometry(20, 1, _hid((64,)), 100, 4, 160 * 1024, None) == _lib.L2A_EINVAL
    assert lib.l2a_value_model_geometry(20, 1, _hid((96,)), 100, 4, 160 * 1024, out) == _lib.L2A_EINVAL
    with pytest.raises(_lib.L2AError, match="width 96"):
        _lib.value_model_geometry(20, (96,), 100)


# ------------------------------------------------------------------------------------------
# 3. MLPValueModel
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discount", [1.0, 0.9, 0.0])
def test_returns_to_go_against_the_brute_force_sum(discount):
    rs = np.random.RandomState(5)
    rewards = rs.randn(23)
    got = MLPValueModel.returns_to_go(rewards, discount)
    want = np.array([sum(discount ** (k - t) * rewards[k] for k in range(t, 23)) for t in range(23)])
    assert got.dtype == np.float64 and got.shape == (23,)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert MLPValueModel.returns_to_go([], discount).shape == (0,)


def _quadratic_data(seed, rows):
    env = SyntheticEnv("half_cheetah")
    od = env.observation_space.shape[0]
    rs = np.random.RandomState(seed)
    obs = rs.randn(rows, od)
    return env, obs, 3.0 - np.sum(obs[:, :4] ** 2, axis=1) + 0.5 * obs[:, 5]


def test_fit_lowers_the_loss_on_a_synthetic_quadratic_value():
    env, obs, val = _quadratic_data(0, 3000)
    _, obs_t, val_t = _quadratic_data(1, 1000)
    model = MLPValueModel(name="val", env=env, hidden_sizes=(64, 64), batch_size=250, learning_rate=0.003, init_seed=0)
    np.random.seed(0)
    torch.manual_seed(0)
    model.fit(obs, val, epochs=0)                           # statistics only
    assert set(model.normalization) == {"obs", "value"}
    assert model.normalization["value"] == (float(np.mean(val)), float(np.std(val)))
    before = float(np.mean((vmc.model_value_fn(model)(obs_t) - val_t) ** 2))
    stats = model.fit(obs, val, epochs=15, compute_normalization=False)
    after = float(np.mean((vmc.model_value_fn(model)(obs_t) - val_t) ** 2))
    print("held-out MSE of the value: %.4f before, %.4f after the fit (value variance %.4f)" % (before, after, np.var(val_t)))
    assert after < before and after < np.var(val_t)
    assert np.isfinite(stats["TrainLoss"]) and np.isfinite(stats["ValidLoss"])


def test_model_pickles_with_its_weights_and_statistics():
    env = SyntheticEnv("half_cheetah")
    model = MLPValueModel(name="val", env=env, hidden_sizes=(64,), hidden_nonlinearity="tanh", init_seed=3)
    model.set_params(vmc.value_weights(20, (64,)))
    model.set_normalization(vmc.value_norm(20))
    twin = pickle.loads(pickle.dumps(model))
    assert twin.hidden_sizes == (64,) and twin.hidden_nonlinearity == "tanh" and twin._native is None
    for a, b in zip(model.get_param_values().items(), twin.get_param_values().items()):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(model.normalization["obs"][0], twin.normalization["obs"][0])
    assert np.array_equal(model.normalization["obs"][1], twin.normalization["obs"][1])
    assert model.normalization["value"] == twin.normalization["value"]
    assert list(model.get_param_values()) == ["hidden_0/kernel", "hidden_0/bias", "output/kernel", "output/bias"]
    assert model.get_param_values()["hidden_0/kernel"].shape == (20, 64)
    assert model.native_eligible() is None
    assert "width 96" in MLPValueModel(name="val", env=env, hidden_sizes=(96,)).native_eligible()
    with pytest.raises(ValueError):
        MLPValueModel(name="val", env=env, hidden_nonlinearity="gelu")


# ------------------------------------------------------------------------------------------
# 4. the float64 restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("od,hidden,act_name", [(20, (64,), "relu"), (17, (64, 64), "tanh"), (41, (128, 64), "swish"),
                                                (9, (64, 128, 64), "sigmoid")])
def test_restatement_agrees_with_a_torch_module(od, hidden, act_name):
    params = vmc.value_weights(od, hidden)
    norm = vmc.value_norm(od)
    obs = vmc.states(11, 50, od, norm).astype(np.float64)
    acts = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "swish": lambda x: x * torch.sigmoid(x)}
    x = torch.from_numpy((obs - norm["obs"][0]) / (norm["obs"][1] + 1e-10))
    for li in range(len(hidden) + 1):
        x = x @ torch.from_numpy(params[2 * li]).double() + torch.from_numpy(params[2 * li + 1]).double()
        if li < len(hidden):
            x = acts[act_name](x)
    want = x[:, 0].numpy() * (norm["value"][1] + 1e-10) + norm["value"][0]
    np.testing.assert_allclose(vmc.restate(params, norm, act_name, obs), want, rtol=1e-12, atol=1e-12)
    bad = obs.copy()
    bad[3, od - 1] = np.inf
    bad[7, 0] = np.nan
    got = vmc.restate(params, norm, act_name, bad)
    assert np.isnan(got[3]) and np.isnan(got[7]) and np.isfinite(np.delete(got, [3, 7])).all()


def test_augmented_returns_are_the_trace_total_plus_the_term_on_its_last_state():
    from oracle.planner import rollout_trace, sample_rs_actions
    from oracle.rewards import make_reward
    case = cases.CASES["hc_rs_discount"]
    env, _, norms = cases.recipe(case)
    od = env.observation_space.shape[0]
    gold = cases.load_golden("hc_rs_discount_s0")
    dyn, rf = cases.oracle_dynamics(case), make_reward(case["env"], env.dt)
    params, norm = vmc.value_weights(od, (64,)), vmc.value_norm(od, base=norms[0])
    np.random.seed(0)
    actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
    total, trace = rollout_trace(dyn, rf, gold["obs0"], actions, case["n"], case["discount"])
    aug, tot2, tr2 = vmc.augmented_returns(dyn, rf, vmc.value_fn(params, norm, "relu"), gold["obs0"], actions, case["n"],
                                           case["discount"], 0.5)
    assert np.array_equal(tot2, total) and np.array_equal(tr2, trace)
    term = 0.5 * case["discount"] ** case["h"] * vmc.restate(params, norm, "relu", trace[case["h"] - 1])
    np.testing.assert_allclose(aug, total + term, rtol=1e-13, atol=1e-13)
    assert np.std(term) > 1e-3                  # (not a constant: the candidates end in different states)
    # the fp32 fold restated: w rounded once, a multiply and an add, w == 0 leaves the returns' bits
    r32, v32 = total.astype(np.float32), vmc.restate(params, norm, "relu", trace[-1]).astype(np.float32)
    w = np.float32(0.5 * vmc.discount_pow(case["discount"], case["h"]))
    assert np.array_equal(vmc.fold_f32(r32, v32, case["discount"], case["h"], 0.5), r32 + w * v32)
    assert abs(vmc.discount_pow(0.9, 7) - 0.9 ** 7) < 1e-15
    v32[0] = np.nan
    assert np.array_equal(vmc.fold_f32(r32, v32, case["discount"], case["h"], 0.0).view(np.uint32), r32.view(np.uint32))
    assert np.isnan(vmc.fold_f32(r32, v32, case["discount"], case["h"], 0.5)[0])


def _recipe():
    from oracle.planner import sample_rs_actions
    from oracle.rewards import make_reward
    case = dict(cases.CASES[vmc.RECIPE_CASE])
    env, _, norms = cases.recipe(case)
    od = env.observation_space.shape[0]
    gold = cases.load_golden(vmc.RECIPE_CASE + "_s0")
    dyn, rf = cases.oracle_dynamics(case), make_reward(case["env"], env.dt)
    params, norm, act = vmc.recipe_value(norms[0], od)
    np.random.seed(vmc.RECIPE_SEED)
    actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
    aug, total, _ = vmc.augmented_returns(dyn, rf, vmc.value_fn(params, norm, act), gold["obs0"], actions, case["n"],
                                          case.get("discount", 1.0), vmc.RECIPE_COEF)
    return case, env, gold, dyn, rf, (params, norm, act), actions, aug.reshape(case["m"], -1), total.reshape(case["m"], -1)


def test_the_recorded_recipe_changes_the_oracles_winner():
    case, _, _, _, _, _, _, aug, total = _recipe()
    assert case["h"] == 3
    assert np.any(np.argmax(aug, axis=1) != np.argmax(total, axis=1))
    assert np.all(vmc.margins(aug) > 2 * RTOL) and np.all(vmc.margins(total) > 2 * RTOL)


# ------------------------------------------------------------------------------------------
# 5. the controller: constructor errors, and the routing with the native calls stubbed
# ------------------------------------------------------------------------------------------
def _value_model(env, hidden=(64, 64), act="relu", base=None):
    od = env.observation_space.shape[0]
    vm = MLPValueModel(name="val", env=env, hidden_sizes=hidden, hidden_nonlinearity=act, init_seed=0)
    vm.set_params(vmc.value_weights(od, hidden))
    vm.set_normalization(vmc.value_norm(od, base=base))
    return vm


def test_constructor_errors():
    case = cases.CASES["hc_rs_m3_n64_h5"]
    env, model = cases.product_model(case)
    kw = dict(name="policy", env=env, dynamics_model=model, n_candidates=case["n"], horizon=case["h"])
    with pytest.raises(_lib.L2AError, match="not eligible.*no host fallback.*width 96"):
        MPCController(value_model=_value_model(env, hidden=(96,)), **kw)

    class Plain(object):
        def predict(self, obs):
            return np.zeros(len(obs))

    with pytest.raises(_lib.L2AError, match="no host fallback"):
        MPCController(value_model=Plain(), **kw)
    vm = _value_model(env)
    for key in ("native_cem_step", "native_mppi_step", "native_icem_step"):
        with pytest.raises(_lib.L2AError, match="plans through the Python loop: the C controller steps"):
            MPCController(value_model=vm, rng="device", use_cem=(key == "native_cem_step"), use_mppi=(key == "native_mppi_step"),
                          use_icem=(key == "native_icem_step"), **dict(kw, **{key: True}))
    with pytest.raises(ValueError, match="terminal_value_coef"):
        MPCController(value_model=vm, terminal_value_coef=float("nan"), **kw)
    ens_case = cases.CASES["hc_rs_m2_n100_h7_e2"]
    env2, ens = cases.product_model(ens_case)
    with pytest.raises(_lib.L2AError, match="not built"):
        MPCController(name="policy", env=env2, dynamics_model=ens, ensemble_planning="particles", value_model=_value_model(env2))

    class Custom(SyntheticEnv):         # a reward the library does not know, and no reward model: nothing would add the value
        def reward(self, obs, act, nxt):
            return np.zeros(len(obs))

    custom = Custom("half_cheetah")
    custom.reward_spec = None
    with pytest.raises(_lib.L2AError, match="needs a plan the library scores"):
        MPCController(name="policy", env=custom, dynamics_model=model, value_model=vm)
    # the recurrent controller does not take the keyword
    rnn_case = cases.CASES[cases.rnn_case_ids()[0].rsplit("_s", 1)[0]]
    renv, rnn_model = cases.product_rnn_model(rnn_case)
    with pytest.raises(TypeError):
        RNNMPCController(name="policy", env=renv, dynamics_model=rnn_model, value_model=vm)
    # without a value model nothing changes
    plain = MPCController(**kw)
    assert plain.value_model is None and not plain._program()
    with_vm = MPCController(value_model=vm, terminal_value_coef=0.5, **kw)
    assert with_vm._program() and with_vm._fusable() and with_vm.terminal_value_coef == 0.5


class _FakeNative(object):
    """Stands in for ``NativeModel``: ``plan_rs_value`` computes the shard's augmented returns with the oracle."""

    def __init__(self, dyn, rf, vfn):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim = 20, 6
        self.dyn, self.rf, self.vfn = dyn, rf, vfn
        self.calls = []
        self.lib = _lib.load()

    def plan_rs_value(self, obs0, actions, m, n, h, discount, reward, value_model, value_coef=1.0, cand_offset=0, returns_out=None,
                      best_key=None, traj_out=None):
        assert value_model == "native value handle"
        rets = vmc.augmented_returns(self.dyn, self.rf, self.vfn, obs0.numpy().astype(np.float64), actions.numpy().astype(np.float64),
                                     n, discount, value_coef)[0].reshape(m, n).astype(np.float32)
        self.calls.append((n, cand_offset, value_coef))
        if returns_out is not None:
            returns_out.copy_(torch.from_numpy(rets))
        if best_key is not None:
            for i in range(m):
                best_key[i] = max(self.lib.l2a_key_encode(ctypes.c_float(float(rets[i, j])), cand_offset + j) for j in range(n))

    def plan_rs(self, *a, **kw):
        raise AssertionError("a plan with a value model must not take an entry without the value")

    plan_rs_program = plan_rs_reward_model = plan_rs_sync = plan_rs_chunk = plan_rs


def _routed_controller(**kw):
    case, env, gold, dyn, rf, (params, norm, act), actions, aug, total = _recipe()
    _, model = cases.product_model(case)
    vm = MLPValueModel(name="val", env=env, hidden_sizes=vmc.RECIPE_HIDDEN, hidden_nonlinearity=act, init_seed=0)
    vm.set_params(params)
    vm.set_normalization(norm)
    vm.planner_value_model = lambda: "native value handle"
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, value_model=vm, terminal_value_coef=vmc.RECIPE_COEF,
                         discount=case.get("discount", 1.0), n_candidates=case["n"], horizon=case["h"], **kw)
    fake = _FakeNative(dyn, rf, vmc.model_value_fn(vm))
    stock_rollout = ctrl._rollout
    oracle_backend.install(ctrl, case)
    ctrl._rollout = stock_rollout                                       # the routing under test
    ctrl._upload_obs = lambda observations: torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32))
    model.planner_model = lambda: fake
    return case, env, gold, ctrl, fake, actions, aug, total


def test_value_model_routes_random_shooting_and_follows_the_oracle_in_both_settings():
    case, env, gold, ctrl, fake, actions, aug, total = _routed_controller()
    m, n = case["m"], case["n"]
    first = actions[0].reshape(m, n, -1)
    np.random.seed(vmc.RECIPE_SEED)
    got, info = ctrl.get_actions(gold["obs0"])
    assert info == {} and fake.calls == [(n, 0, vmc.RECIPE_COEF)]
    best = np.argmax(aug, axis=1)
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, first[np.arange(m), best])
    # and without the value model the same seed picks the oracle's other winner
    plain = cases.product_controller(case)
    oracle_backend.install(plain, case)
    np.random.seed(vmc.RECIPE_SEED)
    got0, _ = plain.get_actions(gold["obs0"])
    best0 = np.argmax(total, axis=1)
    np.testing.assert_array_equal(got0, first[np.arange(m), best0])
    assert np.any(best0 != best) and not np.array_equal(got0, got)


def test_value_model_declines_the_l2a_reward_paths():
    case, env, gold, ctrl, fake, _, _, _ = _routed_controller()
    assert not ctrl._can_pipeline(case["h"] + 5, case["n"]) and not ctrl._can_pipeline_cem(1, 1, case["n"])
    assert ctrl._native_rs_step(np.zeros((2, 20)), 2) is None and ctrl._native_cem_step(np.zeros((2, 20))) is None
    assert fake.calls == []


@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
def test_value_model_routes_cem(cem_mode):
    case, env, gold, ctrl, fake, _, _, _ = _routed_controller(use_cem=True, num_cem_iters=2, cem_mode=cem_mode)
    np.random.seed(0)
    got, _ = ctrl.get_actions(gold["obs0"])
    assert fake.calls == [(case["n"], 0, vmc.RECIPE_COEF)] * 2 and got.shape == (case["m"], 6)
