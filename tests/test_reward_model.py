"""Learned reward models without a GPU: the library's host-only eligibility check, the ABI, the scorer's launch geometry
(``l2a_reward_model_geometry`` over the table of tests/reward_model_geometries.py), the float64 restatement of
the model's semantics against a ``torch`` module, ``MLPRewardModel.fit``, and the controller's routing with the native
calls stubbed."""

import ctypes
import pickle

import numpy as np
import pytest
import torch

import cases
import oracle_backend
import reward_model_cases as rmc
import reward_model_geometries as rmg
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel
from learning_to_adapt_amd.envs import SyntheticEnv
from learning_to_adapt_amd.policies import MPCController

NEW_SYMBOLS = ("l2a_reward_model_check", "l2a_reward_model_create", "l2a_reward_model_destroy",
               "l2a_reward_model_set_weights", "l2a_reward_model_set_norm", "l2a_reward_model_predict",
               "l2a_score_trajectory_model", "l2a_plan_rs_reward_model")


def _check(obs, act, hidden, code=_lib.ACT_CODES["relu"]):
    lib = _lib.load()
    arr = (ctypes.c_int * max(len(hidden), 1))(*hidden)
    rc = lib.l2a_reward_model_check(obs, act, len(hidden), arr, code)
    return rc, lib.l2a_last_error(None).decode()


# ------------------------------------------------------------------------------------------
# 1. the validator and the ABI
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs,act,hidden,code,word", [
    (20, 6, (96,), 1, "width 96"),
    (20, 6, (256, 576), 1, "width 576"),
    (20, 6, (0,), 1, "width 0"),
    (20, 6, (), 1, "0 hidden layers"),
    (20, 6, (64, 64, 64, 64), 1, "4 hidden layers"),
    (65, 6, (64,), 1, "obs_dim 65"),
    (0, 6, (64,), 1, "obs_dim 0"),
    (20, 17, (64,), 1, "act_dim 17"),
    (20, 0, (64,), 1, "act_dim 0"),
    (20, 6, (64,), 5, "activation 5"),
    (20, 6, (64,), -1, "activation -1"),
])
def test_check_rejects(obs, act, hidden, code, word):
    rc, msg = _check(obs, act, hidden, code)
    assert rc == _lib.L2A_EINVAL
    assert msg.startswith("reward model: ") and word in msg


@pytest.mark.parametrize("obs,act,hidden,code", [
    (64, 16, (512, 512, 512), 4),       # every upper limit
    (1, 1, (64,), 0),                   # every lower limit
    (17, 5, (64, 64), 2),               # 2 * 17 + 5 = 39 inputs: no multiple of 4
    (41, 8, (128, 64), 3),              # unequal widths
    (20, 6, (256, 256), 1),
])
def test_check_accepts(obs, act, hidden, code):
    assert _check(obs, act, hidden, code)[0] == _lib.L2A_OK
    names = {v: k for k, v in _lib.ACT_CODES.items() if k is not None}
    assert _lib.reward_model_check(obs, act, hidden, names[code]) is None


def test_check_through_python_gives_the_reason():
    assert "width 96" in _lib.reward_model_check(20, 6, (96,), "relu")
    assert "activation" in _lib.reward_model_check(20, 6, (64,), "gelu")


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert not hasattr(lib, "l2a_reward_model_facts")       # internal to the library


# ------------------------------------------------------------------------------------------
# 1b. the scorer's launch geometry (l2a_reward_model_geometry: the launcher's own function, no GPU)
# ------------------------------------------------------------------------------------------
def _geo(obs, act, hidden, rows, h, cus, lds=rmg.LDS):
    g = _lib.reward_model_geometry(obs, act, hidden, rows, h, cus=cus, lds_per_block=lds)
    return (g["RT"], g["CT"], g["S"]), g


@pytest.mark.parametrize("cus", rmg.CUS)
@pytest.mark.parametrize("row", rmg.ROWS, ids=lambda r: r.id)
def test_every_table_row_takes_its_geometry(row, cus):
    n = rmg.plan_n(row, cus)
    rows = row.m * n
    assert rows >= row.a * 16 * cus + row.b and (row.m == 1 or n % 16) and rows < row.a * 16 * cus + row.b + 2 * row.m
    geo, g = _geo(row.obs, row.act, row.hidden, rows, row.h, cus)
    assert geo == row.expect
    RT, CT, S = geo
    assert g["workgroups"] == -(-rows // (16 * CT)) and g["passes"] == -(-row.h // S)
    kgs = max([-(-(2 * row.obs + row.act) // 16)] + [w // 16 for w in row.hidden])
    assert g["lds_bytes"] == RT * kgs * 1024
    # what the row is there for: a ragged candidate tile in the last workgroup, and empty ones behind it at CT >= 2
    if row.m == 1:
        last = rows - (g["workgroups"] - 1) * 16 * CT
        assert last % 16 == 5 and (CT == 1 or last < 16 * (CT - 1))


def test_the_table_covers_every_geometry_width_and_activation():
    assert sorted(rmg.GEOMETRIES) == sorted({(rt, rt // s, s) for rt in (1, 2, 4, 8) for s in (1, 2, 4, 8) if rt % s == 0})
    assert len(rmg.GEOMETRIES) == 10 and {r.expect for r in rmg.ROWS} == set(rmg.GEOMETRIES)
    assert len({r.id for r in rmg.ROWS}) == len(rmg.ROWS)
    widths = {w for r in rmg.ROWS for w in r.hidden}
    assert {64, 128, 192, 256, 320, 384, 448, 512} <= widths
    assert {(3, 1), (17, 5), (20, 6), (41, 8), (64, 16)} <= {(r.obs, r.act) for r in rmg.ROWS}
    assert {(64, 512), (512, 64), (128, 448, 64)} <= {r.hidden for r in rmg.ROWS}
    assert any(-(-(2 * r.obs + r.act) // 16) > max(r.hidden) // 16 for r in rmg.ROWS)         # kgs = KG0
    acts = {"identity", "relu", "tanh", "sigmoid", "swish"}
    assert {r.activation for r in rmg.ROWS if r.h > r.expect[2]} == acts                         # on a multi-pass row
    assert {r.activation for r in rmg.ROWS if r.expect[1] > 1} == acts                           # on a CT > 1 row
    assert {r.expect[1] for r in rmg.ROWS if r.m == 3 and r.expect[1] > 1} == {2, 4, 8}         # env boundaries in a workgroup
    for r in rmg.ROWS:
        assert r.a == 0 or len(r.hidden) <= 2                                                   # large-row cases stay shallow
    twin = rmg.by_id(rmg.PREDICT[0])
    assert twin.expect == (8, 8, 1) and twin.m == 1 and twin.h == 1
    assert any(r.expect == (8, 8, 1) and r.m == 3 and r.h == 1 and r.id not in rmg.PREDICT for r in rmg.ROWS)


WIDTH_CLASSES = [(20, 6, (64 * t,)) for t in range(1, 9)] + [(64, 16, (64,)), (20, 6, (64, 512)), (41, 8, (128, 448, 64)),
                                                               (3, 1, (256, 256))]


@pytest.mark.parametrize("obs,act,hidden", WIDTH_CLASSES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_geometry_properties_over_a_sweep(obs, act, hidden):
    tpw = max(hidden) // 64
    kgs = max([-(-(2 * obs + act) // 16)] + [w // 16 for w in hidden])
    rows_sweep = sorted(set(list(range(1, 70001, 997)) + [16 * k * cus + d for cus in rmg.CUS for k in range(1, 9)
                                                          for d in (-1, 0, 1, 37) if 0 < 16 * k * cus + d <= 70000] + [70000]))
    seen = set()
    for cus in rmg.CUS:
        for rows in rows_sweep:
            for h in range(1, 34):
                (RT, CT, S), g = _geo(obs, act, hidden, rows, h, cus)
                assert CT * S == RT and RT in (1, 2, 4, 8)
                assert RT * tpw <= 32
                assert RT * kgs * 1024 + 4096 <= rmg.LDS
                assert S == 1 or S // 2 < h
                assert g["workgroups"] == -(-rows // (16 * CT)) and g["passes"] == -(-h // S)
                seen.add((RT, CT, S))
    assert seen <= set(rmg.GEOMETRIES) and max(g[0] for g in seen) == max(rt for rt in (1, 2, 4, 8) if rt * tpw <= 32)


def test_the_geometries_design_quotes():
    """DESIGN section 4.9, a (256, 256) net on 256 CUs: config 2 runs 125 workgroups x 4 passes of 8 steps, the config-1 shape
    32 workgroups x 3 passes of 4 steps."""
    geo, g = _geo(20, 6, (256, 256), 2000, 30, 256)
    assert geo == (8, 1, 8) and g["workgroups"] == 125 and g["passes"] == 4 and g["lds_bytes"] == 128 * 1024
    geo, g = _geo(20, 6, (256, 256), 500, 10, 256)
    assert geo == (4, 1, 4) and g["workgroups"] == 32 and g["passes"] == 3
    assert _geo(20, 6, (256, 256), 500, 10, 0) == (geo, g)                  # num_cu <= 0 means 256
    assert _geo(20, 6, (256, 256), 500, 10, -3) == (geo, g)


def test_geometry_rejects():
    lib = _lib.load()
    out = (ctypes.c_int * 8)()
    hid = (ctypes.c_int * 2)(256, 256)
    call = lambda **kw: lib.l2a_reward_model_geometry(*[kw.get(k, d) for k, d in (                      # noqa: E731
        ("obs", 20), ("act", 6), ("n_hidden", 2), ("hidden", hid), ("rows", 500), ("h", 10), ("cus", 256), ("lds", rmg.LDS), ("out", out))])
    assert call() == _lib.L2A_OK and list(out)[:5] == [4, 1, 4, 32, 3] and list(out)[6:] == [0, 0]
    assert call(out=None) == _lib.L2A_EINVAL
    assert call(rows=0) == _lib.L2A_EINVAL and call(rows=-5) == _lib.L2A_EINVAL
    assert call(h=0) == _lib.L2A_EINVAL
    assert call(hidden=None) == _lib.L2A_EINVAL
    for kw, word in ((dict(obs=65), "obs_dim 65"), (dict(act=17), "act_dim 17"), (dict(n_hidden=0), "0 hidden layers"),
                     (dict(n_hidden=4), "4 hidden layers"), (dict(hidden=(ctypes.c_int * 2)(256, 96)), "width 96")):
        assert call(**kw) == _lib.L2A_EINVAL and word in lib.l2a_last_error(None).decode()
    assert call(lds=8 * 1024) == _lib.L2A_EINVAL            # not even RT = 1 fits
    with pytest.raises(_lib.L2AError, match="width 96"):
        _lib.reward_model_geometry(20, 6, (96,), 100, 3)
    assert "l2a_reward_model_geometry" in _lib.EXPORTED_SYMBOLS


# ------------------------------------------------------------------------------------------
# 2. the float64 restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_name", ["relu", "tanh", "sigmoid", "swish", "identity"])
@pytest.mark.parametrize("od,ad,hidden", [(17, 5, (64, 64)), (41, 8, (128, 64)), (20, 6, (64,))])
def test_restatement_agrees_with_a_torch_module(od, ad, hidden, act_name):
    params = rmc.reward_weights(od, ad, hidden)
    norm = rmc.reward_norm(od, ad)
    obs0, traj, actions = rmc.inputs(3, 1, 50, od, ad, 1, norm)
    obs, nxt, act = np.repeat(obs0, 50, axis=0).astype(np.float64), traj[0].astype(np.float64), actions[0].astype(np.float64)
    layers = []
    sizes = [2 * od + ad] + list(hidden) + [1]
    mods = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid, "swish": torch.nn.SiLU,
            "identity": torch.nn.Identity}
    for li in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[li], sizes[li + 1]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(params[2 * li].astype(np.float64).T))
            lin.bias.copy_(torch.from_numpy(params[2 * li + 1].astype(np.float64)))
        layers.append(lin)
        if li < len(sizes) - 2:
            layers.append(mods[act_name]())
    net = torch.nn.Sequential(*layers)
    x = np.concatenate([(obs - norm["obs"][0]) / (norm["obs"][1] + 1e-10), (act - norm["act"][0]) / (norm["act"][1] + 1e-10),
                        ((nxt - obs) - norm["delta"][0]) / (norm["delta"][1] + 1e-10)], axis=1)
    with torch.no_grad():
        z = net(torch.from_numpy(x))[:, 0].numpy()
    want = z * (norm["reward"][1] + 1e-10) + norm["reward"][0]
    got = rmc.restate(params, norm, act_name, obs, act, nxt)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    # identity statistics, and a non-finite input anywhere in the row
    with torch.no_grad():
        z0 = net(torch.from_numpy(np.concatenate([obs, act, nxt - obs], axis=1)))[:, 0].numpy()
    np.testing.assert_allclose(rmc.restate(params, None, act_name, obs, act, nxt), z0, rtol=1e-12, atol=1e-12)
    for which, col in ((0, 3), (1, 2), (2, od - 1)):
        rows = [obs.copy(), act.copy(), nxt.copy()]
        rows[which][7, col] = np.inf if which else np.nan
        bad = rmc.restate(params, norm, act_name, *rows)
        assert np.isnan(bad[7]) and np.array_equal(np.delete(bad, 7), np.delete(got, 7))


# ------------------------------------------------------------------------------------------
# 3. MLPRewardModel on the host
# ------------------------------------------------------------------------------------------
def _cheetah_data(seed, rows):
    env = SyntheticEnv("half_cheetah")
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    rs = np.random.RandomState(seed)
    obs = rs.randn(rows, od)
    act = rs.uniform(-1.0, 1.0, (rows, ad))
    nxt = obs + 0.1 * rs.randn(rows, od)
    return env, obs, act, nxt, env.reward(obs, act, nxt)


def test_fit_lowers_the_held_out_error():
    env, obs, act, nxt, rew = _cheetah_data(0, 3000)
    _, obs_t, act_t, nxt_t, rew_t = _cheetah_data(1, 1000)
    model = MLPRewardModel(name="rew", env=env, hidden_sizes=(64, 64), batch_size=250, learning_rate=0.003, init_seed=0)
    np.random.seed(0)
    torch.manual_seed(0)
    model.fit(obs, act, nxt, rew, epochs=0)                 # statistics only
    assert set(model.normalization) == {"obs", "act", "delta", "reward"}
    assert model.normalization["reward"] == (float(np.mean(rew)), float(np.std(rew)))
    before = float(np.mean((rmc.model_reward_fn(model)(obs_t, act_t, nxt_t) - rew_t) ** 2))
    stats = model.fit(obs, act, nxt, rew, epochs=15, compute_normalization=False)
    after = float(np.mean((rmc.model_reward_fn(model)(obs_t, act_t, nxt_t) - rew_t) ** 2))
    print("held-out MSE of the reward: %.4f before, %.4f after the fit (reward variance %.4f)" % (before, after, np.var(rew_t)))
    assert after < before and after < np.var(rew_t)
    assert np.isfinite(stats["TrainLoss"]) and np.isfinite(stats["ValidLoss"])


def test_model_pickles_with_its_weights_and_statistics():
    env = SyntheticEnv("half_cheetah")
    model = MLPRewardModel(name="rew", env=env, hidden_sizes=(64,), hidden_nonlinearity="tanh", init_seed=3)
    model.set_params(rmc.reward_weights(20, 6, (64,)))
    model.set_normalization(rmc.reward_norm(20, 6))
    twin = pickle.loads(pickle.dumps(model))
    assert twin.hidden_sizes == (64,) and twin.hidden_nonlinearity == "tanh" and twin._native is None
    for a, b in zip(model.get_param_values().items(), twin.get_param_values().items()):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    for key in ("obs", "act", "delta", "reward"):
        assert np.array_equal(model.normalization[key][0], twin.normalization[key][0])
    assert list(model.get_param_values()) == ["hidden_0/kernel", "hidden_0/bias", "output/kernel", "output/bias"]
    assert model.native_eligible() is None
    assert "width 96" in MLPRewardModel(name="rew", env=env, hidden_sizes=(96,)).native_eligible()
    with pytest.raises(ValueError):
        MLPRewardModel(name="rew", env=env, hidden_nonlinearity="gelu")


# ------------------------------------------------------------------------------------------
# 4. the controller's routing, native calls stubbed
# ------------------------------------------------------------------------------------------
class _FakeNative(object):
    """Stands in for ``NativeModel``: ``plan_rs_reward_model`` computes the shard's returns with the oracle."""

    def __init__(self, case, fn):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim = 20, 6
        self.dyn, self.fn = cases.oracle_dynamics(case), fn
        self.calls = []
        self.lib = _lib.load()

    def plan_rs_reward_model(self, obs0, actions, m, n, h, discount, reward_model, cand_offset=0, returns_out=None,
                             best_key=None, traj_out=None):
        from oracle.planner import rollout_returns
        assert reward_model == "native reward handle"
        rets = rollout_returns(self.dyn, self.fn, obs0.numpy().astype(np.float64), actions.numpy().astype(np.float64), n,
                               discount).reshape(m, n).astype(np.float32)
        self.calls.append((n, cand_offset))
        if returns_out is not None:
            returns_out.copy_(torch.from_numpy(rets))
        if best_key is not None:
            for i in range(m):
                best_key[i] = max(self.lib.l2a_key_encode(ctypes.c_float(float(rets[i, j])), cand_offset + j) for j in range(n))

    def plan_rs(self, *a, **kw):
        raise AssertionError("a reward-model plan must not take l2a_plan_rs")

    plan_rs_program = plan_rs_sync = plan_rs_chunk = plan_rs


def _routed_controller(hidden=(64, 64), **kw):
    case = cases.CASES["hc_rs_m3_n64_h5"]
    env, model = cases.product_model(case)
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=hidden, init_seed=0)
    rm.set_params(rmc.reward_weights(20, 6, hidden))
    rm.set_normalization(rmc.reward_norm(20, 6, base=cases.recipe(case)[2][0]))
    rm.planner_reward_model = lambda: "native reward handle"
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, reward_model=rm, use_reward_model=True,
                         discount=case.get("discount", 1.0), n_candidates=case["n"], horizon=case["h"], **kw)
    fake = _FakeNative(case, rmc.model_reward_fn(rm))
    stock_rollout = ctrl._rollout
    oracle_backend.install(ctrl, case)
    ctrl._rollout = stock_rollout                                       # the routing under test
    ctrl._upload_obs = lambda observations: torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32))
    model.planner_model = lambda: fake
    return case, env, rm, ctrl, fake


def test_native_reward_model_routes_random_shooting():
    from oracle.planner import rs_plan
    case, env, rm, ctrl, fake = _routed_controller()
    assert ctrl._reward_spec is None and ctrl._native_reward_model() is rm and ctrl._fusable() and ctrl._program()
    gold = cases.load_golden("hc_rs_m3_n64_h5_s0")
    np.random.seed(0)
    want, best, returns, _ = rs_plan(fake.dyn, fake.fn, gold["obs0"], env.action_space.low, env.action_space.high, case["n"],
                                     case["h"], case.get("discount", 1.0))
    state = np.random.get_state()
    np.random.seed(0)
    got, info = ctrl.get_actions(gold["obs0"])
    after = np.random.get_state()
    assert info == {} and fake.calls == [(case["n"], 0)]
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    assert not np.array_equal(returns, gold["returns"])                 # not the env's own reward


@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
def test_native_reward_model_routes_cem(cem_mode):
    from oracle.planner import cem_plan
    case, env, rm, ctrl, fake = _routed_controller(use_cem=True, num_cem_iters=1, cem_mode=cem_mode)
    gold = cases.load_golden("hc_rs_m3_n64_h5_s0")
    np.random.seed(0)
    got, _ = ctrl.get_actions(gold["obs0"])                             # raised "needs a fusable closed-form reward" before
    assert fake.calls == [(case["n"], 0)] and got.shape == (case["m"], 6)
    if cem_mode == "reference":
        np.random.seed(0)
        want, best, _ = cem_plan(fake.dyn, fake.fn, gold["obs0"], env.action_space.low, env.action_space.high, case["n"],
                                 case["h"], case.get("discount", 1.0), num_cem_iters=1)
        assert np.array_equal(ctrl.last_plan["best_index"], best)
        np.testing.assert_array_equal(got, want)


def test_native_reward_model_declines_the_l2a_reward_paths():
    case, env, rm, ctrl, fake = _routed_controller()
    assert not ctrl._can_pipeline(case["h"] + 5, case["n"]) and not ctrl._can_pipeline_cem(1, 1, case["n"])
    assert ctrl._native_rs_step(np.zeros((3, 20)), 3) is None and ctrl._native_cem_step(np.zeros((3, 20))) is None
    assert fake.calls == []


def test_other_reward_models_keep_the_unfused_loop():
    case = cases.CASES["hc_rs_m3_n64_h5"]
    env, model = cases.product_model(case)

    class Plain(object):
        def predict(self, obs, act, nxt):
            return env.reward(obs, act, nxt)

    for rm in (Plain(), MLPRewardModel(name="rew", env=env, hidden_sizes=(96,)), None):
        ctrl = MPCController(name="policy", env=env, dynamics_model=model, reward_model=rm, use_reward_model=True,
                             n_candidates=case["n"], horizon=case["h"])
        assert ctrl._native_reward_model() is None and not ctrl._fusable() and not ctrl._program()
        taken = []
        ctrl._get_rs_action_unfused = lambda observations: taken.append(len(observations)) or np.zeros((3, 6))
        ctrl.get_actions(np.zeros((3, 20)))
        assert taken == [3]
        ctrl.use_cem = True
        with pytest.raises(_lib.L2AError, match="fusable"):
            ctrl.get_actions(np.zeros((3, 20)))
    # a native model that is handed over but not switched on changes nothing either
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=case["n"], horizon=case["h"],
                         reward_model=MLPRewardModel(name="rew", env=env, hidden_sizes=(64,)))
    assert ctrl._native_reward_model() is None and ctrl._fusable() and not ctrl._program() and ctrl._reward_spec is not None


def test_a_reward_spec_env_and_the_recurrent_controller_are_untouched():
    case = cases.CASES["hc_rs_m3_n64_h5"]
    ctrl = cases.product_controller(case)
    assert ctrl._native_reward_model() is None and ctrl._fusable() and not ctrl._program()
    oracle_backend.install(ctrl, case)
    gold = cases.load_golden("hc_rs_m3_n64_h5_s0")
    np.random.seed(0)
    got, _ = ctrl.get_actions(gold["obs0"])
    np.testing.assert_array_equal(got, gold["chosen"])
    rnn_case = cases.CASES[cases.rnn_case_ids()[0].rsplit("_s", 1)[0]]
    env, rnn_model = cases.product_rnn_model(rnn_case)
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(64,))
    rnn = cases.product_rnn_controller(rnn_case, model=rnn_model, env=env, reward_model=rm, use_reward_model=True)
    assert rnn._native_reward_model() is None and not rnn._fusable() and not rnn._program()
