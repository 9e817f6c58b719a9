"""The recurrent planner with a reward program or a learned reward model, without a GPU: the ABI of the new entry points, the
rollout's path decision (``l2a_lstm_traj_geometry``) against the arithmetic of the launcher's micro-tile conditions, and the
routing of ``RNNMPCController`` with the native calls stubbed.

Margin condition of every controller case: the float64 oracle's best return leads the runner-up by at least 1e-3 (relative to
``max(1, |best|)``) - a condition on the inputs, asserted on the oracle alone, so that an arg-max comparison is never a tie."""

import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import cases
import oracle_backend
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel, RNNDynamicsModel
from learning_to_adapt_amd.envs import RewardProgram, RewardSpec, SyntheticEnv
from learning_to_adapt_amd.policies import MPCController, RNNMPCController
from oracle import LSTMStateTuple
from oracle.rnn_planner import rnn_cem_plan, rnn_rollout_returns, rnn_rs_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("l2a_lstm_rollout_traj", "l2a_lstm_plan_rs_program", "l2a_lstm_plan_rs_reward_model", "l2a_lstm_traj_geometry")
MARGIN = 1e-3
CASE = "hc_rnn_rs_m2_n64_h4_reset"


# ------------------------------------------------------------------------------------------
# 1. the ABI
# ------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "l2a.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert not hasattr(lib, "l2a_launch_lstm_micro_traj")       # internal to the library


def test_entries_reject_a_null_model():
    """The rejections that need no model (those that do: tests/test_rnn_reward_paths_gpu.py)."""
    lib = _lib.load()
    null = ctypes.c_void_p()
    prog = RewardProgram().with_bias(1.0)
    assert lib.l2a_lstm_rollout_traj(null, null, null, null, null, 1, 1, 1, 0, null, null) == _lib.L2A_EINVAL
    assert lib.l2a_lstm_plan_rs_program(null, null, null, null, null, 1, 1, 1, 1.0, ctypes.byref(prog), 0, null, null, null,
                                        null) == _lib.L2A_EINVAL
    assert lib.l2a_lstm_plan_rs_reward_model(null, null, null, null, null, null, 1, 1, 1, 1.0, 0, null, null, null,
                                             null) == _lib.L2A_EINVAL


@pytest.mark.parametrize("args", [
    dict(obs_dim=0), dict(act_dim=0), dict(units=0), dict(units=1025), dict(m=0), dict(n=0), dict(h=0), dict(micro=-1), dict(micro=3),
    dict(m=1 << 15, n=1 << 15),         # more than 2^30 - 1 candidates
])
def test_geometry_rejects(args):
    kw = dict(obs_dim=20, act_dim=6, units=256, m=2, n=37, h=3, micro=2, cus=256)
    kw.update(args)
    with pytest.raises(_lib.L2AError):
        _lib.lstm_traj_geometry(**kw)
    out = (ctypes.c_int * 8)()
    assert _lib.load().l2a_lstm_traj_geometry(20, 6, 256, 2, 37, 3, 2, 256, None) == _lib.L2A_EINVAL
    assert _lib.load().l2a_lstm_traj_geometry(20, 6, 256, 2, 37, 3, 2, 256, out) == _lib.L2A_OK


# ------------------------------------------------------------------------------------------
# 2. single launch or chain: the launcher's micro-tile conditions, restated
# ------------------------------------------------------------------------------------------
def _restated(obs_dim, act_dim, units, m, n, h, micro, cus):
    """``plan_rnn_launch``'s conditions for micro tiles (csrc/l2a_lstm_api.hip), as plain arithmetic."""
    cus = cus if cus > 0 else 256
    eligible = units in (256, 512) and 1 <= obs_dim <= 64 and 1 <= act_dim <= 16 and obs_dim + act_dim <= 80
    quads = -(-n // 4)
    tiles16 = m * -(-n // 16)
    W = min(cus // m, quads)
    hi = -(-quads // W) if W > 0 else 99
    if 1 <= hi <= 3:
        W = -(-quads // hi)
    unfilled = 2 * tiles16 > cus and tiles16 < cus
    wanted = micro == 2 or (micro == 1 and (unfilled or hi == 1))
    single = eligible and hi <= 3 and wanted
    if not single:
        return dict(single=False, launches=h, workgroups=m * -(-n // 16), workgroups_per_env=0, micro_tiles=hi, full_workgroups=0)
    return dict(single=True, launches=1, workgroups=m * W, workgroups_per_env=W, micro_tiles=hi, full_workgroups=quads - W * (hi - 1))


#        units, obs, act, m, n, h
ROWS = [(256, 20, 6, 2, 37, 3),
        (256, 41, 8, 5, 500, 2),
        (512, 17, 5, 1, 1100, 2),
        (256, 64, 16, 3, 70, 2),
        (128, 20, 6, 2, 40, 3),          # no micro-tile instance: the chain
        (256, 20, 6, 5, 800, 3)]         # four micro tiles per CU at 256 CUs: the chain


@pytest.mark.parametrize("cus", [256, 304, 64, 0])
@pytest.mark.parametrize("micro", [0, 1, 2])
@pytest.mark.parametrize("row", ROWS, ids=lambda r: "u%d_o%d_a%d_m%d_n%d_h%d" % r)
def test_geometry_is_the_launchers_arithmetic(row, micro, cus):
    units, od, ad, m, n, h = row
    got = _lib.lstm_traj_geometry(od, ad, units, m, n, h, micro=micro, cus=cus)
    assert got == _restated(od, ad, units, m, n, h, micro, cus)
    if micro == 0:
        assert not got["single"]


def test_geometry_of_the_tabled_shapes():
    """What the GPU file's shapes reach at 256 CUs (its own asserts read the CU count from the context)."""
    g = [_lib.lstm_traj_geometry(od, ad, u, m, n, h, micro=2, cus=256) for u, od, ad, m, n, h in ROWS]
    assert [x["single"] for x in g] == [True, True, True, True, False, False]
    assert (g[0]["micro_tiles"], g[0]["workgroups"]) == (1, 20) and 37 % 4 == 1          # MT = 1, one live candidate in the last tile
    assert (g[1]["micro_tiles"], g[1]["workgroups_per_env"], g[1]["full_workgroups"]) == (3, 42, 41)     # 41 x 3 + 1 x 2 micro tiles
    assert (g[2]["micro_tiles"], g[2]["workgroups_per_env"], g[2]["full_workgroups"]) == (2, 138, 137)   # 137 x 2 + 1 x 1
    assert g[3]["micro_tiles"] == 1
    assert g[4]["launches"] == 3 and g[5]["micro_tiles"] == 4 and g[5]["launches"] == 3
    # the automatic policy: the plans the fused kernel gives micro tiles (the ReBAL default among them), no others
    auto = [_lib.lstm_traj_geometry(od, ad, u, m, n, h, micro=1, cus=256)["single"] for u, od, ad, m, n, h in ROWS]
    assert auto == [True, True, False, True, False, False]
    assert _lib.lstm_traj_geometry(20, 6, 256, 5, 500, 10, micro=1, cus=256) == dict(
        single=True, launches=1, workgroups=210, workgroups_per_env=42, micro_tiles=3, full_workgroups=41)


# ------------------------------------------------------------------------------------------
# 3. the controller's routing, native calls stubbed
# ------------------------------------------------------------------------------------------
class _FakeNativeLSTM(object):
    """Stands in for ``NativeLSTM``: the plan entries compute the shard's returns with the float64 oracle."""

    sync_max_envs = 64

    def __init__(self, case, fn):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim, self.units = 20, 6, case["units"]
        self.dyn, self.fn = cases.oracle_rnn_dynamics(case), fn
        self.calls = []
        self.lib = _lib.load()

    def _plan(self, kind, obs0, c0, h0, actions, m, n, h, discount, cand_offset, returns_out, best_key):
        hid = LSTMStateTuple(c0.numpy(), h0.numpy())
        rets = rnn_rollout_returns(self.dyn, self.fn, obs0.numpy().astype(np.float64), hid, actions.numpy().astype(np.float64), n,
                                   discount).reshape(m, n).astype(np.float32)
        self.calls.append((kind, n, cand_offset))
        if returns_out is not None:
            returns_out.copy_(torch.from_numpy(rets))
        if best_key is not None:
            for i in range(m):
                best_key[i] = max(self.lib.l2a_key_encode(ctypes.c_float(float(rets[i, j])), cand_offset + j) for j in range(n))

    def plan_rs_program(self, obs0, c0, h0, actions, m, n, h, discount, program, cand_offset=0, returns_out=None, best_key=None,
                        traj_out=None):
        assert isinstance(program, RewardProgram)
        self._plan("program", obs0, c0, h0, actions, m, n, h, discount, cand_offset, returns_out, best_key)

    def plan_rs_reward_model(self, obs0, c0, h0, actions, m, n, h, discount, reward_model, cand_offset=0, returns_out=None,
                             best_key=None, traj_out=None):
        assert reward_model == "native reward handle"
        self._plan("model", obs0, c0, h0, actions, m, n, h, discount, cand_offset, returns_out, best_key)

    def plan_rs(self, obs0, c0, h0, actions, m, n, h, discount, reward, cand_offset=0, returns_out=None, best_key=None):
        assert isinstance(reward, RewardSpec)       # (an l2a_reward: never a program)
        self._plan("spec", obs0, c0, h0, actions, m, n, h, discount, cand_offset, returns_out, best_key)

    def plan_rs_sync(self, *a, **kw):
        raise AssertionError("a plan that is scored by a launch of its own must not take an l2a_reward entry")

    plan_rs_chunk = plan_rs_sync

    def advance(self, obs, act, c, h):
        self.calls.append(("advance", obs.shape[0], 0))
        _, hid = self.dyn.predict(obs.numpy().astype(np.float64), act.numpy().astype(np.float64), LSTMStateTuple(c.numpy(), h.numpy()))
        return torch.from_numpy(np.asarray(hid.c, dtype=np.float32)), torch.from_numpy(np.asarray(hid.h, dtype=np.float32))


def _hidden(case, seed=5):
    rs = np.random.RandomState(seed)
    return LSTMStateTuple(rs.randn(case["m"], case["units"]).astype(np.float32),
                          np.tanh(rs.randn(case["m"], case["units"])).astype(np.float32))


def _routed(reward="program", hidden=(64, 64), wrap=False, **kw):
    """``RNNMPCController`` on the recipe model of CASE with a fake native model; its own ``_rollout`` / ``_plan_keys`` /
    ``_advance_hidden`` are the code under test."""
    case = cases.CASES[CASE]
    env = rpc.program_env(case["env"]) if reward == "program" else SyntheticEnv(case["env"])
    _, model = cases.product_rnn_model(case)
    rm = None
    if reward == "model":
        rm = MLPRewardModel(name="rew", env=env, hidden_sizes=hidden, init_seed=0)
        if rm.native_eligible() is None:
            rm.set_params(rmc.reward_weights(20, 6, hidden))
        rm.set_normalization(rmc.reward_norm(20, 6, base=cases.rnn_recipe(case)[2]))
        rm.planner_reward_model = lambda: "native reward handle"
        kw.update(reward_model=_PredictOnly(rm) if wrap else rm, use_reward_model=True)
    ctrl = RNNMPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0),
                            n_candidates=case["n"], horizon=case["h"], **kw)
    fn = env.reward_spec.evaluate if reward != "model" else rmc.model_reward_fn(rm)
    fake = _FakeNativeLSTM(case, fn)
    stock = (ctrl._rollout, ctrl._advance_hidden)
    oracle_backend.install_rnn(ctrl, case)
    ctrl._rollout, ctrl._advance_hidden = stock                         # the routing under test
    ctrl._upload_obs = lambda observations: torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32))
    model.planner_model = lambda: fake
    ctrl._hidden_state = _hidden(case)
    return case, env, rm, ctrl, fake


class _PredictOnly(object):
    def __init__(self, model):
        self.model = model

    def predict(self, obs, act, nxt):
        return rmc.model_reward_fn(self.model)(obs, act, nxt)


def _margin(returns):
    top = np.sort(returns, axis=1)
    return float(np.min((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1]))))


def _obs(case):
    return cases.load_golden(CASE + "_s0")["obs"][0]


def _check_rs(reward, kind, **kw):
    case, env, rm, ctrl, fake = _routed(reward, **kw)
    assert ctrl._fusable() and ctrl._program()
    obs, hid = _obs(case), _hidden(case)
    np.random.seed(0)
    want, best, returns, nxt = rnn_rs_plan(fake.dyn, fake.fn, obs, hid, env.action_space.low, env.action_space.high, case["n"],
                                           case["h"], case.get("discount", 1.0))
    state = np.random.get_state()
    print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
    assert _margin(returns) >= MARGIN
    np.random.seed(0)
    got, info = ctrl.get_actions(obs)
    after = np.random.get_state()
    assert info == {} and fake.calls == [(kind, case["n"], 0), ("advance", case["m"], 0)]
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    # the controller's own state moved on through `native.advance` (fp32 inputs: the oracle's step to rounding)
    np.testing.assert_allclose(ctrl._hidden_state.c, nxt.c, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ctrl._hidden_state.h, nxt.h, rtol=1e-5, atol=1e-6)


def test_a_program_env_routes_random_shooting():
    """On the parent commit this died on ``assert isinstance(reward, RewardSpec)`` in ``NativeLSTM.plan_rs``."""
    _check_rs("program", "program")


def test_a_native_reward_model_routes_random_shooting():
    _check_rs("model", "model", native_reward_model=True)


@pytest.mark.parametrize("reward,kind,kw", [("program", "program", {}), ("model", "model", dict(native_reward_model=True))])
@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
def test_cem_routes(reward, kind, kw, cem_mode):
    case, env, rm, ctrl, fake = _routed(reward, use_cem=True, num_cem_iters=1, cem_mode=cem_mode, **kw)
    obs, hid = _obs(case), _hidden(case)
    np.random.seed(0)
    got, _ = ctrl.get_actions(obs)
    assert fake.calls == [(kind, case["n"], 0), ("advance", case["m"], 0)] and got.shape == (case["m"], 6)
    if cem_mode == "reference":
        after = np.random.get_state()
        np.random.seed(0)
        want, best, returns, _ = rnn_cem_plan(fake.dyn, fake.fn, obs, hid, env.action_space.low, env.action_space.high, case["n"],
                                              case["h"], case.get("discount", 1.0), num_cem_iters=1,
                                              percent_elites=ctrl.percent_elites)
        state = np.random.get_state()
        print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
        assert _margin(returns) >= MARGIN
        assert np.array_equal(ctrl.last_plan["best_index"], best)
        np.testing.assert_array_equal(got, want)
        assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_the_old_paths_stay():
    # reward model without the keyword: not native, the reference's loop
    case, env, rm, ctrl, fake = _routed("model")
    assert ctrl._native_reward_model() is None and not ctrl._fusable() and not ctrl._program()
    taken = []
    ctrl._get_rs_action_unfused = lambda observations: taken.append(len(observations)) or np.zeros((case["m"], 6))
    ctrl._advance_hidden = lambda observations, actions: None
    ctrl.get_actions(_obs(case))
    assert taken == [case["m"]] and fake.calls == []
    ctrl.use_cem = True
    with pytest.raises(_lib.L2AError, match="fusable"):
        ctrl.get_actions(_obs(case))
    # with the keyword: a network the scorer does not take, and an object with nothing but `predict`, keep the loop too
    for kw in (dict(hidden=(96,)), dict(wrap=True)):
        case, env, rm, ctrl, fake = _routed("model", native_reward_model=True, **kw)
        assert ctrl._takes_reward_models and ctrl._native_reward_model() is None and not ctrl._fusable() and not ctrl._program()
    # a RewardSpec env: the fused l2a_reward entries as before
    case, env, rm, ctrl, fake = _routed("spec")
    assert isinstance(ctrl._reward_spec, RewardSpec) and ctrl._fusable() and not ctrl._program()
    a = torch.zeros((case["h"], case["m"] * case["n"], 6))
    ctrl._rollout(_obs(case), a, case["n"], 0, want_returns=True)
    assert fake.calls == [("spec", case["n"], 0)]
    # ... and the class default is what tests/test_reward_model.py pins
    assert RNNMPCController._takes_reward_models is False and MPCController._takes_reward_models is True


@pytest.mark.parametrize("reward,kw", [("program", {}), ("model", dict(native_reward_model=True))])
def test_the_l2a_reward_paths_decline(reward, kw):
    """The blocking launch, the chunk pipelines and the C steps hand ``_reward_spec`` to an ``l2a_reward`` entry: never entered."""
    case, env, rm, ctrl, fake = _routed(reward, **kw)
    assert ctrl._program()
    assert not ctrl._can_pipeline(case["h"] + 5, case["n"]) and not ctrl._can_pipeline_cem(1, 1, case["n"])
    assert ctrl._native_rs_step(np.zeros((2, 20)), 2) is None and ctrl._native_cem_step(np.zeros((2, 20))) is None
    assert fake.calls == []
    # `_plan_keys`, asked directly with everything else in favour of the blocking launch (one rank, random shooting)
    a = torch.zeros((case["h"], case["m"] * case["n"], 6))
    keys = ctrl._plan_keys(_obs(case), a, case["n"], 0, 1)
    assert torch.is_tensor(keys) and ctrl._hid_next is None and [c[0] for c in fake.calls] == [reward]


def test_pickle_keeps_the_keyword():
    case = cases.CASES[CASE]
    env, model = cases.product_rnn_model(case)
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(64,), init_seed=0)
    on = RNNMPCController(name="policy", env=env, dynamics_model=model, reward_model=rm, use_reward_model=True,
                          n_candidates=8, horizon=2, native_reward_model=True)
    off = RNNMPCController(name="policy", env=env, dynamics_model=model, reward_model=rm, use_reward_model=True,
                           n_candidates=8, horizon=2)
    assert on._native_reward_model() is rm and on._program() and off._native_reward_model() is None
    twin_on, twin_off = pickle.loads(pickle.dumps(on)), pickle.loads(pickle.dumps(off))
    assert twin_on._takes_reward_models is True and twin_on._native_reward_model() is twin_on.reward_model and twin_on._program()
    assert twin_off._takes_reward_models is False and twin_off._native_reward_model() is None and not twin_off._fusable()
    assert "native_reward_model" in RNNMPCController.__init__.__code__.co_varnames
    assert isinstance(model, RNNDynamicsModel)
