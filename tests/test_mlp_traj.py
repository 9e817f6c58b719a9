"""The MLP planner's trajectory rollout without a GPU: the ABI of ``l2a_rollout_traj`` / ``l2a_mlp_traj_geometry``, the path
decision against a Python restatement of the launcher's eligibility arithmetic and automatic rule, and the routing of
``MPCController`` with the native calls stubbed (an env with a ``RewardProgram``, a controller with an ``MLPRewardModel``)."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases
import oracle_backend
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel
from learning_to_adapt_amd.envs import RewardProgram
from learning_to_adapt_amd.policies import MPCController
from mlp_traj_rows import ROWS, row_n
from oracle.planner import cem_plan, rollout_returns, rs_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("l2a_rollout_traj", "l2a_mlp_traj_geometry")
LDS = 160 * 1024


# ------------------------------------------------------------------------------------------
# 1. the ABI
# ------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "l2a.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
    assert not hasattr(lib, "l2a_launch_mlp_micro_traj")        # internal to the library


def test_rollout_rejects_a_null_model():
    """The rejection that needs no model (those that do: tests/test_mlp_traj_gpu.py)."""
    null = ctypes.c_void_p()
    assert _lib.load().l2a_rollout_traj(null, null, null, 1, 1, 1, 0, null, null) == _lib.L2A_EINVAL


@pytest.mark.parametrize("args", [
    dict(obs_dim=0), dict(act_dim=0), dict(n_hidden=0), dict(n_hidden=9), dict(hidden=0), dict(n_sets=0), dict(m=0), dict(n=0), dict(h=0),
    dict(micro=-1), dict(micro=3),
    dict(m=1 << 15, n=1 << 15),                     # more than 2^30 - 1 candidates
    dict(mode="per_block", n_sets=2, m=3),          # more envs than weight sets
])
def test_geometry_rejects(args):
    kw = dict(obs_dim=20, act_dim=6, n_hidden=2, hidden=512, mode="single", n_sets=1, m=2, n=37, h=3, micro=2, cus=256)
    kw.update(args)
    with pytest.raises(_lib.L2AError):
        _lib.mlp_traj_geometry(**kw)
    lib, out = _lib.load(), (ctypes.c_int * 8)()
    assert lib.l2a_mlp_traj_geometry(20, 6, 2, 512, 0, 1, 2, 37, 3, 2, 256, None) == _lib.L2A_EINVAL
    assert lib.l2a_mlp_traj_geometry(20, 6, 2, 512, 7, 1, 2, 37, 3, 2, 256, out) == _lib.L2A_EINVAL       # unknown mode
    assert lib.l2a_mlp_traj_geometry(20, 6, 2, 512, 0, 1, 2, 37, 3, 2, 256, out) == _lib.L2A_OK


# ------------------------------------------------------------------------------------------
# 2. single launch or chain: the launcher's conditions, restated
# ------------------------------------------------------------------------------------------
def _cd(a, b):
    return -(-a // b)


def _set_stride(od, ad, nh, H, micro_ok):
    """Floats of one weight set in the model's storage (``l2a_model_create``): every region rounded up to 16 floats."""
    off = 0

    def take(n):
        nonlocal off
        off += _cd(n, 16) * 16

    def packed(k_in, n_out):
        return _cd(n_out, 16) * _cd(k_in, 16) * 256
    KG0, OT = _cd(od + ad, 16), _cd(od, 16)
    k_in = od + ad
    for l in range(nh + 1):
        n_out = H if l < nh else od
        take(k_in * n_out)
        take(n_out)
        k_in = n_out
    take(packed(od + ad, H))
    take(packed(H, H) * (nh - 1))
    take(packed(H, od))
    if micro_ok:
        take(_micro_floats(H, KG0, nh))
    take(16 * OT)
    take(32 * KG0 + 32 * OT)
    return off


def _micro_floats(H, KG0, nh):
    nrec = 4 * ((KG0 + 1) & ~1) + (nh - 1) * (H // 4) + 16
    return (H // 64) * nrec * 256


def _restated(od, ad, nh, H, mode, E, m, n, h, micro, cus):
    """``plan_traj_rollout`` (csrc/l2a_api.hip) as plain arithmetic: eligibility of the single launch, then the policy."""
    cus = cus if cus > 0 else 256
    mfma_ok = H in (128, 256, 512) and 1 <= nh <= 8 and 1 <= od <= 64 and 1 <= ad <= 16 and od + ad <= 80
    micro_ok = mfma_ok and H in (256, 512)
    chain = dict(single=False, launches=h, workgroups=m * _cd(n, 16), workgroups_per_env=0, micro_tiles=99, full_workgroups=0)
    if not micro_ok:
        return chain
    KG0 = _cd(od + ad, 16)
    e_loop = E if mode == "mean" else 1
    quads = _cd(n, 4)
    W = min(cus // m, quads)
    hi = _cd(quads, W) if W > 0 else 99
    if hi <= 3:
        W = _cd(quads, hi)
        hi = _cd(quads, W)
    chain["micro_tiles"] = hi
    smem = (2 * 12 * (H + 88) + e_loop * 12 * 104 + e_loop * (32 * KG0 + 192 + nh * H)) * 4 + 2 * 4 * 3 * 64 * 16
    span = ((m if mode == "per_block" else e_loop) - 1) * _set_stride(od, ad, nh, H, micro_ok) * 4 + _micro_floats(H, KG0, nh) * 4
    eligible = hi <= 3 and smem <= LDS and span < 2 ** 31 and m * n * od * 4 < 2 ** 31 - 16 and m * n * ad * 4 < 2 ** 31 - 16
    tiles16 = m * _cd(n, 16)
    wanted = micro == 2 or (micro == 1 and (e_loop == 1 or 2 * tiles16 > cus))      # the measured classes: DESIGN 4.8
    if not (eligible and wanted):
        return chain
    return dict(single=True, launches=1, workgroups=m * W, workgroups_per_env=W, micro_tiles=hi, full_workgroups=quads - W * (hi - 1))


MODES = [("single", 1), ("per_block", 5), ("mean", 2), ("mean", 3), ("mean", 5)]


@pytest.mark.parametrize("cus", [32, 64, 256, 304])
@pytest.mark.parametrize("micro", [0, 1, 2])
def test_geometry_is_the_launchers_arithmetic_over_a_sweep(micro, cus):
    singles = hi3 = hi4 = 0
    for H in (128, 256, 512):
        for nh in (1, 2, 3):
            for mode, E in MODES:
                for m in (1, 2, 5):
                    edge = 12 * (cus // m)              # the last n of three micro tiles per workgroup, then the first of four
                    for n in (1, 3, 4, 5, 37, 100, 500, 1027, edge - 4, edge, edge + 1, 4000):
                        for od, ad in ((20, 6), (49, 8)):
                            got = _lib.mlp_traj_geometry(od, ad, nh, H, mode, E, m, n, 3, micro=micro, cus=cus)
                            assert got == _restated(od, ad, nh, H, mode, E, m, n, 3, micro, cus), (H, nh, mode, E, m, n, od, ad)
                            singles += got["single"]
                            hi3 += got["micro_tiles"] == 3 and n == edge
                            hi4 += got["micro_tiles"] == 4 and n == edge + 1
    assert (singles == 0) == (micro == 0) and hi3 > 0 and hi4 > 0


def test_geometry_at_the_limits():
    g = _lib.mlp_traj_geometry
    # three micro tiles per workgroup fit, four do not (256 CUs: n = 3072 | 3073)
    assert g(20, 6, 2, 512, "single", 1, 1, 3072, 10, micro=2, cus=256) == dict(
        single=True, launches=1, workgroups=256, workgroups_per_env=256, micro_tiles=3, full_workgroups=256)
    assert g(20, 6, 2, 512, "single", 1, 1, 3073, 10, micro=2, cus=256) == dict(
        single=False, launches=10, workgroups=193, workgroups_per_env=0, micro_tiles=4, full_workgroups=0)
    # the LDS: eight sets of 3 x 512, five of 6 x 512 need more than 160 KiB
    for nh, E, fits in ((3, 5, True), (3, 8, False), (5, 5, True), (6, 5, False)):
        args = (20, 6, nh, 512, "mean", E, 1, 3000, 4)
        assert g(*args, micro=2, cus=256)["single"] == fits and g(*args, micro=2, cus=256) == _restated(*args, 2, 256)
    # a step's slice of the trajectory inside one buffer descriptor: < 2^31 - 16 bytes (a device of 2^22 CUs, so that the plan fits)
    big = 1 << 22
    for n, fits in ((8388607, True), (8388608, False)):
        args = (64, 16, 2, 256, "single", 1, 1, n, 2)
        assert n * 64 * 4 < 2 ** 31 - 16 if fits else n * 64 * 4 >= 2 ** 31 - 16
        assert g(*args, micro=2, cus=big)["single"] == fits and g(*args, micro=2, cus=big) == _restated(*args, 2, big)
    # ... and of the actions, where they are wider than the observation
    args = (4, 16, 2, 256, "single", 1, 1, 40000000, 2)
    assert not g(*args, micro=2, cus=1 << 24)["single"] and g(*args, micro=2, cus=1 << 24) == _restated(*args, 2, 1 << 24)
    # the weight sets a per-block plan streams span less than 2^31 bytes
    for m, fits in ((100, True), (400, False)):
        args = (20, 6, 3, 512, "per_block", 400, m, 40, 2)
        assert g(*args, micro=2, cus=big)["single"] == fits and g(*args, micro=2, cus=big) == _restated(*args, 2, big)
    # width 128 has no micro-tile instance; more envs than CUs have no workgroup geometry
    assert g(20, 6, 2, 128, "single", 1, 1, 40, 3, micro=2, cus=256)["micro_tiles"] == 99
    assert g(20, 6, 2, 512, "single", 1, 300, 40, 3, micro=2, cus=256) == dict(
        single=False, launches=3, workgroups=900, workgroups_per_env=0, micro_tiles=99, full_workgroups=0)


def test_the_automatic_rule_takes_the_measured_classes():
    """profiles/mlp_traj.jsonl: one set per candidate at any size, mean ensembles of more than CUs / 2 16-candidate tiles."""
    g = lambda *a: _lib.mlp_traj_geometry(*a, micro=1, cus=256)["single"]      # noqa: E731
    assert g(20, 6, 2, 512, "single", 1, 1, 500, 10)            # config-1 shape
    assert g(41, 8, 3, 512, "per_block", 5, 5, 500, 10)         # GrBAL default
    assert g(20, 6, 2, 256, "single", 1, 1, 500, 10) and g(41, 8, 3, 256, "per_block", 5, 5, 500, 10)
    assert g(20, 6, 2, 512, "single", 1, 1, 3000, 10) and g(20, 6, 2, 512, "single", 1, 1, 100, 10)
    assert not g(20, 6, 2, 512, "mean", 5, 1, 100, 10) and not g(20, 6, 2, 512, "mean", 5, 1, 500, 10)
    assert not g(20, 6, 2, 256, "mean", 5, 1, 500, 10)
    assert not g(20, 6, 2, 512, "mean", 5, 1, 2048, 10) and g(20, 6, 2, 512, "mean", 5, 1, 2049, 10)     # 128 | 129 tiles
    assert g(20, 6, 2, 256, "mean", 5, 1, 2100, 10) and g(20, 6, 2, 512, "mean", 5, 1, 3000, 10)
    assert _lib.mlp_traj_geometry(41, 8, 3, 512, "per_block", 5, 5, 500, 10, micro=1, cus=256) == dict(
        single=True, launches=1, workgroups=210, workgroups_per_env=42, micro_tiles=3, full_workgroups=41)
    # every recorded plan: the rule is the recorded verdict
    import json
    seen = 0
    for line in open(os.path.join(ROOT, "profiles", "mlp_traj.jsonl")):
        r = json.loads(line)
        if r["kind"] != "plan":
            continue
        od, ad = (41, 8) if r["mode"] == "per_block" else (20, 6)
        auto = _lib.mlp_traj_geometry(od, ad, len(r["hidden"]), r["hidden"][0], r["mode"], r["n_sets"], r["m"], r["n"], r["h"], micro=1,
                                      cus=r["compute_units"])["single"]
        assert r["single_wins"] == (r["single_over_parent_chain"] < 1.0 - r["spread"]) and auto == r["single_wins"], r["plan"]
        seen += 1
    assert seen >= 10


def test_the_gpu_rows_on_256_cus():
    """What tests/test_mlp_traj_gpu.py's rows reach at 256 CUs (its own asserts read the CU count from the context)."""
    g = {r["id"]: _lib.mlp_traj_geometry(r["od"], r["ad"], len(r["hidden"]), r["hidden"][0], r["mode"], r["E"], r["m"], row_n(r, 256),
                                         r["h"], micro=2, cus=256) for r in ROWS}
    assert all(x["single"] for x in g.values())
    assert (g["h256x1_n3"]["workgroups"], g["h256x1_n3"]["micro_tiles"]) == (1, 1)
    assert (g["h256x2_tanh_above_cus"]["micro_tiles"], g["h256x2_tanh_above_cus"]["full_workgroups"]) == (2, 128)    # 128 x 2 + 1 x 1
    assert (g["h512x3_pb_above_2cus"]["micro_tiles"], g["h512x3_pb_above_2cus"]["workgroups_per_env"],
            g["h512x3_pb_above_2cus"]["full_workgroups"]) == (3, 86, 85)                                               # 85 x 3 + 1 x 2


# ------------------------------------------------------------------------------------------
# 3. the controller's routing, native calls stubbed
# ------------------------------------------------------------------------------------------
CASE = "hc_rs_m3_n64_h5"


class _FakeNative(object):
    """Stands in for ``NativeModel``: the two plan entries compute the shard's returns with the float64 oracle."""

    def __init__(self, case, fn):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim = 20, 6
        self.dyn, self.fn = cases.oracle_dynamics(case), fn
        self.calls = []
        self.lib = _lib.load()

    def _plan(self, kind, obs0, actions, m, n, h, discount, cand_offset, returns_out, best_key):
        rets = rollout_returns(self.dyn, self.fn, obs0.numpy().astype(np.float64), actions.numpy().astype(np.float64), n,
                               discount).reshape(m, n).astype(np.float32)
        self.calls.append((kind, n, cand_offset))
        if returns_out is not None:
            returns_out.copy_(torch.from_numpy(rets))
        if best_key is not None:
            for i in range(m):
                best_key[i] = max(self.lib.l2a_key_encode(ctypes.c_float(float(rets[i, j])), cand_offset + j) for j in range(n))

    def plan_rs_program(self, obs0, actions, m, n, h, discount, program, cand_offset=0, returns_out=None, best_key=None, traj_out=None):
        assert isinstance(program, RewardProgram)
        self._plan("program", obs0, actions, m, n, h, discount, cand_offset, returns_out, best_key)

    def plan_rs_reward_model(self, obs0, actions, m, n, h, discount, reward_model, cand_offset=0, returns_out=None, best_key=None,
                             traj_out=None):
        assert reward_model == "native reward handle"
        self._plan("model", obs0, actions, m, n, h, discount, cand_offset, returns_out, best_key)

    def plan_rs(self, *a, **kw):
        raise AssertionError("a plan that is scored by a launch of its own must not take an l2a_reward entry")

    plan_rs_sync = plan_rs_chunk = rollout_traj = plan_rs           # (the controller needs no call of the rollout alone)


def _routed(reward, **kw):
    case = cases.CASES[CASE]
    env, model = cases.product_model(case)
    if reward == "program":
        env = rpc.program_env(case["env"])
        fn = env.reward
    else:
        rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(64, 64), init_seed=0)
        rm.set_params(rmc.reward_weights(20, 6, (64, 64)))
        rm.set_normalization(rmc.reward_norm(20, 6, base=cases.recipe(case)[2][0]))
        rm.planner_reward_model = lambda: "native reward handle"
        kw.update(reward_model=rm, use_reward_model=True)
        fn = rmc.model_reward_fn(rm)
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0), n_candidates=case["n"],
                         horizon=case["h"], **kw)
    fake = _FakeNative(case, fn)
    stock_rollout = ctrl._rollout
    oracle_backend.install(ctrl, case)
    ctrl._rollout = stock_rollout                                       # the routing under test
    ctrl._upload_obs = lambda observations: torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32))
    model.planner_model = lambda: fake
    return case, env, ctrl, fake


@pytest.mark.parametrize("reward", ["program", "model"])
def test_random_shooting_reaches_the_plan_entry_with_the_oracles_action(reward):
    case, env, ctrl, fake = _routed(reward)
    assert ctrl._fusable() and ctrl._program()
    gold = cases.load_golden(CASE + "_s0")
    np.random.seed(0)
    want, best, returns, _ = rs_plan(fake.dyn, fake.fn, gold["obs0"], env.action_space.low, env.action_space.high, case["n"], case["h"],
                                     case.get("discount", 1.0))
    state = np.random.get_state()
    np.random.seed(0)
    got, info = ctrl.get_actions(gold["obs0"])
    after = np.random.get_state()
    assert info == {} and fake.calls == [(reward, case["n"], 0)]
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


@pytest.mark.parametrize("reward", ["program", "model"])
def test_cem_reaches_the_plan_entry_with_the_oracles_action(reward):
    case, env, ctrl, fake = _routed(reward, use_cem=True, num_cem_iters=1, cem_mode="reference")
    gold = cases.load_golden(CASE + "_s0")
    np.random.seed(0)
    want, best, returns = cem_plan(fake.dyn, fake.fn, gold["obs0"], env.action_space.low, env.action_space.high, case["n"], case["h"],
                                   case.get("discount", 1.0), num_cem_iters=1, percent_elites=ctrl.percent_elites)
    state = np.random.get_state()
    np.random.seed(0)
    got, _ = ctrl.get_actions(gold["obs0"])
    after = np.random.get_state()
    assert fake.calls == [(reward, case["n"], 0)]
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
