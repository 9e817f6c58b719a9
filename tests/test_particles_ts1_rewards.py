"""TS1 particle plans of reward programs and reward models without a GPU: the three C entries' declarations and their refusal of
null handles, ``MPCController(ts1_step_rewards=...)`` - default, pickling, what it lifts and what it leaves - the routing of
``_rollout`` with the native calls stubbed, and the NumPy restatement of the step boundary
(``tests/particle_ts1_step_reference.py``) against ``RewardProgram.returns_f32``.

The declaration, keyword and routing tests exercise the product and fail without the feature; the two ``test_restatement_...``
tests touch the references only and pin what the GPU tests judge the product by."""

import ctypes
import inspect
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import cases
import particle_ts1_reference as t1
import particle_ts1_step_reference as ps
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs import RewardProgram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("l2a_particle_step", "l2a_plan_rs_particles_ts1_program", "l2a_plan_rs_particles_ts1_reward_model")
OBJ = os.path.join(ROOT, "learning_to_adapt_amd", "csrc", "_obj", "l2a_particle_step.o")
OD, AD = 20, 6


def _case(E=3, planner="rs", hidden=(128, 128)):
    return dict(env="half_cheetah", mode="mean", hidden=hidden, E=E, n=50, h=7, planner=planner)


def _program_controller(**kw):
    env, model = cases.product_model(_case())
    env.reward_spec = rpc.new_reward_program(OD, AD, env.dt)
    return cases.product_controller(_case(kw.pop("E", 3), kw.pop("planner", "rs")), model=model, env=env,
                                    ensemble_planning="particles", **kw)


def _reward_model(env, hidden=(64,)):
    from learning_to_adapt_amd.dynamics import MLPRewardModel
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=hidden, init_seed=0)
    rm.set_params(rmc.reward_weights(OD, AD, hidden))
    rm.set_normalization(rmc.reward_norm(OD, AD))
    return rm


def _reward_model_controller(**kw):
    env, model = cases.product_model(_case())
    rm = _reward_model(env)
    return rm, cases.product_controller(_case(), model=model, env=env, ensemble_planning="particles", reward_model=rm,
                                        use_reward_model=True, **kw)


# --------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    lib = _lib.load()
    c = ctypes
    vp, i32, f32, u64, i64, f64 = c.c_void_p, c.c_int, c.c_float, c.c_ulonglong, c.c_longlong, c.c_double
    tail = [f32, u64, u64, vp, i32, vp, vp, vp, vp, vp]
    want = {
        "l2a_particle_step": [vp, vp, i32, vp, vp, i64, vp, None, f64, vp, vp, vp, vp, u64, u64, i32, i32, i32, i32, i32, i32, i32, vp],
        "l2a_plan_rs_particles_ts1_program": [vp, vp, vp, i32, i32, i32, f64, None] + tail,
        "l2a_plan_rs_particles_ts1_reward_model": [vp, vp, vp, vp, i32, i32, i32, f64] + tail,
    }
    for name in SYMBOLS:
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl, name + " is not declared in include/l2a.h"
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is i32
        assert len(fn.argtypes) == len(want[name]) == decl.group(1).count(",") + 1, name
        for got, exp in zip(fn.argtypes, want[name]):
            assert exp is None or got is exp, name
    from test_abi import _declared_functions
    assert sorted(_lib.EXPORTED_SYMBOLS) == _declared_functions()


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    zero = ctypes.c_float(0.0)
    assert lib.l2a_particle_step(None, None, 0, None, None, 0, None, None, 1.0, None, None, None, None, 0, 0, 0, 1, 2, 1, 1, 1, 0,
                                 None) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_particles_ts1_program(None, None, None, 1, 1, 1, 1.0, None, zero, 0, 0, None, 0, None, None, None, None,
                                                 None) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_particles_ts1_reward_model(None, None, None, None, 1, 1, 1, 1.0, zero, 0, 0, None, 0, None, None, None,
                                                      None, None) == _lib.L2A_EINVAL


def test_step_kernel_has_no_scratch(tmp_path):
    """Read from the build's own object; where a library travelled without its objects, the unit is compiled with the build's flags."""
    from learning_to_adapt_amd.csrc import build as l2a_build
    obj = OBJ
    if not os.path.exists(obj):
        src, flags = l2a_build.unit_table()["l2a_particle_step.o"]
        obj = str(tmp_path / "l2a_particle_step.o")
        subprocess.run([l2a_build._hipcc()] + l2a_build.FLAGS + flags + ["-c", os.path.join(l2a_build.HERE, src), "-o", obj],
                       check=True, capture_output=True)
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa_notes.sh"), obj, "particle_step"], capture_output=True,
                         text=True, check=True).stdout
    line = [ln for ln in out.splitlines() if "l2a_particle_step_k" in ln]
    assert len(line) == 1, out
    assert "private_segment_fixed_size:0" in line[0] and "vgpr_spill_count:0" in line[0], line[0]


# -------------------------------------------------------------------------------------------------------------- the keyword
def test_keyword_default_and_pickle():
    from learning_to_adapt_amd.policies import MPCController, RNNMPCController
    params = inspect.signature(MPCController.__init__).parameters
    assert params["ts1_step_rewards"].default is False
    assert "ts1_step_rewards" not in inspect.signature(RNNMPCController.__init__).parameters
    assert cases.product_controller(_case()).ts1_step_rewards is False
    ctrl = _program_controller(particle_sampling="ts1", ts1_step_rewards=True, risk_coef=0.5)
    assert ctrl.ts1_step_rewards is True and isinstance(ctrl._reward_spec, RewardProgram) and ctrl._program()
    back = pickle.loads(pickle.dumps(ctrl))
    assert back.ts1_step_rewards is True and back.particle_sampling == "ts1" and back.risk_coef == 0.5
    assert isinstance(back._reward_spec, RewardProgram)
    assert pickle.loads(pickle.dumps(cases.product_controller(_case()))).ts1_step_rewards is False


def test_the_keyword_lifts_the_refusal_and_only_that():
    # off: the old refusals stand
    with pytest.raises(_lib.L2AError, match="reward program"):
        _program_controller(particle_sampling="ts1")
    with pytest.raises(_lib.L2AError, match="fused reward formula only"):
        _reward_model_controller(particle_sampling="ts1")
    with pytest.raises(_lib.L2AError, match="fused reward formula only"):
        _reward_model_controller(particle_sampling="ts1", ts1_step_rewards=False)
    # on: both construct, under every planner
    assert _program_controller(particle_sampling="ts1", ts1_step_rewards=True).particle_sampling == "ts1"
    assert _program_controller(particle_sampling="ts1", ts1_step_rewards=True, planner="cem")._program()
    for kw in (dict(use_mppi=True), dict(use_icem=True)):
        assert _program_controller(particle_sampling="ts1", ts1_step_rewards=True, rng="device", **kw)._program()
    rm, ctrl = _reward_model_controller(particle_sampling="ts1", ts1_step_rewards=True)
    assert ctrl._native_reward_model() is rm and ctrl._reward_spec is None
    # the keyword lifts nothing else
    with pytest.raises(ValueError, match="ensemble_planning='particles'"):
        cases.product_controller(_case(), particle_sampling="ts1", ts1_step_rewards=True)
    with pytest.raises(_lib.L2AError, match="native_cem_step"):
        _program_controller(particle_sampling="ts1", ts1_step_rewards=True, planner="cem", rng="device", native_cem_step=True)
    # and changes nothing where there was nothing to lift
    plain = cases.product_controller(_case(), ensemble_planning="particles", particle_sampling="ts1", ts1_step_rewards=True)
    assert not isinstance(plain._reward_spec, RewardProgram) and plain._reward_spec is not None
    assert _program_controller(ts1_step_rewards=True).particle_sampling == "tsinf"


# --------------------------------------------------------------------------------------------------------- routing (stubbed)
class _FakeNative(object):
    def __init__(self, E):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim, self.n_sets = OD, AD, E
        self.calls = []

    def plan_rs_particles(self, *a, **kw):
        self.calls.append(("tsinf", a, kw))

    def plan_rs_particles_ts1(self, *a, **kw):
        self.calls.append(("ts1", a, kw))


def _stub(ctrl):
    fake = _FakeNative(3)
    ctrl.dynamics_model.planner_model = lambda: fake
    ctrl._check_blocks = lambda m: None
    ctrl._upload_obs = lambda observations: None
    return fake


def test_rollout_hands_the_program_to_the_ts1_plan():
    obs, acts = np.zeros((2, OD)), torch.zeros((7, 2 * 50, AD))
    ctrl = _program_controller(particle_sampling="ts1", ts1_step_rewards=True, risk_coef=1.5)
    fake = _stub(ctrl)
    torch.manual_seed(1234)
    for _ in range(3):
        ctrl._rollout(obs, acts, 50, 5, True)
    m, h = 2, 7
    assert [c[0] for c in fake.calls] == ["ts1"] * 3
    assert [c[2]["offset"] for c in fake.calls] == [0, h * m, 2 * h * m]
    assert all(c[1][6] is ctrl._reward_spec and isinstance(c[1][6], RewardProgram) for c in fake.calls)
    assert all(c[2]["seed"] == 1234 and c[2]["cand_offset"] == 5 and c[2]["risk_coef"] == 1.5 for c in fake.calls)
    assert ctrl._particles["ts1_offset"] == 2 * h * m and ctrl._particles["members"].shape == (m, 3, 50)
    # TS-infinity on the same env is handed the same program
    ctrl = _program_controller(ts1_step_rewards=True)
    fake = _stub(ctrl)
    ctrl._rollout(obs, acts, 50, 0, True)
    assert [c[0] for c in fake.calls] == ["tsinf"] and fake.calls[0][1][6] is ctrl._reward_spec


def test_rollout_hands_the_native_reward_model_to_the_ts1_plan():
    obs, acts = np.zeros((2, OD)), torch.zeros((7, 2 * 50, AD))
    rm, ctrl = _reward_model_controller(particle_sampling="ts1", ts1_step_rewards=True)
    rm.planner_reward_model = lambda: "native reward handle"
    fake = _stub(ctrl)
    torch.manual_seed(77)
    for _ in range(2):
        ctrl._rollout(obs, acts, 50, 0, False)
    assert [c[0] for c in fake.calls] == ["ts1"] * 2
    assert all(c[1][6] == "native reward handle" for c in fake.calls)
    assert [c[2]["offset"] for c in fake.calls] == [0, 7 * 2] and fake.calls[0][2]["seed"] == 77
    assert fake.calls[0][2]["score_out"] is None
    # ... and TS-infinity makes the same choice
    rm, ctrl = _reward_model_controller(ts1_step_rewards=True)
    rm.planner_reward_model = lambda: "native reward handle"
    fake = _stub(ctrl)
    ctrl._rollout(obs, acts, 50, 0, True)
    assert [c[0] for c in fake.calls] == ["tsinf"] and fake.calls[0][1][6] == "native reward handle"


def test_controller_level_sharding_stays_refused():
    ctrl = _program_controller(particle_sampling="ts1", ts1_step_rewards=True)
    fake = _stub(ctrl)
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl._rollout(np.zeros((1, OD)), torch.zeros((7, 50, AD)), 50, 0, True)
    assert fake.calls == []


def test_native_model_routes_by_the_reward_kind(monkeypatch):
    """``NativeModel.plan_rs_particles_ts1`` picks the C entry by the reward's type and counts the plan (a stub library: no GPU)."""
    from learning_to_adapt_amd.dynamics import native_model as nm
    monkeypatch.setattr(nm, "_stream_ptr", lambda device: None)

    class _Lib(object):
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if not name.startswith("l2a_"):
                raise AttributeError(name)
            return lambda *a: self.calls.append((name, a)) or 0

    class _Ctx(object):
        def check(self, rc, what):
            self.what = what

    class _T(object):          # a tensor as far as the wrapper's assertions look
        is_cuda, dtype = True, torch.float32

        def __init__(self, count):
            self.count = count

        def is_contiguous(self):
            return True

        def numel(self):
            return self.count

        def data_ptr(self):
            return 64

    class _RM(nm.NativeRewardModel):
        def __init__(self):
            self.handle = ctypes.c_void_p(128)

        def __del__(self):
            pass

    model = nm.NativeModel.__new__(nm.NativeModel)
    model.__dict__.update(lib=_Lib(), ctx=_Ctx(), handle=ctypes.c_void_p(32), obs_dim=OD, act_dim=AD, n_sets=3,
                          device=torch.device("cpu"), program_plans=0, reward_model_plans=0)
    m, n, h = 2, 5, 4
    obs0, acts = _T(m * OD), _T(h * m * n * AD)
    prog = rpc.new_reward_program(OD, AD, 0.05)
    model.plan_rs_particles_ts1(obs0, acts, m, n, h, 0.9, prog, seed=3, offset=8, score_out=_T(m * n))
    assert model.lib.calls[-1][0] == "l2a_plan_rs_particles_ts1_program" and model.ctx.what == "l2a_plan_rs_particles_ts1_program"
    assert (model.program_plans, model.reward_model_plans, model.particle_plans) == (1, 0, 1)
    assert model.lib.calls[-1][1][3:7] == (m, n, h, 0.9) and model.lib.calls[-1][1][9:11] == (3, 8)
    rm = _RM()
    model.plan_rs_particles_ts1(obs0, acts, m, n, h, 0.9, rm, seed=3, offset=8, score_out=_T(m * n))
    assert model.lib.calls[-1][0] == "l2a_plan_rs_particles_ts1_reward_model" and model.lib.calls[-1][1][1] is rm.handle
    assert (model.program_plans, model.reward_model_plans, model.particle_plans) == (1, 1, 2)
    with pytest.raises(_lib.L2AError, match="RewardSpec, a RewardProgram or a NativeRewardModel"):
        model.plan_rs_particles_ts1(obs0, acts, m, n, h, 0.9, "a reward", score_out=_T(m * n))


# ------------------------------------------------------------------------------------------------------- the fp32 restatement
def _trajectory(seed, m, E, n, h):
    rs = np.random.RandomState(seed)
    pre0 = rs.randn(m, E, OD).astype(np.float32)
    posts = (rs.randn(h, m, E, n, OD) * 1.5).astype(np.float32)
    acts = rs.uniform(-1, 1, (h, m, E, n, AD)).astype(np.float32)
    return pre0, posts, acts


def test_restatement_with_identity_tables_is_returns_f32_bit_for_bit():
    m, E, n, h = 2, 3, 9, 5
    pre0, posts, acts = _trajectory(1, m, E, n, h)
    for prog in (rpc.every_kind_program(OD, AD), rpc.new_reward_program(OD, AD, 0.05)):
        for discount in (1.0, 0.97):
            got = ps.chain(pre0, posts, acts, t1.identity_table(m, n, E, h), discount, program=prog)
            rows = m * E * n
            want = prog.returns_f32(np.repeat(pre0.reshape(m * E, OD), n, axis=0), posts.reshape(h, rows, OD),
                                    acts.reshape(h, rows, AD), discount)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.int32).ravel(), want.view(np.int32))
            # given rewards: the same sum of the same step rewards
            rew = np.stack([prog.evaluate_f32(np.repeat(pre0.reshape(m * E, OD), n, axis=0) if t == 0 else posts[t - 1].reshape(rows, OD),
                                              acts[t].reshape(rows, AD), posts[t].reshape(rows, OD)).reshape(m, E, n) for t in range(h)])
            given = ps.chain(pre0, posts, acts, t1.identity_table(m, n, E, h), discount, rewards=rew)
            assert np.array_equal(given.view(np.int32), got.view(np.int32))
    # a non-identity table moves states and returns together: the particle that ends in block e collected pi's rewards
    prog = rpc.every_kind_program(OD, AD)
    table = t1.perm_table(5, 0, 0, m, n, E)
    state, ret = ps.step(pre0, posts[0], acts[0], None, 1.0, table, program=prog)
    _, plain = ps.step(pre0, posts[0], acts[0], None, 1.0, None, program=prog)
    want_s, want_r = t1.shuffle(posts[0], plain, table)
    assert np.array_equal(state, want_s) and np.array_equal(ret.view(np.int32), want_r.view(np.int32))
    assert not np.array_equal(ret, plain)


def test_restatement_at_horizon_one_ignores_the_tables_and_keeps_the_addition():
    m, E, n = 2, 3, 9
    pre0, posts, acts = _trajectory(2, m, E, n, 1)
    prog = rpc.every_kind_program(OD, AD)
    empty = np.zeros((0, m, n, E), dtype=np.uint8)
    got = ps.chain(pre0, posts, acts, empty, 0.9, program=prog)
    rows = m * E * n
    want = prog.returns_f32(np.repeat(pre0.reshape(m * E, OD), n, axis=0), posts.reshape(1, rows, OD), acts.reshape(1, rows, AD), 0.9)
    assert np.array_equal(got.view(np.int32).ravel(), want.view(np.int32))
    # step 0 without ret_in is 0 + disc * r: a -0 reward comes out +0, with a ret_in of -0 it stays -0
    rew = np.full((m, E, n), -0.0, dtype=np.float32)
    _, zero = ps.step(pre0, posts[0], acts[0], None, 1.0, None, rewards=rew)
    _, minus = ps.step(pre0, posts[0], acts[0], rew, 1.0, None, rewards=rew)
    assert not np.signbit(zero).any() and np.signbit(minus).all()
    # the margin helper: a row at a bound has margin 0, a row without INRANGE terms inf
    obs, act, nxt = np.zeros((2, OD)), np.zeros((2, AD)), np.zeros((2, OD))
    nxt[0, 5], nxt[1, 5] = 3.5, 0.75
    assert np.array_equal(ps.inrange_margin(prog, obs, act, nxt), [0.0, 2.75 / 3.5])
    assert np.isinf(ps.inrange_margin(RewardProgram().with_bias(1.0), obs, act, nxt)).all()
