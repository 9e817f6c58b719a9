"""TS1 particle plans without a GPU: the three C entries' declarations, ``l2a_particle_perm`` (host only) against the NumPy
restatement of ``tests/particle_ts1_reference.py``, the restatement against ``tests/particle_reference.py``, and every argument
check and the routing of ``MPCController(particle_sampling=...)``.

The declaration, ``l2a_particle_perm``, keyword and routing tests exercise the product and fail without the feature; the two
``test_restatement_...`` tests touch the references and the oracle only and pin what the GPU tests judge the product by.

Uniformity bounds (derived, not measured and then set): over N = 60 000 candidates of one fixed seed the count of an event of
probability p is binomial - standard deviation sqrt(N p (1 - p)) - up to the draw's bias of at most k / 2^32 per step, which is
below 1e-4 counts here.  Each of the 6 permutations of E = 3 (p = 1/6, sd 91.3) and each of the 25 (position, value) cells of E = 5
(p = 1/5, sd 98.0) lies within 5 standard deviations of N p.  The seed is fixed, so the test is deterministic."""

import ctypes
import inspect
import itertools
import os
import pickle
import re

import numpy as np
import pytest
import torch

import cases
import particle_reference as pr
import particle_ts1_reference as t1
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs.synthetic_env import SyntheticEnv
from learning_to_adapt_amd.utils import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("l2a_particle_perm", "l2a_particle_shuffle", "l2a_plan_rs_particles_ts1")
SEEDS = (0x0123456789ABCDEF, 7)
SENTINEL = 0xA5
TOP = (1 << 31) - 1


def _case(E=3, mode="mean", planner="rs", hidden=(128, 128)):
    return dict(env="half_cheetah", mode=mode, hidden=hidden, E=E, n=50, h=7, planner=planner)


def lib_perm(seed, offset, t, m, i_first, i_count, cand_first, cand_count, E, expect_rc=_lib.L2A_OK, null=False):
    """``l2a_particle_perm`` into a sentinel-filled array with 64 guard bytes on either side."""
    lib = _lib.load()
    size = max(i_count, 0) * max(cand_count, 0) * max(E, 1)
    buf = np.full(size + 128, SENTINEL, dtype=np.uint8)
    out = None if null else ctypes.c_void_p(buf.ctypes.data + 64)
    rc = lib.l2a_particle_perm(seed, offset, t, m, i_first, i_count, cand_first, cand_count, E, out)
    assert rc == expect_rc, (rc, seed, offset, t, m, i_first, i_count, cand_first, cand_count, E)
    assert np.all(buf[:64] == SENTINEL) and np.all(buf[64 + size:] == SENTINEL), "guard bytes overwritten"
    if rc != _lib.L2A_OK:
        assert np.all(buf == SENTINEL), "a refused call wrote its output"
        return None
    return buf[64:64 + size].reshape(i_count, cand_count, E).copy()


# --------------------------------------------------------------------------------------------------------------- declarations
def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    lib = _lib.load()
    c = ctypes
    vp, i32, f32, u64 = c.c_void_p, c.c_int, c.c_float, c.c_ulonglong
    want = {
        "l2a_particle_perm": [u64, u64, i32, i32, i32, i32, i32, i32, i32, vp],
        "l2a_particle_shuffle": [vp, vp, vp, vp, vp, vp, u64, u64, i32, i32, i32, i32, i32, i32, vp],
        "l2a_plan_rs_particles_ts1": [vp, vp, vp, i32, i32, i32, c.c_double, None, f32, u64, u64, vp, i32, vp, vp, vp, vp, vp],
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
    assert "TS1" in text and "TS-infinity" in text
    assert lib.l2a_particle_shuffle(None, None, None, None, None, None, 0, 0, 0, 1, 2, 1, 1, 0, None) == _lib.L2A_EINVAL
    assert lib.l2a_plan_rs_particles_ts1(None, None, None, 1, 1, 1, 1.0, None, ctypes.c_float(0.0), 0, 0, None, 0, None, None, None,
                                         None, None) == _lib.L2A_EINVAL


# ----------------------------------------------------------------------------------------------------------- l2a_particle_perm
@pytest.mark.parametrize("E", [1, 2, 3, 4, 5, 6, 8, 9, 16])
def test_perm_equals_the_restatement(E):
    m, t, count = 3, 6, 37
    for seed in SEEDS:
        for offset in (0, 1 << 20, (1 << 33) - (t + 1) * m):            # the last: the final slot is 2^33 - 1
            for first in (0, 1000, TOP - count):                        # gj up to 2^31 - 2
                got = lib_perm(seed, offset, t, m, 0, m, first, count, E)
                want = t1.perm_table(seed, offset, t, m, count, E, cand_offset=first)
                assert np.array_equal(got, want), (E, seed, offset, first)
                assert np.array_equal(np.sort(got, axis=2), np.broadcast_to(np.arange(E, dtype=np.uint8), got.shape)), "no permutation"
    if E > 1:       # the stream moves with every one of its five values
        base = lib_perm(SEEDS[0], 0, 0, m, 0, 1, 0, 200, E)
        assert not np.array_equal(base, lib_perm(SEEDS[1], 0, 0, m, 0, 1, 0, 200, E))
        assert not np.array_equal(base, lib_perm(SEEDS[0], 1, 0, m, 0, 1, 0, 200, E))
        assert not np.array_equal(base, lib_perm(SEEDS[0], 0, 1, m, 0, 1, 0, 200, E))
        assert not np.array_equal(base, lib_perm(SEEDS[0], 0, 0, m, 1, 1, 0, 200, E))
        assert not np.array_equal(base, lib_perm(SEEDS[0], 0, 0, m, 0, 1, 200, 200, E))
        assert np.array_equal(lib_perm(SEEDS[0], 0, 1, m, 0, 1, 0, 200, E), lib_perm(SEEDS[0], m, 0, m, 0, 1, 0, 200, E)), "slot = offset + t m + i"


def test_perm_is_positional():
    seed, offset, t, m, E = SEEDS[0], 12345, 2, 4, 5
    full = lib_perm(seed, offset, t, m, 0, m, 0, 300, E)
    for i_first, i_count, c_first, c_count in ((1, 2, 17, 100), (3, 1, 299, 1), (0, 4, 0, 1), (2, 0, 5, 5), (0, 1, 9, 0)):
        part = lib_perm(seed, offset, t, m, i_first, i_count, c_first, c_count, E)
        assert np.array_equal(part, full[i_first:i_first + i_count, c_first:c_first + c_count])


def test_perm_is_uniform():
    N, seed = 60000, 20181129
    p3 = lib_perm(seed, 0, 0, 1, 0, 1, 0, N, 3)[0].astype(np.int64)
    code = p3[:, 0] * 9 + p3[:, 1] * 3 + p3[:, 2]
    sd = np.sqrt(N * (1 / 6) * (5 / 6))
    worst3 = 0.0
    for perm in itertools.permutations(range(3)):
        count = int(np.sum(code == perm[0] * 9 + perm[1] * 3 + perm[2]))
        worst3 = max(worst3, abs(count - N / 6) / sd)
    p5 = lib_perm(seed, 0, 0, 1, 0, 1, 0, N, 5)[0]
    sd = np.sqrt(N * 0.2 * 0.8)
    worst5 = max(abs(int(np.sum(p5[:, pos] == val)) - N / 5) / sd for pos in range(5) for val in range(5))
    print("permutation counts: E=3 worst %.2f sd, E=5 cells worst %.2f sd" % (worst3, worst5))
    assert worst3 <= 5.0 and worst5 <= 5.0


def test_perm_refusals_leave_the_output_untouched():
    ok = dict(seed=1, offset=0, t=0, m=2, i_first=0, i_count=2, cand_first=0, cand_count=4, E=3)

    def refused(**kw):
        a = dict(ok, **kw)
        null = a.pop("null", False)
        lib_perm(a["seed"], a["offset"], a["t"], a["m"], a["i_first"], a["i_count"], a["cand_first"], a["cand_count"], a["E"],
                 expect_rc=_lib.L2A_EINVAL, null=null)

    lib_perm(**ok)
    refused(E=0)
    refused(E=17)
    refused(E=-1)
    refused(null=True)
    refused(t=-1)
    refused(m=0)
    refused(i_first=-1)
    refused(i_count=-1)
    refused(cand_first=-1)
    refused(cand_count=-1)
    refused(i_first=1, i_count=2)                       # env 2 of 2
    refused(cand_first=TOP - 3, cand_count=4)           # gj = 2^31 - 1
    lib_perm(**dict(ok, cand_first=TOP - 4))
    refused(offset=(1 << 33) - 1)                       # env 1's slot would be 2^33
    lib_perm(**dict(ok, offset=(1 << 33) - 2))
    refused(offset=(1 << 33) - 2, t=1)
    refused(offset=(1 << 64) - 1)
    refused(offset=(1 << 63) + 5)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def _plan(seed, m, n, h, E, hidden=(32, 32)):
    from oracle import planner
    env = SyntheticEnv("half_cheetah")
    sets, norms = synthetic.make_members(env, hidden, E)
    np.random.seed(seed)
    obs = synthetic.make_obs0(m, 20)
    return env, sets, norms, obs, planner.sample_rs_actions(env.action_space.low, env.action_space.high, n, m, h)


def test_restatement_with_identity_permutations_is_ts_infinity():
    m, n, h, E = 2, 9, 4, 3
    env, sets, norms, obs, actions = _plan(5, m, n, h, E)
    want = pr.member_returns64(env, sets, norms, obs, actions, n, discount=0.9)
    got = t1.particle_returns64(env, sets, norms, obs, actions, n, t1.identity_table(m, n, E, h), discount=0.9)
    assert np.array_equal(got, want)
    tables = np.stack([t1.perm_table(3, 0, t, m, n, E) for t in range(h - 1)])
    mixed = t1.particle_returns64(env, sets, norms, obs, actions, n, tables, discount=0.9)
    assert not np.array_equal(mixed, want), "the permutations changed nothing"


def test_restatement_at_horizon_one_ignores_the_permutations():
    m, n, E = 2, 9, 3
    env, sets, norms, obs, actions = _plan(6, m, n, 1, E)
    want = pr.member_returns64(env, sets, norms, obs, actions, n)
    got = t1.particle_returns64(env, sets, norms, obs, actions, n, np.zeros((0, m, n, E), dtype=np.uint8))
    assert np.array_equal(got, want)


def test_restated_shuffle_moves_state_and_return_together():
    rs = np.random.RandomState(1)
    m, E, n, O = 2, 4, 5, 3
    state, ret = rs.randn(m, E, n, O), rs.randn(m, E, n)
    table = t1.perm_table(9, 0, 0, m, n, E)
    s, r = t1.shuffle(state, ret, table)
    for i in range(m):
        for j in range(n):
            for e in range(E):
                assert np.array_equal(s[i, e, j], state[i, table[i, j, e], j]) and r[i, e, j] == ret[i, table[i, j, e], j]
    s, r = t1.shuffle(state, ret, t1.identity_table(m, n, E))
    assert np.array_equal(s, state) and np.array_equal(r, ret)


# ------------------------------------------------------------------------------------------------------ controller arguments
def test_defaults_change_nothing():
    from learning_to_adapt_amd.policies import MPCController, RNNMPCController
    assert inspect.signature(MPCController.__init__).parameters["particle_sampling"].default == "tsinf"
    assert inspect.signature(RNNMPCController.__init__).parameters["particle_sampling"].default == "tsinf"
    assert cases.product_controller(_case()).particle_sampling == "tsinf"
    assert cases.product_controller(_case(), ensemble_planning="particles").particle_sampling == "tsinf"


def test_keyword_and_pickle():
    ctrl = cases.product_controller(_case(E=2), ensemble_planning="particles", particle_sampling="ts1", risk_coef=0.5)
    assert ctrl.particle_sampling == "ts1" and ctrl._program() and ctrl.native_step is True
    back = pickle.loads(pickle.dumps(ctrl))
    assert back.particle_sampling == "ts1" and back.ensemble_planning == "particles" and back.risk_coef == 0.5
    assert pickle.loads(pickle.dumps(cases.product_controller(_case(), ensemble_planning="particles"))).particle_sampling == "tsinf"
    for kw in (dict(planner="cem"),):
        assert cases.product_controller(_case(**kw), ensemble_planning="particles", particle_sampling="ts1")._program()
    for kw in (dict(use_mppi=True), dict(use_icem=True)):
        assert cases.product_controller(_case(), rng="device", ensemble_planning="particles", particle_sampling="ts1", **kw)._program()


def test_argument_errors():
    from learning_to_adapt_amd.envs import RewardProgram
    with pytest.raises(ValueError, match="particle_sampling"):
        cases.product_controller(_case(), ensemble_planning="particles", particle_sampling="ts2")
    with pytest.raises(ValueError, match="ensemble_planning='particles'"):
        cases.product_controller(_case(), particle_sampling="ts1")
    with pytest.raises(_lib.L2AError, match="ensemble"):
        cases.product_controller(_case(E=1, mode="single"), ensemble_planning="particles", particle_sampling="ts1")
    with pytest.raises(_lib.L2AError, match="reward"):
        cases.product_controller(_case(), ensemble_planning="particles", particle_sampling="ts1", use_reward_model=True)
    env, model = cases.product_model(_case())
    import reward_program_cases as rpc
    env.reward_spec = rpc.new_reward_program(20, 6, env.dt)
    assert isinstance(env.reward_spec, RewardProgram)
    with pytest.raises(_lib.L2AError, match="reward program"):
        cases.product_controller(_case(), model=model, env=env, ensemble_planning="particles", particle_sampling="ts1")
    cases.product_controller(_case(), model=model, env=env, ensemble_planning="particles")      # (TS-infinity scores programs)
    with pytest.raises(_lib.L2AError, match="native_cem_step"):
        cases.product_controller(_case(planner="cem"), rng="device", ensemble_planning="particles", particle_sampling="ts1",
                                 native_cem_step=True)


def test_recurrent_controller_refuses_the_keyword():
    name = cases.rnn_case_ids()[0]
    case, _ = cases.split_id(name)
    with pytest.raises(_lib.L2AError, match="particle_sampling"):
        cases.product_rnn_controller(dict(case, planner="rnn_rs"), particle_sampling="ts1")
    assert cases.product_rnn_controller(dict(case, planner="rnn_rs"), particle_sampling="tsinf").ensemble_planning == "mean"


# --------------------------------------------------------------------------------------------------------- routing (stubbed)
class _FakeNative(object):
    def __init__(self, E):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim, self.n_sets = 20, 6, E
        self.calls = []

    def plan_rs_particles(self, *a, **kw):
        self.calls.append(("tsinf", a, kw))

    def plan_rs_particles_ts1(self, *a, **kw):
        self.calls.append(("ts1", a, kw))


def _stubbed(**kw):
    ctrl = cases.product_controller(_case(), ensemble_planning="particles", **kw)
    fake = _FakeNative(3)
    ctrl.dynamics_model.planner_model = lambda: fake
    ctrl._check_blocks = lambda m: None
    ctrl._upload_obs = lambda observations: None
    return ctrl, fake


def test_routing_tsinf_and_ts1():
    obs = np.zeros((2, 20))
    acts = torch.zeros((7, 2 * 50, 6))
    ctrl, fake = _stubbed()
    ctrl._rollout(obs, acts, 50, 0, True)
    assert [c[0] for c in fake.calls] == ["tsinf"] and "seed" not in fake.calls[0][2]

    for rng in ("numpy", "device"):
        ctrl, fake = _stubbed(particle_sampling="ts1", rng=rng, risk_coef=1.5)
        torch.manual_seed(1234)
        state = np.random.get_state()
        for _ in range(3):
            ctrl._rollout(obs, acts, 50, 5, True)
        assert [c[0] for c in fake.calls] == ["ts1"] * 3
        m, h = 2, 7
        assert [c[2]["offset"] for c in fake.calls] == [0, h * m, 2 * h * m]
        assert all(c[2]["seed"] == 1234 and c[2]["cand_offset"] == 5 and c[2]["risk_coef"] == 1.5 for c in fake.calls)
        assert fake.calls[0][1][2:6] == (m, 50, h, ctrl.discount) and fake.calls[0][1][6] is ctrl._reward_spec
        assert ctrl._particles["ts1_offset"] == 2 * h * m and ctrl._particles["members"].shape == (m, 3, 50)
        after = np.random.get_state()
        assert state[2] == after[2] and np.array_equal(state[1], after[1]), "np.random was consumed"
        torch.manual_seed(99)               # a changed seed restarts the counter
        ctrl._rollout(obs, acts, 50, 0, True)
        assert fake.calls[-1][2]["seed"] == 99 and fake.calls[-1][2]["offset"] == 0
        ctrl._rollout(obs[:1], acts[:, :50], 50, 0, False)
        assert fake.calls[-1][2]["offset"] == 1 * h * 1 and fake.calls[-1][2]["score_out"] is None


def test_controller_level_sharding_is_refused():
    ctrl, fake = _stubbed(particle_sampling="ts1")
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl._rollout(np.zeros((1, 20)), torch.zeros((7, 50, 6)), 50, 0, True)
    assert fake.calls == []
