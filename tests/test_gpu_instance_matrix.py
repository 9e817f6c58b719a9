"""Every compiled rollout-kernel instance against the float64 oracle: one case per row of tests/instance_matrix.py.

Each MFMA / micro-tile MLP instance (unit x (OT, KG0) x variant x activation family x one-hidden-layer) and each LSTM instance
(units x (OT, KG0) x unit-tile split on / off, the two micro-tile ones) has its own register allocation and its own compile-time
bounds on the last observation tile and the last k-group; the rows put a model on the EDGES of those bounds and a plan on the
launch geometry that reaches the instance (asserted without a GPU in tests/test_instance_matrix.py; that routing assumes 256
compute units).  Per row:

  * every candidate's return against `oracle.planner.rollout_returns` in float64 (`rel_err < RTOL` of test_gpu_parity.py);
  * the published key decodes to the arg-max of the returns the kernel wrote and to that return, bit for bit;
  * the same plan relaunched with split = 0, fan = 0, micro = 0, double = 0 gives the same returns and keys bit for bit;
  * on one row per unit and (OT, KG0, variant) the generic VALU kernel agrees within 2e-5 and picks the same winner.

Rows that differ in policy alone share their model, inputs and oracle returns (`_mlp_case`, `_lstm_case`: read-only).

LSTM: the launcher has no dry run, so the routing of those rows rests on its conditions as read from l2a_lstm_api.hip (and
restated arithmetically in test_instance_matrix.py): with micro policy 0 the micro-tile branch is skipped (:199, `wanted`); the
unit-tile split is taken iff the split policy is non-zero and 2 x tiles <= CUs and h < 4096 (:221) - n = 37, m = 1 is three
tiles; with micro policy 2 a plan of at most three micro tiles per workgroup on 256 / 512 units takes the micro-tile kernel
(:192, :199; the generic stacks' branch at :136 is not involved: a single LSTM layer is not `generic`).  SPLIT on and SPLIT off
must agree bit for bit.
"""

import functools
import zlib

import numpy as np
import pytest
import torch

import instance_matrix as im
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_lstm import NativeLSTM
from learning_to_adapt_amd.dynamics.native_model import NativeModel
from learning_to_adapt_amd.envs import RewardSpec
from learning_to_adapt_amd.utils import synthetic
from oracle import LSTMStateTuple, OracleLSTMDynamics, OracleMLPDynamics
from oracle.planner import rollout_returns
from oracle.rnn_planner import rnn_rollout_returns
from test_gpu_parity import RTOL, rel_err

pytestmark = pytest.mark.gpu

OFFSET = 7
DISCOUNT = 0.9
VALU_RTOL = 2e-5                # test_gpu_parity.test_mfma_and_valu_kernels_agree
BASELINE = dict(split=0, fan=0, micro=0, double=0)
DEFAULTS = dict(split=1, fan=1, micro=1, double=1)


@pytest.fixture(scope="module", autouse=True)
def _needs_256_compute_units():
    cus = _lib.Context.get(0).info()["compute_units"]
    if cus != 256:
        pytest.skip("the routing of the instance matrix assumes 256 compute units (device reports %d)" % cus)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x3FFFFFFF


def _reward(kind, obs_dim):
    if kind == "dist":          # the last three observation dims
        return RewardSpec.make(dist_coef=1.0, ctrl_coef=0.005, dist_index=obs_dim - 3)
    return RewardSpec.make(w_vel=1.0, dt=0.05, ctrl_coef=0.05, vel_index=obs_dim - 1)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


class _Case(object):
    pass


@functools.lru_cache(maxsize=2)
def _mlp_case(obs_dim, act_dim, hidden, activation, E, mode, m, n, h, reward):
    key = (obs_dim, act_dim, hidden, activation, E, mode, m, n, h)
    rs = np.random.RandomState(_seed("inputs", *key))
    low, high = -np.ones(act_dim) * 2.0, np.ones(act_dim) * 2.0
    sets = [synthetic.make_weight_set(obs_dim, act_dim, list(hidden), _seed("weights", e, *key)) for e in range(E)]
    norms = [synthetic.make_norm(obs_dim, act_dim, low, high, _seed("norm", e, *key)) for e in range(E)]
    c = _Case()
    c.spec = _reward(reward, obs_dim)
    dyn = OracleMLPDynamics(obs_dim, act_dim, sets, norms, mode=mode, hidden_nonlinearity=activation)
    obs0 = rs.randn(m, obs_dim)
    acts = rs.uniform(low, high, (h, m * n, act_dim))
    c.want = rollout_returns(dyn, c.spec.evaluate, obs0, acts, n, DISCOUNT).reshape(m, n)
    c.want.setflags(write=False)
    c.native = NativeModel(obs_dim, act_dim, list(hidden), activation, None, E, mode)
    for e in range(E):
        c.native.set_weights(e, sets[e])
        c.native.set_norm(e, norms[e])
    c.inputs = (_up(obs0, c.native.device), _up(acts, c.native.device))
    return c


@functools.lru_cache(maxsize=2)
def _lstm_case(obs_dim, act_dim, units, activation, m, n, h, reward):
    key = (obs_dim, act_dim, units, activation, m, n, h)
    rs = np.random.RandomState(_seed("inputs", *key))
    low, high = -np.ones(act_dim), np.ones(act_dim)
    params = synthetic.make_lstm_set(obs_dim, act_dim, units, _seed("weights", *key))
    norm = synthetic.make_norm(obs_dim, act_dim, low, high, _seed("norm", *key))
    c = _Case()
    c.spec = _reward(reward, obs_dim)
    dyn = OracleLSTMDynamics(obs_dim, act_dim, params, norm, hidden_nonlinearity=activation)
    obs0 = rs.randn(m, obs_dim)
    hid = LSTMStateTuple(rs.randn(m, units).astype(np.float32), np.tanh(rs.randn(m, units)).astype(np.float32))
    acts = rs.uniform(low, high, (h, m * n, act_dim))
    c.want = rnn_rollout_returns(dyn, c.spec.evaluate, obs0, hid, acts, n, DISCOUNT).reshape(m, n)
    c.want.setflags(write=False)
    c.native = NativeLSTM(obs_dim, act_dim, units, activation, None)
    c.native.set_weights(params)
    c.native.set_norm(norm)
    dev = c.native.device
    c.inputs = (_up(obs0, dev), _up(hid.c, dev), _up(hid.h, dev), _up(acts, dev))
    return c


def _set_policy(ctx, policy, kernel="auto"):
    ctx.set_split(policy["split"])
    ctx.set_fan(policy["fan"])
    ctx.set_micro(policy["micro"])
    ctx.set_double_rounds(policy["double"])
    ctx.set_kernel(kernel)


def _launch(ctx, case, row, policy, kernel="auto"):
    _set_policy(ctx, policy, kernel)
    dev = case.native.device
    rets = torch.full((row.m, row.n), float("nan"), dtype=torch.float32, device=dev)
    best = torch.zeros((row.m,), dtype=torch.int64, device=dev)
    case.native.plan_rs(*case.inputs, row.m, row.n, row.h, DISCOUNT, case.spec, cand_offset=OFFSET, returns_out=rets,
                        best_key=best)
    torch.cuda.synchronize()
    assert ctx.launch_status() == 0
    return rets.cpu().numpy(), best.cpu().numpy()


def _check(row, got, keys, want):
    assert np.all(np.isfinite(want)), "oracle returns of %s are not finite: lower the weight scale of this shape" % row.id
    assert np.all(np.isfinite(got))
    assert rel_err(got, want) < RTOL
    for i in range(got.shape[0]):
        ret, idx = _lib.key_decode(keys[i])
        assert idx - OFFSET == int(np.argmax(got[i])) and ret == got[i, idx - OFFSET]


@pytest.mark.parametrize("row", im.MLP_ROWS, ids=[r.id for r in im.MLP_ROWS])
def test_mlp_instance_matches_oracle(row):
    case = _mlp_case(row.obs_dim, row.act_dim, tuple(row.hidden), row.activation, row.E, row.mode, row.m, row.n, row.h, row.reward)
    ctx = _lib.Context.get(0)
    try:
        got, keys = _launch(ctx, case, row, row.policy)
        base, base_keys = _launch(ctx, case, row, BASELINE)
        valu = _launch(ctx, case, row, BASELINE, "valu") if row.valu else None
    finally:
        _set_policy(ctx, DEFAULTS)
    _check(row, got, keys, case.want)
    assert np.array_equal(got, base) and np.array_equal(keys, base_keys)
    if valu is not None:
        assert rel_err(got, valu[0]) < VALU_RTOL
        assert np.array_equal(keys & 0x7FFFFFFF, valu[1] & 0x7FFFFFFF)          # same winner


@pytest.mark.parametrize("row", im.LSTM_ROWS, ids=[r.id for r in im.LSTM_ROWS])
def test_lstm_instance_matches_oracle(row):
    case = _lstm_case(row.obs_dim, row.act_dim, row.hidden, row.activation, row.m, row.n, row.h, row.reward)
    ctx = _lib.Context.get(0)
    try:
        got, keys = _launch(ctx, case, row, row.policy)
        other, other_keys = _launch(ctx, case, row, dict(row.policy, micro=0, split=0 if row.policy["split"] else 1))
    finally:
        _set_policy(ctx, DEFAULTS)
    _check(row, got, keys, case.want)
    # SPLIT on against SPLIT off (a micro-tile row: against the unit-tile split)
    assert np.array_equal(got, other) and np.array_equal(keys, other_keys)
