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

Rows that differ in policy alone share their model, inputs and oracle trace (`_mlp_case`, `_lstm_case`: read-only).

The CARRY of every row that has one (the micro-tile kernels are never launched with one: `plan_rollout` in l2a_api.hip and
`plan_rnn_launch` in l2a_lstm_api.hip keep every launch with per-row states or a state output off them) - what a launch hands to the next one: `state_out` (LSTM: `c_out`, `h_out`) written, per-row
observations / hidden states, `returns_in` and the discount power read.  In the same test, while the row's case is warm, under
the row's policy with micro = 0 and again under BASELINE:

  * chunk A = horizon step 0 from the shared observations, chunk B = steps 1 and 2 from what A wrote; B's returns and keys
    equal the single launch bit for bit, the states A and B wrote match the oracle's trace after steps 1 and 3 (`rel_err < RTOL`);
  * one `l2a_predict` / `l2a_lstm_predict` of m * n rows with observations, actions and hidden states drawn per row, against
    `dyn.predict` (the bars of test_predict_matches_oracle / test_gpu_rnn_predict_matches_oracle);
  * every output equals BASELINE's bit for bit; every state output lies in a sentinel-filled buffer with 16 guard rows on
    each side, pre-filled with NaN: the guards are untouched, no NaN is left.

`test_generic_recurrent_branches_match_oracle`: the same four launches on the generic recurrent kernels (matrix-core and VALU),
one row of `instance_matrix.GENERIC_ROWS` per run-time branch of l2a_rnn_mfma.h, against `OracleRNNStackDynamics` in float64.

LSTM: test_instance_matrix.py asks the launcher's plan function (`plan_rnn_launch`, through `l2a_lstm_plan_geometry`) that every
row reaches its instance, and restates its conditions arithmetically: with micro policy 0 no plan takes micro tiles
(`lstm_micro_wanted`); the unit-tile split is taken iff the split policy is non-zero and 2 x tiles <= CUs and h < 4096 - n = 37,
m = 1 is three tiles; with micro policy 2 a plan of at most three micro tiles per workgroup on 256 / 512 units takes the micro-tile
kernel (the generic stacks' branch is not involved: `rnn_shape` makes a single eligible LSTM layer the tuned model, not a
`generic` one).  SPLIT on and SPLIT off must agree bit for bit.
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
from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
from oracle import LSTMStateTuple, OracleLSTMDynamics, OracleMLPDynamics, OracleRNNStackDynamics
from oracle.planner import rollout_trace
from oracle.rnn_planner import rnn_rollout_trace
from test_gpu_parity import RTOL, rel_err
from test_rnn import _tol_returns

pytestmark = pytest.mark.gpu

OFFSET = 7
DISCOUNT = 0.9
VALU_RTOL = 2e-5                # test_gpu_parity.test_mfma_and_valu_kernels_agree
BASELINE = dict(split=0, fan=0, micro=0, double=0)
DEFAULTS = dict(split=1, fan=1, micro=1, double=1)
GUARD = 16                      # rows of sentinel on each side of every state output
SENTINEL = -7.25e5
PREDICT_TOL = dict(rtol=2e-5, atol=2e-5)            # test_gpu_parity.test_predict_matches_oracle
LSTM_PREDICT_TOL = dict(rtol=1e-5, atol=1e-5)       # test_rnn.test_gpu_rnn_predict_matches_oracle: observations ...
LSTM_STATE_TOL = dict(rtol=1e-5, atol=2e-6)         # ... and c / h


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


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def has_carry(row):
    """The micro-tile kernels are never given a carry launch (`plan_rollout`, `plan_rnn_launch`: plans only)."""
    return row.instance.family in ("mlp", "lstm")


class _Guarded(object):
    """[rows, width] inside a buffer with GUARD rows of SENTINEL on each side; the interior starts as NaN."""

    def __init__(self, rows, width, dev):
        self.full = torch.full((rows + 2 * GUARD, width), SENTINEL, dtype=torch.float32, device=dev)
        self.inner = self.full[GUARD:GUARD + rows]
        self.inner.fill_(float("nan"))
        assert self.inner.is_contiguous() and self.inner.data_ptr() == self.full.data_ptr() + 4 * GUARD * width

    def read(self):
        """The interior as a NumPy array, once the guards are seen untouched and no NaN is left inside."""
        full = self.full.cpu().numpy()
        assert np.all(full[:GUARD] == np.float32(SENTINEL)) and np.all(full[-GUARD:] == np.float32(SENTINEL)), "guard rows overwritten"
        inner = full[GUARD:-GUARD]
        assert not np.any(np.isnan(inner)), "rows left unwritten: %s" % np.unique(np.nonzero(np.isnan(inner))[0])[:8]
        return inner


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
    want, states = rollout_trace(dyn, c.spec.evaluate, obs0, acts, n, DISCOUNT)
    c.want, c.states = _frozen(want.reshape(m, n)), _frozen(states)
    c.native = NativeModel(obs_dim, act_dim, list(hidden), activation, None, E, mode)
    for e in range(E):
        c.native.set_weights(e, sets[e])
        c.native.set_norm(e, norms[e])
    c.inputs = (_up(obs0, c.native.device), _up(acts, c.native.device))
    # predict: every row its own observation and action (step 0 of the plan reads one observation per env)
    c.pred_rows = (rs.randn(m * n, obs_dim), rs.uniform(low, high, (m * n, act_dim)))
    c.pred_inputs = tuple(_up(a, c.native.device) for a in c.pred_rows)
    c.pred_want = functools.lru_cache(maxsize=1)(lambda: _frozen(dyn.predict(*c.pred_rows)))      # once per case, on first use
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
    want, states, hiddens = rnn_rollout_trace(dyn, c.spec.evaluate, obs0, hid, acts, n, DISCOUNT)
    c.want, c.states = _frozen(want.reshape(m, n)), _frozen(states)
    c.cells = [(_frozen(hd.c), _frozen(hd.h)) for hd in hiddens]
    c.native = NativeLSTM(obs_dim, act_dim, units, activation, None)
    c.native.set_weights(params)
    c.native.set_norm(norm)
    dev = c.native.device
    c.inputs = (_up(obs0, dev), _up(hid.c, dev), _up(hid.h, dev), _up(acts, dev))
    # predict: every row its own observation, action and state
    c.pred_rows = (rs.randn(m * n, obs_dim), rs.uniform(low, high, (m * n, act_dim)),
                   rs.randn(m * n, units).astype(np.float32), np.tanh(rs.randn(m * n, units)).astype(np.float32))
    c.pred_inputs = tuple(_up(a, dev) for a in c.pred_rows)

    @functools.lru_cache(maxsize=1)
    def pred_want():        # once per case, on first use
        nxt, hd = dyn.predict(c.pred_rows[0], c.pred_rows[1], LSTMStateTuple(c.pred_rows[2], c.pred_rows[3]))
        return _frozen(nxt), _frozen(hd.c), _frozen(hd.h)
    c.pred_want = pred_want
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


def _mlp_carry(ctx, case, row, policy, kernel="auto"):
    """Chunk A (step 0), chunk B (steps 1, 2: from what A wrote) and one predict of per-row inputs under `policy`."""
    _set_policy(ctx, policy, kernel)
    native, dev = case.native, case.native.device
    obs0, acts = case.inputs
    m, n, od = row.m, row.n, row.obs_dim
    rets = [torch.full((m, n), float("nan"), dtype=torch.float32, device=dev) for _ in (0, 1)]
    st = [_Guarded(m * n, od, dev) for _ in (0, 1)]
    best = torch.zeros((m,), dtype=torch.int64, device=dev)
    native.plan_rs_chunk(obs0, False, acts[0:1].contiguous(), m, n, 1, 0, DISCOUNT, case.spec, cand_offset=OFFSET,
                         returns_out=rets[0], state_out=st[0].inner)
    native.plan_rs_chunk(st[0].inner, True, acts[1:row.h].contiguous(), m, n, row.h - 1, 1, DISCOUNT, case.spec,
                         cand_offset=OFFSET, returns_in=rets[0], returns_out=rets[1], state_out=st[1].inner, best_key=best)
    pred = _Guarded(m * n, od, dev)
    native.predict(case.pred_inputs[0], case.pred_inputs[1], n_blocks=m, out=pred.inner)
    torch.cuda.synchronize()
    assert ctx.launch_status() == 0
    return dict(returns=rets[1].cpu().numpy(), keys=best.cpu().numpy(), state_a=st[0].read(), state_b=st[1].read(),
                predict=pred.read())


def _lstm_carry(ctx, case, row, policy, kernel="auto"):
    _set_policy(ctx, policy, kernel)
    native, dev = case.native, case.native.device
    obs0, c0, h0, acts = case.inputs
    m, n, od, U = row.m, row.n, row.obs_dim, native.units
    rets = [torch.full((m, n), float("nan"), dtype=torch.float32, device=dev) for _ in (0, 1)]
    st, cs, hs = [[_Guarded(m * n, w, dev) for _ in (0, 1)] for w in (od, U, U)]
    best = torch.zeros((m,), dtype=torch.int64, device=dev)
    native.plan_rs_chunk(obs0, c0, h0, False, acts[0:1].contiguous(), m, n, 1, 0, DISCOUNT, case.spec, cand_offset=OFFSET,
                         returns_out=rets[0], state_out=st[0].inner, c_out=cs[0].inner, h_out=hs[0].inner)
    native.plan_rs_chunk(st[0].inner, cs[0].inner, hs[0].inner, True, acts[1:row.h].contiguous(), m, n, row.h - 1, 1, DISCOUNT,
                         case.spec, cand_offset=OFFSET, returns_in=rets[0], returns_out=rets[1], state_out=st[1].inner,
                         c_out=cs[1].inner, h_out=hs[1].inner, best_key=best)
    pred = [_Guarded(m * n, w, dev) for w in (od, U, U)]
    rc = native.lib.l2a_lstm_predict(native.handle, *[_ptr(t) for t in case.pred_inputs], m * n,
                                     *[_ptr(g.inner) for g in pred], _stream_ptr(dev))
    ctx.check(rc, "l2a_lstm_predict")
    torch.cuda.synchronize()
    assert ctx.launch_status() == 0
    out = dict(returns=rets[1].cpu().numpy(), keys=best.cpu().numpy())
    for k in (0, 1):
        out.update({"state_" + "ab"[k]: st[k].read(), "c_" + "ab"[k]: cs[k].read(), "h_" + "ab"[k]: hs[k].read()})
    out.update(predict=pred[0].read(), predict_c=pred[1].read(), predict_h=pred[2].read())
    return out


def _print_err(row, name, got, want):
    """The measured figure in front of its assertion (pytest shows it for a failing test, -s for all)."""
    print("%s %s: rel_err %.3e" % (row.id, name, rel_err(got, want)))


def _check_chain(row, carry, base, got, keys):
    assert np.array_equal(carry["returns"], got) and np.array_equal(carry["keys"], keys), "chunk chain differs from the single launch"
    assert sorted(carry) == sorted(base)
    for name in carry:      # include/l2a.h: the policies change the launch geometry only
        assert np.array_equal(carry[name], base[name]), "%s under the row's policy differs from the baseline geometry" % name


def _check_states(row, carry, names, wants):
    for name, want in zip(names, wants):
        assert np.all(np.isfinite(want)), "oracle %s of %s is not finite: lower the weight scale of this shape" % (name, row.id)
        _print_err(row, name, carry[name], want)
        assert rel_err(carry[name], want) < RTOL, name


@pytest.mark.parametrize("row", im.MLP_ROWS, ids=[r.id for r in im.MLP_ROWS])
def test_mlp_instance_matches_oracle(row):
    case = _mlp_case(row.obs_dim, row.act_dim, tuple(row.hidden), row.activation, row.E, row.mode, row.m, row.n, row.h, row.reward)
    ctx = _lib.Context.get(0)
    carry = base_carry = None
    try:
        got, keys = _launch(ctx, case, row, row.policy)
        base, base_keys = _launch(ctx, case, row, BASELINE)
        valu = _launch(ctx, case, row, BASELINE, "valu") if row.valu else None
        if has_carry(row):
            carry = _mlp_carry(ctx, case, row, dict(row.policy, micro=0))
            base_carry = _mlp_carry(ctx, case, row, BASELINE)
    finally:
        _set_policy(ctx, DEFAULTS)
    _check(row, got, keys, case.want)
    assert np.array_equal(got, base) and np.array_equal(keys, base_keys)
    if valu is not None:
        assert rel_err(got, valu[0]) < VALU_RTOL
        assert np.array_equal(keys & 0x7FFFFFFF, valu[1] & 0x7FFFFFFF)          # same winner
    if has_carry(row):
        _check_chain(row, carry, base_carry, got, keys)
        _check_states(row, carry, ("state_a", "state_b"), (case.states[0], case.states[row.h - 1]))
        np.testing.assert_allclose(carry["predict"].astype(np.float64), case.pred_want(), **PREDICT_TOL)


@pytest.mark.parametrize("row", im.LSTM_ROWS, ids=[r.id for r in im.LSTM_ROWS])
def test_lstm_instance_matches_oracle(row):
    case = _lstm_case(row.obs_dim, row.act_dim, row.hidden, row.activation, row.m, row.n, row.h, row.reward)
    ctx = _lib.Context.get(0)
    carry = base_carry = None
    try:
        got, keys = _launch(ctx, case, row, row.policy)
        other, other_keys = _launch(ctx, case, row, dict(row.policy, micro=0, split=0 if row.policy["split"] else 1))
        if has_carry(row):
            carry = _lstm_carry(ctx, case, row, dict(row.policy, micro=0))
            base_carry = _lstm_carry(ctx, case, row, BASELINE)
    finally:
        _set_policy(ctx, DEFAULTS)
    _check(row, got, keys, case.want)
    # SPLIT on against SPLIT off (a micro-tile row: against the unit-tile split)
    assert np.array_equal(got, other) and np.array_equal(keys, other_keys)
    if has_carry(row):
        last = row.h - 1
        _check_chain(row, carry, base_carry, got, keys)
        _check_states(row, carry, ("state_a", "c_a", "h_a", "state_b", "c_b", "h_b"),
                      (case.states[0],) + case.cells[0] + (case.states[last],) + case.cells[last])
        nxt, c1, h1 = case.pred_want()
        np.testing.assert_allclose(carry["predict"].astype(np.float64), nxt, **LSTM_PREDICT_TOL)
        np.testing.assert_allclose(carry["predict_c"], c1, **LSTM_STATE_TOL)
        np.testing.assert_allclose(carry["predict_h"], h1, **LSTM_STATE_TOL)


# ---- the generic recurrent kernels: one row per run-time branch ------------------------------------------------------------------

def _flat_hidden(row, hidden):
    """A hidden state as the oracle structures it -> the (c, h) rows the launches take: the layers' states side by side,
    c = 0 for the cells that have none."""
    layers = list(hidden) if len(row.units) > 1 else [hidden]
    if row.cell == "lstm":
        return np.concatenate([l.c for l in layers], axis=1), np.concatenate([l.h for l in layers], axis=1)
    h = np.concatenate(layers, axis=1)
    return np.zeros_like(h), h


def _draw_hidden(row, rs, rows):
    layers = []
    for u in row.units:
        c, h = rs.randn(rows, u).astype(np.float32), np.tanh(rs.randn(rows, u)).astype(np.float32)
        layers.append(LSTMStateTuple(c, h) if row.cell == "lstm" else h)
    return layers if len(layers) > 1 else layers[0]


@functools.lru_cache(maxsize=1)
def _generic_oracle(row):
    """Model, inputs and the float64 trace of a GENERIC_ROWS entry (no GPU involved; read-only)."""
    m, n, h = im.GENERIC_M, im.GENERIC_N, im.H
    rs = np.random.RandomState(_seed("inputs", row.id))
    low, high = -np.ones(row.act_dim), np.ones(row.act_dim)
    c = _Case()
    c.params = synthetic.make_rnn_stack_set(row.obs_dim, row.act_dim, list(row.units), row.cell, _seed("weights", row.id))
    c.norm = synthetic.make_norm(row.obs_dim, row.act_dim, low, high, _seed("norm", row.id))
    c.spec = _reward(row.reward, row.obs_dim)
    dyn = OracleRNNStackDynamics(row.obs_dim, row.act_dim, row.units, row.cell, c.params, c.norm,
                                 hidden_nonlinearity=row.activation, dtype=np.float64)
    obs0 = rs.randn(m, row.obs_dim)
    hid = _draw_hidden(row, rs, m)
    acts = rs.uniform(low, high, (h, m * n, row.act_dim))
    want, states, hiddens = rnn_rollout_trace(dyn, c.spec.evaluate, obs0, hid, acts, n, DISCOUNT)
    c.want, c.states = _frozen(want.reshape(m, n)), _frozen(states)
    c.cells = [tuple(_frozen(a) for a in _flat_hidden(row, hd)) for hd in hiddens]
    pobs, pact, phid = rs.randn(m * n, row.obs_dim), rs.uniform(low, high, (m * n, row.act_dim)), _draw_hidden(row, rs, m * n)
    nxt, hd = dyn.predict(pobs, pact, phid)
    c.pred_want = (_frozen(nxt),) + tuple(_frozen(a) for a in _flat_hidden(row, hd))
    c.host_inputs = (obs0,) + _flat_hidden(row, hid) + (acts,)
    c.host_pred_inputs = (pobs, pact) + _flat_hidden(row, phid)
    return c


def _generic_case(row):
    c = _generic_oracle(row)
    if not hasattr(c, "native"):
        c.native = NativeLSTM(row.obs_dim, row.act_dim, list(row.units), row.activation, None, cell_type=row.cell)
        c.native.set_weights(c.params)
        c.native.set_norm(c.norm)
        c.inputs = tuple(_up(a, c.native.device) for a in c.host_inputs)
        c.pred_inputs = tuple(_up(a, c.native.device) for a in c.host_pred_inputs)
    return c


@pytest.mark.parametrize("kernel", ["mfma", "valu"])
@pytest.mark.parametrize("row", im.GENERIC_ROWS, ids=[r.id for r in im.GENERIC_ROWS])
def test_generic_recurrent_branches_match_oracle(row, kernel):
    """`l2a_rnn_mfma_k` ("mfma") and `l2a_rnn_valu_k` ("valu") on one model per run-time branch: the plan, its chunk chain
    and a predict of per-row inputs against `OracleRNNStackDynamics` in float64 (m = 2, n = 37, h = 3, non-zero states)."""
    case = _generic_case(row)
    plan = im.Row(row.id, None, row.obs_dim, row.act_dim, None, row.activation, 1, "single", im.GENERIC_M, im.GENERIC_N, im.H,
                  BASELINE, None, row.reward, False)
    ctx = _lib.Context.get(0)
    try:
        got, keys = _launch(ctx, case, plan, BASELINE, kernel)
        carry = _lstm_carry(ctx, case, plan, BASELINE, kernel)
    finally:
        _set_policy(ctx, DEFAULTS)
    assert np.all(np.isfinite(case.want)), "oracle returns of %s are not finite: lower the weight scale of this shape" % row.id
    print("%s %s returns: %.3e" % (row.id, kernel, _tol_returns(got, case.want)))
    assert np.all(np.isfinite(got)) and _tol_returns(got, case.want) < 1e-4
    for i in range(got.shape[0]):
        ret, idx = _lib.key_decode(keys[i])
        assert idx - OFFSET == int(np.argmax(got[i])) and ret == got[i, idx - OFFSET]
    assert np.array_equal(carry["returns"], got) and np.array_equal(carry["keys"], keys), "chunk chain differs from the single launch"
    last = im.H - 1
    _check_states(plan, carry, ("state_a", "c_a", "h_a", "state_b", "c_b", "h_b", "predict", "predict_c", "predict_h"),
                  (case.states[0],) + case.cells[0] + (case.states[last],) + case.cells[last] + case.pred_want)
    if row.cell != "lstm":      # these cells have no c: the launches write zeros
        assert not carry["c_a"].any() and not carry["c_b"].any() and not carry["predict_c"].any()
