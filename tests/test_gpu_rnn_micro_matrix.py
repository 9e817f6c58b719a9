"""Every body of the generic recurrent micro-tile kernel against the float64 oracle: one case per row of tests/rnn_micro_matrix.py.

`l2a_rnn_micro_k<UW, CELL, MTM>` (csrc/l2a_rnn_micro.h) has eight instances and 27 bodies `l2a_rnn_micro_body<MT, ...>`; the rows
put a model on the edges of the input shapes (odd KG0 padded with zero iterations, OT = 1 .. 4, actions in both slots, the
limits 64 / 16) and a plan on the deal that reaches each body (asserted without a GPU in tests/test_rnn_micro_matrix.py, and
again here at the device's own CU count).  Per row, under micro policy 2:

  * every candidate's return against `rnn_rollout_trace` on `OracleRNNStackDynamics(dtype=float64)` (`_tol_returns < 1e-4`),
    from non-zero hidden states that differ per env, with a discount of 0.97 and `cand_offset` != 0;
  * the published key decodes to the arg-max (first maximum) of the returns the kernel wrote and to that return bit for bit;
    a keys-only launch publishes the same keys;
  * `returns_out` lies in a sentinel-filled buffer with guard rows on both sides, pre-filled with NaN: guards untouched, no NaN left;
  * the same plan under micro policy 0 (`l2a_rnn_mfma_k`, pinned to the oracle by `instance_matrix.GENERIC_ROWS`) has the same
    arg-max and returns within 2e-6 of max(1, max |return|) (256 units) / 4e-6 (512 units: the two kernels differ in the output
    layer's summation order only, whose error grows at most linearly with the number of summed units);
  * micro policy 1 gives the bits of policy 2 wherever it takes micro tiles too (the launcher's geometry is asked).

`test_second_set_weights_refreshes_the_micro_pack`: one model per cell type and width gets a second `set_weights`; micro tiles and
the 16-candidate kernel must both follow the new weights (the micro-tile kernels read a packed copy of their own).
"""

import functools
import zlib

import numpy as np
import pytest
import torch

import rnn_micro_matrix as rm
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_lstm import NativeLSTM
from learning_to_adapt_amd.envs import RewardSpec
from learning_to_adapt_amd.utils import synthetic
from oracle import LSTMStateTuple, OracleRNNStackDynamics
from oracle.rnn_planner import rnn_rollout_trace
from test_rnn import _tol_returns

pytestmark = pytest.mark.gpu

OFFSET = 11
DISCOUNT = 0.97
RTOL = 1e-4                     # the project's bar for this kernel against the oracle (tests/test_rnn.py)
MARGIN = 1e-3                   # top-2 margin of the oracle's returns (tests/test_rnn_reward_paths_gpu.py): a condition on the inputs
PAIR_TOL = {256: 2e-6, 512: 4e-6}   # against the 16-candidate kernel, of max(1, max |return|)
GUARD = 3                       # rows of sentinel on each side of returns_out
SENTINEL = -7.25e5


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x3FFFFFFF


def _reward(kind, obs_dim):
    """Ten times the coefficients of tests/test_gpu_instance_matrix.py: with one action dim among up to 65 inputs and up to 129
    envs in a plan, the candidates' returns lie too close for every env's two best to be MARGIN apart at the smaller scale (the
    bars against the oracle and the 16-candidate kernel are relative, so the scale does not loosen them)."""
    if kind == "dist":          # the last three observation dims
        return RewardSpec.make(dist_coef=10.0, ctrl_coef=0.05, dist_index=obs_dim - 3)
    return RewardSpec.make(w_vel=10.0, dt=0.05, ctrl_coef=0.5, vel_index=obs_dim - 1)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


class _Case(object):
    pass


def _draw_hidden(row, rs):
    """Non-zero states, one per env: the oracle's structure and the launches' flat (c, h) rows (c = 0 for cells without one)."""
    layers, cs, hs = [], [], []
    for u in row.units:
        c, h = rs.randn(row.m, u).astype(np.float32), np.tanh(rs.randn(row.m, u)).astype(np.float32)
        layers.append(LSTMStateTuple(c, h) if row.cell == "lstm" else h)
        cs.append(c if row.cell == "lstm" else np.zeros_like(h))
        hs.append(h)
    return (layers if len(layers) > 1 else layers[0]), np.concatenate(cs, axis=1), np.concatenate(hs, axis=1)


def margin(returns):
    """The smallest gap between an env's two best returns."""
    top = np.sort(np.asarray(returns, dtype=np.float64), axis=1)
    return float(np.min(top[:, -1] - top[:, -2]))


def model_of(row, tag="weights"):
    params = synthetic.make_rnn_stack_set(row.obs_dim, row.act_dim, list(row.units), row.cell, _seed(tag, row.id))
    low, high = -np.ones(row.act_dim), np.ones(row.act_dim)
    norm = synthetic.make_norm(row.obs_dim, row.act_dim, low, high, _seed("norm", row.id))
    return params, norm


def oracle_returns(row, params, norm, inputs):
    dyn = OracleRNNStackDynamics(row.obs_dim, row.act_dim, row.units, row.cell, params, norm,
                                 hidden_nonlinearity=row.activation, dtype=np.float64)
    obs0, hid, acts = inputs
    want = rnn_rollout_trace(dyn, _reward(row.reward, row.obs_dim).evaluate, obs0, hid, acts, row.n, DISCOUNT)[0]
    return _frozen(want.reshape(row.m, row.n))


@functools.lru_cache(maxsize=2)
def oracle_case(row):
    """Model, inputs and the float64 returns of a row (no GPU involved; read-only).  Rows are plain tuples: two rows that are
    equal share the case."""
    rs = np.random.RandomState(_seed("inputs", row.id, row.salt))
    c = _Case()
    c.params, c.norm = model_of(row)
    c.spec = _reward(row.reward, row.obs_dim)
    obs0 = rs.randn(row.m, row.obs_dim)
    hid, c_flat, h_flat = _draw_hidden(row, rs)
    acts = rs.uniform(-1.0, 1.0, (row.h, row.m * row.n, row.act_dim))
    c.oracle_inputs = (obs0, hid, acts)
    c.host_inputs = (obs0, c_flat, h_flat, acts)
    c.want = oracle_returns(row, c.params, c.norm, c.oracle_inputs)
    return c


def _gpu_case(row):
    c = oracle_case(row)
    if not hasattr(c, "native"):
        c.native = NativeLSTM(row.obs_dim, row.act_dim, list(row.units), row.activation, None, cell_type=row.cell)
        c.native.set_weights(c.params)
        c.native.set_norm(c.norm)
        c.inputs = tuple(_up(a, c.native.device) for a in c.host_inputs)
    return c


class _Guarded(object):
    """[rows, width] inside a buffer with GUARD rows of SENTINEL on each side; the interior starts as NaN."""

    def __init__(self, rows, width, dev):
        self.full = torch.full((rows + 2 * GUARD, width), SENTINEL, dtype=torch.float32, device=dev)
        self.inner = self.full[GUARD:GUARD + rows]
        self.inner.fill_(float("nan"))
        assert self.inner.is_contiguous() and self.inner.data_ptr() == self.full.data_ptr() + 4 * GUARD * width

    def read(self):
        full = self.full.cpu().numpy()
        assert np.all(full[:GUARD] == np.float32(SENTINEL)) and np.all(full[-GUARD:] == np.float32(SENTINEL)), "guard rows overwritten"
        inner = full[GUARD:-GUARD]
        assert not np.any(np.isnan(inner)), "returns left unwritten: %s" % (np.argwhere(np.isnan(inner))[:8].tolist(),)
        return inner


def _launch(ctx, case, row, micro, returns=True):
    ctx.set_micro(micro)
    dev = case.native.device
    rets = _Guarded(row.m, row.n, dev) if returns else None
    best = torch.zeros((row.m,), dtype=torch.int64, device=dev)
    case.native.plan_rs(*case.inputs, row.m, row.n, row.h, DISCOUNT, case.spec, cand_offset=OFFSET,
                        returns_out=rets.inner if returns else None, best_key=best)
    torch.cuda.synchronize()
    ctx.launch_status()
    return (rets.read() if returns else None), best.cpu().numpy()


def _geometry(row, micro, cus):
    return _lib.lstm_plan_geometry(row.obs_dim, row.act_dim, list(row.units), row.cell, row.m, row.n, row.h, micro=micro, cus=cus)


def _check_routing(row, cus, mtm, mts):
    g = _geometry(row, 2, cus)
    assert g["family"] == "generic_micro" and g["mtm"] == mtm and rm.workgroup_sizes(g) == set(mts), \
        "%s: on this device (%d compute units; the rows are laid out for 256) the launcher deals %s, not workgroups of %s micro " \
        "tiles on the mtm = %d instance" % (row.id, cus, g, sorted(mts), mtm)


def _check_key(got, keys):
    for i in range(got.shape[0]):
        ret, idx = _lib.key_decode(keys[i])
        assert idx - OFFSET == int(np.argmax(got[i])) and ret == got[i, idx - OFFSET], i


def _pair_err(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b)) / max(1.0, float(np.max(np.abs(b)))))


@pytest.mark.parametrize("row", rm.ROWS, ids=[r.id for r in rm.ROWS])
def test_rnn_micro_body_matches_oracle(row):
    case = _gpu_case(row)
    ctx = _lib.Context.get(0)
    cus = ctx.info()["compute_units"]
    _check_routing(row, cus, row.instance.mtm, row.mts)
    policy1_is_micro = _geometry(row, 1, cus)["family"] == "generic_micro"
    try:
        got, keys = _launch(ctx, case, row, 2)
        _, keys_only = _launch(ctx, case, row, 2, returns=False)
        base, base_keys = _launch(ctx, case, row, 0)
        auto = _launch(ctx, case, row, 1) if policy1_is_micro else None
    finally:
        ctx.set_micro(1)
    want = case.want
    assert np.all(np.isfinite(want)) and margin(want) >= MARGIN, row.id         # (also in test_rnn_micro_matrix.py, without a GPU)
    err, pair = _tol_returns(got, want), _pair_err(got, base)
    print("%s: micro tiles against the oracle %.3e, the 16-candidate kernel against the oracle %.3e, micro tiles against the "
          "16-candidate kernel %.3e" % (row.id, err, _tol_returns(base, want), pair))
    assert np.all(np.isfinite(got)) and err < RTOL
    _check_key(got, keys)
    assert np.array_equal(keys, keys_only)
    for i in range(row.m):      # the oracle's winner (separated by MARGIN) is the kernel's
        assert _lib.key_decode(keys[i])[1] - OFFSET == int(np.argmax(want[i])), i
    # the 16-candidate kernel: same arg-max, returns a few ulps of the largest return apart
    _check_key(base, base_keys)
    assert np.array_equal(np.argmax(got, axis=1), np.argmax(base, axis=1))
    assert pair < PAIR_TOL[row.units[0]]
    if auto is not None:
        assert np.array_equal(auto[0], got) and np.array_equal(auto[1], keys)


@pytest.mark.parametrize("row", rm.REFRESH_ROWS, ids=[r.id for r in rm.REFRESH_ROWS])
def test_second_set_weights_refreshes_the_micro_pack(row):
    """`set_weights` packs a third copy of the weights for this kernel (`layer_mk`, `pk_mo`: l2a_rnn_micro_pack_k,
    l2a_lstm_micro_pack_out_k).  After a second `set_weights` both kernels must compute the NEW model."""
    old = _gpu_case(row)
    ctx = _lib.Context.get(0)
    _check_routing(row, ctx.info()["compute_units"], 3, (1,))
    new_params, _ = model_of(row, "second weights")
    want = oracle_returns(row, new_params, old.norm, old.oracle_inputs)
    assert np.all(np.isfinite(want)) and margin(want) >= MARGIN
    try:
        before, _ = _launch(ctx, old, row, 2)
        old.native.set_weights(new_params)
        try:
            got, keys = _launch(ctx, old, row, 2)
            base, base_keys = _launch(ctx, old, row, 0)
        finally:
            old.native.set_weights(old.params)          # the case is shared: leave it as it was built
    finally:
        ctx.set_micro(1)
    err, pair = _tol_returns(got, want), _pair_err(got, base)
    print("%s: after the second set_weights, micro tiles against the oracle %.3e, 16-candidate kernel %.3e, between them %.3e; "
          "against the old weights' returns %.3e" % (row.id, err, _tol_returns(base, want), pair, _tol_returns(got, before)))
    assert _tol_returns(before, old.want) < RTOL
    assert err < RTOL and _tol_returns(base, want) < RTOL
    _check_key(got, keys)
    _check_key(base, base_keys)
    assert np.array_equal(np.argmax(got, axis=1), np.argmax(base, axis=1))
    assert pair < PAIR_TOL[row.units[0]]
    # not vacuous: the new model's returns are far from the old one's (a stale pack would reproduce `before`)
    assert _tol_returns(got, before) > 100 * RTOL and _tol_returns(want, old.want) > 100 * RTOL
