"""Every row of tests/adapt_matrix.py on the GPU: one GrBAL adaptation step (csrc/l2a_adapt.h) through the row's entry point into
a per-block model whose sets all hold distinct sentinel models, then

* sets 0 .. m-1 against the float64 autograd step, per tensor |got - want| <= 3e-5 max(step, 1e-3) + 2e-7 (the bar of
  tests/test_gpu_random_shapes.py; the worst error / bar of each row is printed and recorded in DESIGN.md 7);
* sets m .. n_sets-1 bit-equal to their sentinels; the base tensors and the batches unchanged;
* `host` / `raw` rows bit-equal to the `device` entry on the inputs normalised on the host (float64, then the cast), the caller's
  arrays overwritten right after the call returns;
* misaligned rows within 2 bars of the aligned run of the same model (the fallbacks sum in another order: not bit-equal);
* rows whose model the matrix-core planner takes: a second model loaded with the adapted raw tensors through `set_weights` plans
  bit for bit like the adapted one (returns and keys, 16-candidate and micro-tile kernel) - the packed copies the update wrote
  against the library's own packer; every other row: `l2a_predict` of the adapted sets against the float64-adapted oracle.

The reference of a row is computed once (adapt_matrix.reference) and never written to."""

import ctypes

import numpy as np
import pytest
import torch

import adapt_matrix as am
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativeModel, _stream_ptr
from learning_to_adapt_amd.envs import RewardSpec
from learning_to_adapt_amd.utils import synthetic
from oracle import OracleMLPDynamics

pytestmark = pytest.mark.gpu

PLAN_N, PLAN_H = 37, 3
PREDICT_ROWS, PREDICT_TOL = 24, 2e-4        # per set; the bar of test_adapt_oracle.test_device_adapt_matches_oracle


def _dev():
    return torch.device("cuda:0")


def _base_tensors(base_np, aligned):
    """The base parameters on the device.  Misaligned: each a contiguous view ONE FLOAT into a larger buffer."""
    out = []
    for w in base_np:
        w = np.ascontiguousarray(w, dtype=np.float32)
        if aligned:
            t = torch.from_numpy(w).to(_dev())
            assert t.data_ptr() % 16 == 0
        else:
            buf = torch.zeros((w.size + 8,), dtype=torch.float32, device=_dev())
            t = buf[1:1 + w.size].view(w.shape)
            t.copy_(torch.from_numpy(w))
            assert t.is_contiguous() and t.data_ptr() % 16 == 4
        out.append(t)
    return out


def _model(row, sentinels=True):
    nm = NativeModel(row.od, row.ad, row.hidden, row.act, None, row.n_sets, "per_block")
    if sentinels:
        for e in range(row.n_sets):
            nm.set_weights(e, am.sentinel(row, e))
    return nm


def _step(nm, row, base, inp, entry):
    """One step through `entry`; the caller's host arrays are overwritten as soon as the call returns.  -> the device batches
    (device entry) for the unchanged check."""
    if entry == "device":
        x, y = torch.from_numpy(inp["x"]).to(_dev()), torch.from_numpy(inp["y"]).to(_dev())
        nm.adapt_sgd(base, x, y, row.lr)
        return x, y
    if entry == "host":
        x, y = inp["x"].copy(), inp["y"].copy()
        nm.adapt_sgd_host(base, x, y, row.lr)
        x[:] = 7.0
        y[:] = -7.0
        return None
    ob, ac, nx = inp["obs"].copy(), inp["act"].copy(), inp["obs_next"].copy()
    norm = {k: (v[0].copy(), v[1].copy()) for k, v in inp["norm"].items()}
    nm.adapt_sgd_raw(base, ob, ac, nx, norm, row.lr)
    for a in (ob, ac, nx) + tuple(v for pair in norm.values() for v in pair):
        a[:] = 3.0
    return None


def _sets(nm, lo, hi):
    torch.cuda.synchronize()
    return [[w.cpu().numpy() for w in nm.get_weights(e)] for e in range(lo, hi)]


def _judge(row, got, ref, scale=1.0):
    """Worst |got - want| / bar over tasks and tensors; asserts every one is within `scale` bars."""
    worst = 0.0
    for e in range(row.m):
        want, steps = ref[e]
        for pi, (g, w, s) in enumerate(zip(got[e], want, steps)):
            assert g.shape == w.shape and g.dtype == np.float32
            err, b = float(np.abs(g.astype(np.float64) - w).max()), am.bar(float(np.abs(s).max()))
            worst = max(worst, err / b)
            assert err <= scale * b, (row.name, e, pi, g.shape, err, b)
    return worst


def _sentinels_intact(nm, row, lo):
    for e, got in zip(range(lo, row.n_sets), _sets(nm, lo, row.n_sets)):
        for pi, (g, w) in enumerate(zip(got, am.sentinel(row, e))):
            assert np.array_equal(g, w), (row.name, "set %d tensor %d was written" % (e, pi))


def _plans_like_its_packed_twin(row, adapted):
    """The three copies the update wrote (reference layout, MFMA fragment order, micro-tile order) against the library's packer."""
    packed = NativeModel(row.od, row.ad, row.hidden, row.act, None, row.m, "per_block")
    low, high = -np.ones(row.ad), np.ones(row.ad)
    norm = synthetic.make_norm(row.od, row.ad, low, high, 4242)
    for e in range(row.m):
        packed.set_weights(e, adapted.get_weights(e))
        adapted.set_norm(e, norm)
        packed.set_norm(e, norm)
    spec = RewardSpec.make(w_vel=1.0, dt=0.02, alive=0.05, vel_index=row.od - 1)
    rs = np.random.RandomState(11)
    obs0 = torch.from_numpy(rs.randn(row.m, row.od).astype(np.float32)).to(_dev())
    acts = torch.from_numpy(rs.uniform(low, high, (PLAN_H, row.m * PLAN_N, row.ad)).astype(np.float32)).to(_dev())
    ctx = _lib.Context.get(0)
    try:
        for micro in (0, 2):
            ctx.set_micro(micro)
            outs = []
            for nm in (adapted, packed):
                rets = torch.empty((row.m, PLAN_N), dtype=torch.float32, device=_dev())
                best = torch.zeros((row.m,), dtype=torch.int64, device=_dev())
                nm.plan_rs(obs0, acts, row.m, PLAN_N, PLAN_H, 0.97, spec, returns_out=rets, best_key=best)
                torch.cuda.synchronize()
                ctx.launch_status()
                outs.append((rets.cpu().numpy(), best.cpu().numpy()))
            assert np.all(np.isfinite(outs[0][0]))
            assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), (row.name, micro)
    finally:
        ctx.set_micro(1)
        packed.close()


def _predicts_like_the_oracle(row, adapted, ref):
    low, high = -np.ones(row.ad), np.ones(row.ad)
    norm = synthetic.make_norm(row.od, row.ad, low, high, 4242)
    for e in range(row.m):
        adapted.set_norm(e, norm)
    dyn = OracleMLPDynamics(row.od, row.ad, [[np.asarray(q, dtype=np.float32) for q in ref[e][0]] for e in range(row.m)], norm,
                            mode="per_block", hidden_nonlinearity=row.act)
    rs = np.random.RandomState(9)
    obs = rs.randn(row.m * PREDICT_ROWS, row.od)
    act = rs.uniform(low, high, (row.m * PREDICT_ROWS, row.ad))
    got = adapted.predict(torch.from_numpy(obs.astype(np.float32)).to(_dev()), torch.from_numpy(act.astype(np.float32)).to(_dev()),
                          n_blocks=row.m)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got.cpu().numpy(), dyn.predict(obs.astype(np.float32), act.astype(np.float32)),
                               rtol=PREDICT_TOL, atol=PREDICT_TOL)


@pytest.mark.parametrize("row", am.ROWS, ids=[r.name for r in am.ROWS])
def test_row_matches_the_float64_step(row):
    inp, ref = am.inputs(row), am.reference(row.name)
    base = _base_tensors(inp["base"], row.aligned)
    keep = [t.clone() for t in base]
    nm = _model(row)
    batches = _step(nm, row, base, inp, row.entry)
    got = _sets(nm, 0, row.m)
    worst = _judge(row, got, ref)
    print("ADAPT-MATRIX %s worst error / bar %.4f" % (row.name, worst))
    _sentinels_intact(nm, row, row.m)
    for t, k in zip(base, keep):
        assert torch.equal(t, k), (row.name, "a base tensor was written")
    if batches is not None:
        assert np.array_equal(batches[0].cpu().numpy(), inp["x"]) and np.array_equal(batches[1].cpu().numpy(), inp["y"])
    if row.entry != "device" or not row.aligned:
        twin = _model(row, sentinels=False)
        _step(twin, row, base if row.aligned else _base_tensors(inp["base"], True), inp, "device")
        other = _sets(twin, 0, row.m)
        twin.close()
        for e in range(row.m):
            for pi, (a, b) in enumerate(zip(got[e], other[e])):
                if row.aligned:     # another entry point, the same arithmetic
                    assert np.array_equal(a, b), (row.name, row.entry, e, pi)
                else:               # another summation order
                    two_bars = 2.0 * am.bar(float(np.abs(ref[e][1][pi]).max()))
                    assert float(np.abs(a.astype(np.float64) - b).max()) <= two_bars, (row.name, e, pi)
    if am.mfma_eligible(row.od, row.ad, row.hidden):
        _plans_like_its_packed_twin(row, nm)
    else:
        _predicts_like_the_oracle(row, nm, ref)
    nm.close()


@pytest.mark.parametrize("name", am.TWICE)
def test_second_step_depends_on_the_base_alone(name):
    """Two consecutive steps with different batches: the second result is the single step of its own batch, bit for bit - the
    step reads the base, never the sets (or the scratch) the first one left."""
    row = am.BY_NAME[name]
    first, second, ref = am.inputs(row, salt=1), am.inputs(row), am.reference(name)
    assert not np.array_equal(first["x"], second["x"])
    base = _base_tensors(second["base"], row.aligned)
    nm, once = _model(row), _model(row)
    _step(nm, row, base, first, row.entry)
    after_first = _sets(nm, 0, row.m)
    _step(nm, row, base, second, row.entry)
    _step(once, row, base, second, row.entry)
    got, want = _sets(nm, 0, row.m), _sets(once, 0, row.m)
    _judge(row, got, ref)
    for e in range(row.m):
        for a, b, c in zip(got[e], want[e], after_first[e]):
            assert np.array_equal(a, b) and not np.array_equal(a, c)
    _sentinels_intact(nm, row, row.m)
    nm.close()
    once.close()


def test_refusals_leave_every_set_alone():
    """rows 0 and 17, m 0 and n_sets + 1, swish, a non-identity output layer, a null base pointer, the raw entry at 129 inputs:
    L2A_EINVAL each, and every set still holds its sentinel."""
    row = am.BY_NAME["in4-h8"]
    inp = am.inputs(row)
    lib = _lib.load()
    stream = _stream_ptr(_dev())

    def ptrs(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])

    def batches(r, m, rows):
        x = torch.zeros((max(m, 1), max(rows, 1), r.od + r.ad), dtype=torch.float32, device=_dev())
        y = torch.zeros((max(m, 1), max(rows, 1), r.od), dtype=torch.float32, device=_dev())
        return x, y

    base = _base_tensors(inp["base"], True)
    nm = _model(row)
    for m, rows in ((1, 0), (1, 17), (0, 4), (row.n_sets + 1, 4)):
        x, y = batches(row, m, rows)
        rc = lib.l2a_model_adapt_sgd(nm.handle, ptrs(base), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), m, rows,
                                     ctypes.c_float(0.1), stream)
        assert rc == _lib.L2A_EINVAL, (m, rows, rc)
        xh, yh = np.zeros(tuple(x.shape), np.float32), np.zeros(tuple(y.shape), np.float32)
        rc = lib.l2a_model_adapt_sgd_host(nm.handle, ptrs(base), ctypes.c_void_p(xh.ctypes.data), ctypes.c_void_p(yh.ctypes.data), m,
                                          rows, ctypes.c_float(0.1), stream)
        assert rc == _lib.L2A_EINVAL, ("host", m, rows, rc)
    x, y = batches(row, 1, 4)
    args = (ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), 1, 4, ctypes.c_float(0.1), stream)
    assert lib.l2a_model_adapt_sgd(nm.handle, None, *args) == _lib.L2A_EINVAL
    for hole in range(len(base)):
        holed = list(base)
        holed[hole] = None
        assert lib.l2a_model_adapt_sgd(nm.handle, ptrs(holed), *args) == _lib.L2A_EINVAL, hole
    assert lib.l2a_model_adapt_sgd(nm.handle, ptrs(base), None, args[1], *args[2:]) == _lib.L2A_EINVAL
    assert lib.l2a_model_adapt_sgd(nm.handle, ptrs(base), args[0], None, *args[2:]) == _lib.L2A_EINVAL
    _sentinels_intact(nm, row, 0)
    nm.close()

    for hidden_act, output_act in (("swish", None), ("tanh", "tanh"), ("relu", "relu")):
        bad = NativeModel(row.od, row.ad, row.hidden, hidden_act, output_act, row.n_sets, "per_block")
        for e in range(row.n_sets):
            bad.set_weights(e, am.sentinel(row, e))
        assert lib.l2a_model_adapt_sgd(bad.handle, ptrs(base), *args) == _lib.L2A_EINVAL, (hidden_act, output_act)
        _sentinels_intact(bad, row, 0)
        bad.close()

    wide = am.BY_NAME["in129-h70-50"]
    winp = am.inputs(wide)
    nm = _model(wide)
    with pytest.raises(_lib.L2AError, match="l2a_model_adapt_sgd_raw failed \\(%d\\)" % _lib.L2A_EINVAL):
        nm.adapt_sgd_raw(_base_tensors(winp["base"], True), np.zeros((1, 4, wide.od)), np.zeros((1, 4, wide.ad)), np.zeros((1, 4, wide.od)),
                         {"obs": (np.zeros(wide.od), np.ones(wide.od)), "act": (np.zeros(wide.ad), np.ones(wide.ad)),
                          "delta": (np.zeros(wide.od), np.ones(wide.od))}, 0.1)
    _sentinels_intact(nm, wide, 0)
    nm.close()
