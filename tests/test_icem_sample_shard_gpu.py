"""``l2a_icem_sample_shard`` (``csrc/l2a_icem.hip``: the SHARD instance of ``l2a_icem_sample_k``) against ``l2a_icem_sample`` on the
same inputs: one rank of a sharded plan fetches, draws and clips ALL ``n_it`` rows - ``a_clip``, ``mean_out`` and ``std_out`` bit for
bit the unsharded call's - and keeps the rollout tensor of its window ``[lo, hi)`` only, ``seq_local [h, m (hi - lo), A]``; kept rows
and the mean row inside the window are rows like any other.  Every output starts from a sentinel and sits between guard words
(``test_cem_kernels_gpu._Out``): ``seq_local`` is allocated at exactly ``h * m * (hi - lo) * A`` floats, so a store behind it trips
the guard.  Bit equality throughout: the two calls run the same arithmetic.  The two calls are one kernel body, so with injected
normals the unsharded call is also held to ``icem_reference.sample_f32`` (``test_icem_kernels_gpu.check_sample``), bit for bit."""

import numpy as np
import pytest

from learning_to_adapt_amd import _lib
from test_cem_kernels_gpu import _Out, _ull, _up
from test_icem_kernels_gpu import NAN, SAMPLE_KEYS, _bits, check_sample, run_sample, sample_inputs

pytestmark = pytest.mark.gpu

KK = 4
# (n_it, m, h, A): 39 sample rows in workgroups of four - a partial last workgroup, three envs, one of them fresh | D = 32: four rows
# per workgroup again, two envs that both hold kept rows | D = 2080: one row per workgroup and two passes of the LDS tile (128 + 2
# steps at A = 16) - seq_local is stored at step t0 + tt with the window's row index in the second one; n_it = 3 is below the inner
# windows of ``windows``, so this shape gets its own
SHAPES = [(13, 3, 5, 6), (40, 2, 4, 8), (3, 2, 130, 16)]
KC = {3: [3, 4, 2], 2: [2, 4]}
SHIFT = {3: [1, 0, -1], 2: [1, 0]}


def windows(n):
    """name -> [lo, hi): all rows, an inner window, one row, an empty window, kept rows only (hi <= kc of every running env), the
    window that holds the add_mean row."""
    if n < 13:
        return dict(full=(0, n), one=(1, 2), empty=(2, 2), kept=(0, 2), mean=(n - 1, n), tail=(1, n))
    return dict(full=(0, n), inner=(4, 9), one=(5, 6), empty=(7, 7), kept=(0, 2), mean=(n - 3, n))


def run_shard(ctx, inp, lo, hi, expect_rc=_lib.L2A_OK, null_seq=False):
    """One ``l2a_icem_sample_shard`` call; the four outputs as host arrays, guards checked.  An empty (or refused) window gets a
    tensor of one candidate to leave alone."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad, Kk = inp["n"], inp["m"], inp["h"], inp["ad"], inp["Kk"]
    D = h * ad
    width = max(hi - lo, 1) if 0 <= lo <= hi <= n else 1
    what = "sample_shard n=%d m=%d h=%d ad=%d window=[%d, %d) inject=%d" % (n, m, h, ad, lo, hi, inp["z"] is not None)
    dev = {k: (_up(inp[k]) if inp[k] is not None else None) for k in SAMPLE_KEYS}
    arg = {k: _ptr(dev[k]) for k in SAMPLE_KEYS}
    out = dict(mean_out=_Out((m, D), torch.float32, NAN), std_out=_Out((m, D), torch.float32, NAN),
               a_clip=_Out((n, m, D), torch.float32, NAN), seq=_Out((h, m * width, ad), torch.float32, NAN))
    rc = ctx.lib.l2a_icem_sample_shard(ctx.handle, arg["z"], _ull(inp.get("seed", 0)), _ull(inp.get("off", 0)), arg["mean"], arg["std"],
                                       arg["kept"], arg["kc"], arg["shift"], arg["sigma0"], float(inp["rho"]), arg["low"], arg["high"],
                                       n, m, h, ad, Kk, int(inp["add_mean"]), lo, hi, out["mean_out"].ptr(), out["std_out"].ptr(),
                                       out["a_clip"].ptr(), None if null_seq else out["seq"].ptr(), _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    host = {k: o.host(k + " " + what) for k, o in out.items()}           # (the guard words behind every buffer)
    for k in SAMPLE_KEYS:
        if inp[k] is not None:
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(inp[k])), "input changed: %s %s" % (k, what)
    if expect_rc != _lib.L2A_OK:
        assert all(np.isnan(v).all() for v in host.values()), "output written by a refused call: " + what
        return rc
    return host


def _inputs(shape, inject):
    n, m, h, ad = shape
    rs = np.random.RandomState(n + 10 * h)
    return sample_inputs(rs, n, m, h, ad, 0.5, SHIFT[m], Kk=KK, kc=KC[m], add_mean=1, inject=inject, seed=0x5EED0000ABCD1234,
                         off=0 if inject else 977 * n * m * h * ad)


@pytest.mark.parametrize("inject", [True, False], ids=["injected", "philox"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_h%d_A%d" % s)
def test_every_window_matches_the_unsharded_sample(shape, inject):
    n, m, h, ad = shape
    ctx = _lib.Context.get(0)
    inp = _inputs(shape, inject)
    full = run_sample(ctx, inp)
    assert not np.isnan(full["seq"]).any()
    if inject:
        check_sample(full, inp, True, "the unsharded call against the reference, n=%d m=%d h=%d ad=%d" % shape)
    seq_rows = full["seq"].reshape(h, m, n, ad)
    # the rows the windows are about are what they are named after: kept rows differ from drawn ones, the mean row is clip(mu')
    running = [i for i in range(m) if SHIFT[m][i] >= 0]
    assert all(KC[m][i] >= 2 for i in running)
    for name, (lo, hi) in windows(n).items():
        got = run_shard(ctx, inp, lo, hi, null_seq=(name == "empty" and inject))
        for key in ("a_clip", "mean_out", "std_out"):
            assert np.array_equal(_bits(got[key]), _bits(full[key])), (name, key)
        if hi == lo:
            assert np.isnan(got["seq"]).all(), "an empty window wrote seq_local"
            continue
        # plan row i * (hi - lo) + (j - lo) of every step t holds row i * n_it + j of the full tensor
        want = np.ascontiguousarray(seq_rows[:, :, lo:hi, :]).reshape(h, m * (hi - lo), ad)
        assert np.array_equal(_bits(got["seq"]), _bits(want)), (name, lo, hi)
    # the mean row inside its window: clip(mu'[i]) of every env, as the full call wrote it
    lo, hi = windows(n)["mean"]
    low, high = np.tile(inp["low"], h), np.tile(inp["high"], h)
    for i in range(m):
        row = full["a_clip"][n - 1, i]
        assert np.array_equal(_bits(row), _bits(np.clip(full["mean_out"][i], low, high))), i


def test_bad_windows_are_refused_and_write_nothing():
    ctx = _lib.Context.get(0)
    inp = _inputs(SHAPES[0], True)
    for lo, hi in ((-1, 4), (3, 14), (5, 4)):
        assert run_shard(ctx, inp, lo, hi, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    # a window that holds candidates needs its tensor; l2a_icem_sample's own refusals hold as well
    assert run_shard(ctx, inp, 0, 4, expect_rc=_lib.L2A_EINVAL, null_seq=True) == _lib.L2A_EINVAL
    assert run_shard(ctx, dict(inp, rho=1.0), 0, 4, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_shard(ctx, dict(inp, Kk=8193), 0, 4, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
