"""``l2a_mppi_sample_shard`` (``csrc/l2a_mppi.hip``: the SHARD instance of ``l2a_mppi_sample_k``) against ``l2a_mppi_sample`` on the
same inputs: one rank of a sharded plan samples ALL candidates - ``a_clip`` and ``mean_out`` bit for bit the unsharded call's - and
keeps the rollout tensor of its window ``[lo, hi)`` only, ``seq_local [h, m (hi - lo), A]``.  Every output starts from a sentinel
and sits between guard words (``test_cem_kernels_gpu._Out``).  Bit equality throughout: the two calls run the same arithmetic.
The two calls are one kernel body, so with injected normals both are also held to ``mppi_reference.sample_f32``, bit for bit - a
mistake they share would cancel in the comparison above."""

import numpy as np
import pytest

import mppi_reference as mr
from learning_to_adapt_amd import _lib
from test_cem_kernels_gpu import _Out, _ull, _up
from test_mppi_kernels_gpu import NAN, _bits, run_sample, sample_inputs

pytestmark = pytest.mark.gpu

# (n, m, h, A, world): 26 rows - a partial last workgroup - in uneven shards | two passes of the LDS tile (32 steps per pass at
# A = 16) and an empty shard (8 ranks, 7 candidates) | more than one workgroup per candidate row group, three envs | three passes
# (32 + 32 + 6), three envs with the three shifts, windows of 2 and 3 | two passes at A = 6 (85 + 1), windows of 2, 2, 2 and 3
SHAPES = [(13, 2, 5, 3, 3), (7, 1, 40, 16, 8), (96, 3, 6, 6, 4), (5, 3, 70, 16, 2), (9, 2, 86, 6, 4)]


def _window(n, rank, world):
    return (rank * n) // world, ((rank + 1) * n) // world


def run_shard(ctx, inp, lo, hi, expect_rc=_lib.L2A_OK, null_seq=False):
    """One ``l2a_mppi_sample_shard`` call; ``mean_out`` / ``a_clip`` / ``seq_local`` as host arrays, guards checked.  ``seq_local`` is
    allocated for at least one candidate so that an empty window has a sentinel-filled tensor to leave alone."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad = inp["n"], inp["m"], inp["h"], inp["ad"]
    D = h * ad
    width = max(hi - lo, 1) if 0 <= lo <= hi <= n else 1
    what = "sample_shard n=%d m=%d h=%d ad=%d window=[%d, %d) inject=%d" % (n, m, h, ad, lo, hi, inp["z"] is not None)
    keys = ("mean", "shift", "sigma", "low", "high", "z")
    dev = {k: (_up(inp[k]) if inp[k] is not None else None) for k in keys}
    out = dict(mean_out=_Out((m, D), torch.float32, NAN), a_clip=_Out((n, m, D), torch.float32, NAN),
               seq=_Out((h, m * width, ad), torch.float32, NAN))
    rc = ctx.lib.l2a_mppi_sample_shard(ctx.handle, _ptr(dev["z"]), _ull(inp.get("seed", 0)), _ull(inp.get("off", 0)), _ptr(dev["mean"]),
                                       _ptr(dev["shift"]), _ptr(dev["sigma"]), float(inp["beta"]), _ptr(dev["low"]), _ptr(dev["high"]),
                                       n, m, h, ad, lo, hi, out["mean_out"].ptr(), out["a_clip"].ptr(),
                                       None if null_seq else out["seq"].ptr(), _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    host = {k: o.host(k + " " + what) for k, o in out.items()}           # (the guard words behind every buffer)
    for k in keys:
        if inp[k] is not None:
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(inp[k])), "input changed: %s %s" % (k, what)
    if expect_rc != _lib.L2A_OK:
        assert all(np.isnan(v).all() for v in host.values()), "output written by a refused call: " + what
        return rc
    return host


@pytest.mark.parametrize("inject", [True, False], ids=["injected", "philox"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_m%d_h%d_A%d_w%d" % s)
def test_every_rank_matches_the_unsharded_sample(shape, inject):
    n, m, h, ad, world = shape
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n + 10 * h)
    shift = [(-1, 1, 0)[i % 3] for i in range(m)] if m > 1 else [1]
    inp = sample_inputs(rs, n, m, h, ad, 0.6, shift, inject=inject, seed=0x5EED0000ABCD1234, off=0 if inject else 977 * n * m * h * ad)
    full = run_sample(ctx, inp)
    assert not np.isnan(full["seq"]).any()
    seq_rows = full["seq"].reshape(h, m, n, ad)
    if inject:
        want_mean, want_a, want_seq = mr.sample_f32(inp["mean"], inp["shift"], inp["z"], inp["sigma"], inp["beta"], inp["low"],
                                                    inp["high"], n, m, h, ad)
        assert np.array_equal(_bits(full["mean_out"]), _bits(want_mean)), "mean_out against the reference"
        assert np.array_equal(_bits(full["a_clip"]), _bits(want_a)), "a_clip against the reference"
        assert np.array_equal(_bits(full["seq"]), _bits(want_seq)), "seq against the reference"
        ref_rows = want_seq.reshape(h, m, n, ad)
    widths = []
    for rank in range(world):
        lo, hi = _window(n, rank, world)
        widths.append(hi - lo)
        got = run_shard(ctx, inp, lo, hi, null_seq=(hi == lo and rank % 2 == 1))
        assert np.array_equal(_bits(got["a_clip"]), _bits(full["a_clip"])), (rank, "a_clip")
        assert np.array_equal(_bits(got["mean_out"]), _bits(full["mean_out"])), (rank, "mean_out")
        if hi == lo:
            assert np.isnan(got["seq"]).all(), "an empty window wrote seq_local"
            continue
        # plan row i * (hi - lo) + (j - lo) of every step t holds row i * n + j of the full tensor
        want = np.ascontiguousarray(seq_rows[:, :, lo:hi, :]).reshape(h, m * (hi - lo), ad)
        assert np.array_equal(_bits(got["seq"]), _bits(want)), (rank, lo, hi)
        if inject:
            want = np.ascontiguousarray(ref_rows[:, :, lo:hi, :]).reshape(h, m * (hi - lo), ad)
            assert np.array_equal(_bits(got["seq"]), _bits(want)), ("seq_local against the reference", rank, lo, hi)
    assert sum(widths) == n
    if world == 3:
        assert len(set(widths)) > 1                                     # uneven shards
    if world > n:
        assert 0 in widths                                              # an empty shard
        got = run_shard(ctx, inp, n, n)                                 # (also at the far end, with a tensor to leave alone)
        assert np.isnan(got["seq"]).all() and np.array_equal(_bits(got["a_clip"]), _bits(full["a_clip"]))


def test_bad_windows_are_refused_and_write_nothing():
    ctx = _lib.Context.get(0)
    inp = sample_inputs(np.random.RandomState(2), 13, 2, 5, 3, 0.6, [1, -1])
    for lo, hi in ((-1, 4), (3, 14), (5, 4)):
        assert run_shard(ctx, inp, lo, hi, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    # a window that holds candidates needs its tensor; l2a_mppi_sample's own refusals hold as well
    assert run_shard(ctx, inp, 0, 4, expect_rc=_lib.L2A_EINVAL, null_seq=True) == _lib.L2A_EINVAL
    assert run_shard(ctx, dict(inp, beta=0.0), 0, 4, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
