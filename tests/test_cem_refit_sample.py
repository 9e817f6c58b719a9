"""``l2a_cem_refit_sample``: the CEM iteration boundary (elite rank, mean / std refit, next samples) in one launch.

CPU: the entry point is declared, exported and bound, and its kernel runs without scratch.  GPU: every output is
bit-identical to ``l2a_cem_refit`` followed by ``l2a_cem_sample`` on the same inputs - both readings, injected and Philox
normals, candidate shards (an empty one included), elite counts 1 and n // 10, exact ties, NaN / inf returns, in place and
with distinct input buffers, and a shape beyond the launch's LDS budget (the entry point's fallback to the two calls)."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from learning_to_adapt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "learning_to_adapt_amd", "csrc", "_obj", "l2a_cem.o")


def test_refit_sample_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    assert re.search(r"\bint l2a_cem_refit_sample\(", text)
    assert "l2a_cem_refit_sample" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.l2a_cem_refit_sample.restype is ctypes.c_int
    assert len(lib.l2a_cem_refit_sample.argtypes) == 25
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT l2a_cem_refit_sample$", nm, flags=re.M)


def test_refit_sample_kernel_has_no_scratch():
    if not os.path.exists(OBJ):
        pytest.skip("library not built")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa_notes.sh"), OBJ, "refit_sample"], capture_output=True,
                         text=True, check=True).stdout
    line = [ln for ln in out.splitlines() if "l2a_cem_refit_sample_k" in ln]
    assert len(line) == 1, out
    assert "private_segment_fixed_size:0" in line[0] and "vgpr_spill_count:0" in line[0], line[0]


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _returns(rs, m, n, kind="mixed"):
    r = rs.randn(m, n).astype(np.float32) * 10
    if kind == "equal":
        r[:] = np.float32(1.5)
    elif kind == "nan":
        r[:] = np.nan
    elif n >= 8:
        r[:, n // 2] = r[:, 1]                          # exact ties across the index order
        r[:, n - 1] = r[:, 0]
        r[0, 2:6] = r[0, 3]
        r[0, n // 3] = np.nan                           # diverged rollouts sort last
        r[-1, n // 4] = -np.inf
        r[-1, n // 5] = np.inf
        r[:, n // 6] = 0.0
        r[:, n // 7] = -0.0                             # -0 == +0: a tie, broken by the index
    return r


def _case(ctx, rs, n, m, h, ad, k, reference, inject, lo, hi, in_place, kind="mixed", alpha=0.1):
    """Run both paths on the same inputs; assert every output bit-identical."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    lib = ctx.lib
    dev = torch.device("cuda:0")
    D = h * ad
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rets = up(_returns(rs, m, n, kind))
    a_in = up(rs.randn(n, m, D).astype(np.float32))
    mean0 = up((0.3 * rs.randn(m, D)).astype(np.float32))
    z = up(rs.randn(n, m, D).astype(np.float32)) if inject else None
    low, high = up(np.linspace(-0.8, -0.3, ad).astype(np.float32)), up(np.linspace(0.4, 0.9, ad).astype(np.float32))
    seed, off = 0x5EED0000ABCD1234 + n, 977 * n * m
    nsel = hi - lo
    stream = _stream_ptr(dev)
    mean0_host = mean0.cpu()

    def outs():
        nan = float("nan")
        return dict(rows=torch.full((m * k,), -7, dtype=torch.int32, device=dev), mean=mean0.clone(),
                    std=torch.full((m, D), nan, device=dev), a_clip=torch.full((n, m, D), nan, device=dev),
                    a_raw=torch.full((n, m, D), nan, device=dev), seq=torch.full((h, m * max(nsel, 1), ad), nan, device=dev))

    want = outs()
    ctx.check(lib.l2a_cem_refit(ctx.handle, _ptr(rets), _ptr(a_in), n, m, D, k, int(reference), alpha, _ptr(want["rows"]),
                                _ptr(want["mean"]), _ptr(want["std"]), stream), "l2a_cem_refit")
    ctx.check(lib.l2a_cem_sample(ctx.handle, _ptr(z), ctypes.c_ulonglong(seed), ctypes.c_ulonglong(off), _ptr(want["mean"]),
                                 _ptr(want["std"]), _ptr(low), _ptr(high), n, m, h, ad, int(reference), lo, hi, _ptr(want["a_clip"]),
                                 _ptr(want["a_raw"]), _ptr(want["seq"]) if nsel > 0 else None, stream), "l2a_cem_sample")
    got = outs()
    if in_place:        # the samples and the mean are overwritten by the launch that reads them (one slice per step)
        got["a_clip"] = a_in.clone()
        src, mean_in = got["a_clip"], None
    else:
        src, mean_in = a_in, mean0
    ctx.check(lib.l2a_cem_refit_sample(ctx.handle, _ptr(rets), _ptr(src), n, m, h, ad, k, int(reference), alpha, _ptr(z),
                                       ctypes.c_ulonglong(seed), ctypes.c_ulonglong(off), _ptr(low), _ptr(high), lo, hi,
                                       _ptr(got["rows"]), _ptr(mean_in), _ptr(got["mean"]), _ptr(got["std"]), _ptr(got["a_clip"]),
                                       _ptr(got["a_raw"]), _ptr(got["seq"]) if nsel > 0 else None, stream), "l2a_cem_refit_sample")
    torch.cuda.synchronize()
    what = "n=%d m=%d h=%d ad=%d k=%d reference=%d inject=%d shard=(%d, %d) in_place=%d %s" % (
        n, m, h, ad, k, reference, inject, lo, hi, in_place, kind)
    for key in ("rows", "mean", "std", "a_clip", "a_raw", "seq"):
        assert torch.equal(_bits(got[key]), _bits(want[key])), "%s differs: %s" % (key, what)
    assert torch.equal(_bits(mean0.cpu()), _bits(mean0_host))        # mean_in is read only


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("n", [37, 400, 4000])
def test_refit_sample_matches_refit_then_sample(n, m):
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(1000 * m + n)
    shards = [(0, n), (n // 3, (2 * n) // 3), (n // 2, n // 2)]
    c = 0
    for reference in (True, False):
        for k in sorted({1, max(n // 10, 1)}):
            for inject in (True, False):
                for in_place in (False, True):
                    lo, hi = shards[c % 3]
                    c += 1
                    _case(ctx, rs, n, m, 4, 3, k, reference, inject, lo, hi, in_place)


@pytest.mark.gpu
@pytest.mark.parametrize("reference", [True, False])
def test_refit_sample_config5_shape(reference):
    """Config 5's iteration (m = 1, n = 4000, h = 30, act_dim = 6, 400 elites) and its 8-way shard 0."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(5)
    for inject in (False, True):
        _case(ctx, rs, 4000, 1, 30, 6, 400, reference, inject, 0, 4000, False)
        _case(ctx, rs, 4000, 1, 30, 6, 400, reference, inject, 0, 500, True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["equal", "nan"])
def test_refit_sample_all_tied_returns(kind):
    """Every return equal (or every rollout diverged): one bin, ranks decided by the index alone."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(11)
    for reference in (True, False):
        _case(ctx, rs, 400, 2, 3, 2, 40, reference, False, 0, 400, False, kind=kind)


@pytest.mark.gpu
def test_refit_sample_fallback_beyond_lds():
    """30000 candidates: the fused launch's bins exceed a workgroup's LDS, the entry point runs refit + sample itself."""
    ctx = _lib.Context.get(0)
    for reference in (0, 1):
        assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, 30000, 1, 2, 2, 3000, reference) == 0
        assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, 4000, 1, 30, 6, 400, reference) == 1
    rs = np.random.RandomState(3)
    for reference in (True, False):
        _case(ctx, rs, 30000, 1, 2, 2, 3000, reference, False, 0, 30000, False)
        _case(ctx, rs, 30000, 1, 2, 2, 3000, reference, True, 100, 200, True)
