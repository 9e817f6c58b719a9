"""The iCEM planner kernels of ``csrc/l2a_icem.hip`` (``l2a_icem_sample_k``; ``l2a_icem_rank_k`` + ``l2a_icem_stats_k`` behind
``l2a_icem_refit``) against ``tests/icem_reference.py``, a plain NumPy restatement pinned by ``tests/test_icem_reference.py``.  The C
entry points are called directly; every output starts from NaN (integers: -7) and sits between 64 guard words
(``test_cem_kernels_gpu._Out``); the inputs are checked unchanged.

Bounds (derived, none measured and then set): samples from injected normals bit for bit (``sample_f32``); samples from the Philox
stream at ``rho = 0`` bit for bit against ``l2a_cem_sample(reference = 0)`` on the same seed and offset; the refit's elites, counts,
index, kept rows and packed action exact, its mean and std within ``icem_reference.refit_bounds``.  The refit tests print the worst
error / bound ratio they saw (``-s``)."""

import ctypes

import numpy as np
import pytest

import icem_reference as ir
from learning_to_adapt_amd import _lib
from test_cem_kernels_gpu import Worst, _Out, _ull, _up, returns_pattern
from test_mppi_kernels_gpu import PATTERNS, SHIFTS3

pytestmark = pytest.mark.gpu

NAN = float("nan")
SAMPLE_KEYS = ("mean", "std", "kept", "kc", "shift", "sigma0", "low", "high", "z")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _bounds(ad):
    return np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)


def _same_on_device(dev, host, what):
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(host)), "input changed: " + what


# ---------------------------------------------------------------------------------------------------------------------- harness
def run_sample(ctx, inp, with_seq=True, expect_rc=_lib.L2A_OK, alias=None, null=None):
    """One ``l2a_icem_sample`` call; returns ``mean_out`` / ``std_out`` / ``a_clip`` / ``seq`` as host arrays (guards checked).  With
    an error expected: every output must still hold NaN.  ``alias = (output, input)`` passes the input's buffer as that output;
    ``null`` names an argument passed as NULL."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad, Kk = inp["n"], inp["m"], inp["h"], inp["ad"], inp["Kk"]
    D = h * ad
    what = "sample n=%d m=%d h=%d ad=%d rho=%g Kk=%d kc=%s shift=%s add_mean=%d inject=%d seq=%d" % (
        n, m, h, ad, inp["rho"], Kk, None if inp["kc"] is None else list(inp["kc"]), list(inp["shift"]), inp["add_mean"],
        inp["z"] is not None, with_seq)
    dev = {k: (_up(inp[k]) if inp[k] is not None else None) for k in SAMPLE_KEYS}
    out = dict(mean_out=_Out((m, D), torch.float32, NAN), std_out=_Out((m, D), torch.float32, NAN),
               a_clip=_Out((max(n, 1), m, D), torch.float32, NAN), seq=_Out((h, m * max(n, 1), ad), torch.float32, NAN))
    ptr = {k: o.ptr() for k, o in out.items()}
    if not with_seq:
        ptr["seq"] = None
    if alias is not None:
        ptr[alias[0]] = _ptr(dev[alias[1]])
    arg = {k: _ptr(dev[k]) for k in SAMPLE_KEYS}
    if null is not None:
        (ptr if null in ptr else arg)[null] = None
    rc = ctx.lib.l2a_icem_sample(ctx.handle, arg["z"], _ull(inp.get("seed", 0)), _ull(inp.get("off", 0)), arg["mean"], arg["std"],
                                 arg["kept"], arg["kc"], arg["shift"], arg["sigma0"], float(inp["rho"]), arg["low"], arg["high"],
                                 n, m, h, ad, Kk, int(inp["add_mean"]), ptr["mean_out"], ptr["std_out"], ptr["a_clip"], ptr["seq"],
                                 _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    host = {k: o.host(k + " " + what) for k, o in out.items()}
    for k in SAMPLE_KEYS:
        if inp[k] is not None:
            _same_on_device(dev[k], inp[k], k + " " + what)
    if expect_rc != _lib.L2A_OK:
        assert all(np.isnan(v).all() for v in host.values()), "output written by a refused call: " + what
        return rc
    if not with_seq:
        assert np.isnan(host["seq"]).all(), "seq written though NULL was passed: " + what
    return host


def sample_inputs(rs, n, m, h, ad, rho, shift, Kk=0, kc=None, add_mean=0, inject=True, seed=0, off=0):
    D = h * ad
    low, high = _bounds(ad)
    sigma0 = (0.1 + 0.5 * rs.rand(ad)).astype(np.float32)
    mean = (0.7 * rs.randn(m, D)).astype(np.float32)            # beyond both bounds in some dimensions
    std = (0.05 + 0.6 * rs.rand(m, D)).astype(np.float32)
    kept = np.clip((0.5 * rs.randn(m, Kk, D)).astype(np.float32), np.tile(low, h), np.tile(high, h)) if Kk > 0 else None
    z = rs.randn(max(n, 1), m, D).astype(np.float32) if inject else None
    return dict(n=n, m=m, h=h, ad=ad, rho=rho, Kk=Kk, add_mean=add_mean, shift=np.asarray(shift, dtype=np.int32), mean=mean, std=std,
                kept=kept, kc=None if Kk == 0 else np.asarray(kc, dtype=np.int32), sigma0=sigma0, low=low, high=high, z=z, seed=seed,
                off=off)


def want_sample(inp):
    return ir.sample_f32(inp["mean"], inp["std"], inp["kept"], inp["kc"], inp["shift"], inp["z"], inp["sigma0"], inp["rho"], inp["low"],
                         inp["high"], inp["n"], inp["m"], inp["h"], inp["ad"], inp["Kk"], inp["add_mean"])


def check_sample(got, inp, with_seq, what):
    mu, sd, a, seq = want_sample(inp)
    assert np.array_equal(_bits(got["mean_out"]), _bits(mu)), "mean_out: " + what
    assert np.array_equal(_bits(got["std_out"]), _bits(sd)), "std_out: " + what
    assert np.array_equal(_bits(got["a_clip"]), _bits(a)), "a_clip: " + what
    if with_seq:
        assert np.array_equal(_bits(got["seq"]), _bits(seq)), "seq: " + what
    return a


# ------------------------------------------------------------------------------------------------- sample with injected normals
SAMPLE_N = (1, 2, 63, 64, 65, 257)
K_SAMPLE = 4


def sample_cases():
    """The sub-cases of one injected-normals test, ``(n, m, Kk, shift, kc, add_mean, with_seq)``: every ``n_it`` of ``SAMPLE_N`` x every
    ``Kk`` in (0, 1, K) x every one of the six shift vectors of ``SHIFTS3`` at m = 3 and the three shifts at m = 1 - explicit loops, so
    no combination depends on a counter's period.  Env i's stored count walks (0, 1, Kk) with the index of ``n_it``, moved on by the
    vector's index and by i; the mean row and a NULL ``seq`` follow the (vector, Kk) index.  ``check_sample_cases`` states what
    that covers."""
    out = []
    for ni, n in enumerate(SAMPLE_N):
        for ki, Kk in enumerate((0, 1, K_SAMPLE)):
            for vi, shift in enumerate(list(SHIFTS3) + [[-1], [1], [0]]):
                idx = vi * 3 + ki
                kc = [int((0, 1, Kk)[(ni + vi + i) % 3]) for i in range(len(shift))]
                out.append((n, len(shift), Kk, list(shift), kc, (idx // 4) % 2, idx % 4 != 3))
    return out


def check_sample_cases(cs):
    """Every shift vector met every ``Kk`` at every ``n_it``; with kept rows on (``Kk`` = 1, K), every sign of an env's shift met every
    distinct stored count, at m = 1 and at m = 3; the mean row and the NULL ``seq`` were both on and off at every ``n_it``."""
    vectors = [tuple(v) for v in SHIFTS3] + [(-1,), (1,), (0,)]
    assert {(n, Kk, tuple(sh)) for n, _, Kk, sh, _, _, _ in cs} == {(n, Kk, v) for n in SAMPLE_N for Kk in (0, 1, K_SAMPLE) for v in vectors}
    for Kk in (1, K_SAMPLE):
        for m in (1, 3):
            seen = {(int(np.sign(sh[i])), kc[i]) for _, mm, kk, sh, kc, _, _ in cs if kk == Kk and mm == m for i in range(m)}
            assert seen == {(sg, k) for sg in (-1, 0, 1) for k in {0, 1, Kk}}, (Kk, m, sorted(seen))
    for n in SAMPLE_N:
        assert {(am, ws) for nn, _, _, _, _, am, ws in cs if nn == n} == {(0, True), (0, False), (1, True), (1, False)}, n


@pytest.mark.parametrize("rho", [0.0, 0.5, 0.96875])
@pytest.mark.parametrize("h,ad", [(1, 1), (2, 16), (3, 11), (30, 6), (10, 8), (7, 16)])
def test_sample_with_injected_normals_bit_for_bit(h, ad, rho):
    """(The shapes take 4, 4, 4, 1, 3 and 2 sample rows per workgroup: the entry point's choice, ``256 // D`` held to 1 .. 4.)
    ``mean_out``, ``std_out``, ``a_clip`` and ``seq`` equal ``sample_f32`` bit for bit over ``sample_cases``: all six mixed shift
    vectors at m = 3 and the three shifts at m = 1 with every ``Kk`` in (0, 1, K) at every ``n_it``, per-env counts in (0, 1, Kk) - at
    ``n_it`` = 1 and 2 that is ``kc >= n_it`` -, the mean row on and off, with and without ``seq``."""
    ctx = _lib.Context.get(0)
    seed = 1000 * h + 10 * ad + int(rho * 32)
    rs = np.random.RandomState(seed)
    cs = sample_cases()
    check_sample_cases(cs)
    on_low = on_high = kept_beyond = False
    for n, m, Kk, shift, kc, add_mean, with_seq in cs:
        inp = sample_inputs(rs, n, m, h, ad, rho, shift, Kk=Kk, kc=kc, add_mean=add_mean)
        got = run_sample(ctx, inp, with_seq=with_seq)
        what = "n=%d m=%d h=%d ad=%d rho=%g Kk=%d kc=%s shift=%s add_mean=%d" % (n, m, h, ad, rho, Kk, kc, shift, add_mean)
        a = check_sample(got, inp, with_seq, what)
        on_low = on_low or bool((a == np.tile(inp["low"], h)).any())
        on_high = on_high or bool((a == np.tile(inp["high"], h)).any())
        kept_beyond = kept_beyond or any(ir.kept_count(kc[i], Kk, shift[i]) >= n for i in range(m))
    assert on_low and on_high, "no sub-case put a sample on each bound"
    assert kept_beyond, "no sub-case had as many kept rows as candidates"


@pytest.mark.parametrize("h,ad", [(130, 16), (300, 7)])
def test_sample_over_a_horizon_of_several_passes(h, ad):
    """The horizon goes through the LDS tiles in passes of ``2048 // (rows * A)`` steps (one row per workgroup at these lengths):
    128 + 2 steps at A = 16, 292 + 8 at A = 7.  The recurrence enters the second pass with its state from the first, and the last
    pass is shorter: bit for bit against ``sample_f32`` with mixed shifts, kept rows (shifted across the pass boundary) and the
    mean row."""
    ctx = _lib.Context.get(0)
    assert h > 2048 // ad and 256 // (h * ad) < 1
    rs = np.random.RandomState(h + ad)
    c = 0
    for n in (2, 5):
        for m, shift in ((1, [1]), (3, [0, -1, 1]), (3, [1, 0, -1])):
            for rho in (0.5, 0.96875):
                Kk = (0, 2)[c % 2]
                inp = sample_inputs(rs, n, m, h, ad, rho, shift, Kk=Kk, kc=[(2, 1, 0)[(c + i) % 3] for i in range(m)], add_mean=(c // 2) % 2)
                with_seq = c % 5 != 4
                c += 1
                check_sample(run_sample(ctx, inp, with_seq=with_seq), inp, with_seq, "h=%d ad=%d n=%d m=%d rho=%g Kk=%d" % (h, ad, n, m, rho, Kk))


def test_the_mean_row_wins_over_a_kept_row():
    """``n_it = 1`` with ``kc = 1``: with ``add_mean`` the only row is ``clip(mu')``, without it the kept row; ``n_it = 3`` with three
    kept rows: the last one gives way to the mean."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(21)
    h, ad = 3, 4
    lowD, highD = np.tile(_bounds(ad)[0], h), np.tile(_bounds(ad)[1], h)
    for n, Kk in ((1, 1), (3, 3)):
        for add_mean in (1, 0):
            inp = sample_inputs(rs, n, 2, h, ad, 0.5, [0, 1], Kk=Kk, kc=[Kk, Kk], add_mean=add_mean)
            got = run_sample(ctx, inp)
            check_sample(got, inp, True, "n=%d Kk=%d add_mean=%d" % (n, Kk, add_mean))
            for i in range(2):
                shifted = ir.shift_rows(inp["kept"][i, n - 1], inp["shift"][i] > 0, h, ad)
                mean_row = np.clip(got["mean_out"][i], lowD, highD)
                assert np.array_equal(_bits(got["a_clip"][n - 1, i]), _bits(mean_row if add_mean else shifted))


# ---------------------------------------------------------------------------------------------------------- Philox bit-identity
def _cem_sample(ctx, inp, mean, std):
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad = inp["n"], inp["m"], inp["h"], inp["ad"]
    dev = [_up(v) for v in (mean, std, inp["low"], inp["high"])]
    a_clip, seq = _Out((n, m, h * ad), torch.float32, NAN), _Out((h, m * n, ad), torch.float32, NAN)
    rc = ctx.lib.l2a_cem_sample(ctx.handle, None, _ull(inp["seed"]), _ull(inp["off"]), _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]),
                                _ptr(dev[3]), n, m, h, ad, 0, 0, n, a_clip.ptr(), None, seq.ptr(), _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == _lib.L2A_OK, ctx.lib.l2a_last_error(ctx.handle).decode()
    return a_clip.host("cem a_clip"), seq.host("cem seq")


@pytest.mark.parametrize("off", [0, (1 << 32) - 5, 1 << 40])
def test_philox_stream_is_cem_sample_bit_for_bit(off):
    """``rho = 0``, ``Kk = 0``, Philox normals: ``a_clip`` and ``seq`` equal ``l2a_cem_sample(reference = 0)`` on the same seed and
    offset, bit for bit (the launch at 2^32 - 5 crosses into the counter's high word).  Two settings in which CEM's
    ``mean + z * std`` rounds as this kernel's separate product and sum do whether or not a compiler fuses it: fresh envs
    (``mu' = 0``: the sum adds zero) and kept spreads that are powers of two (the product is exact)."""
    ctx = _lib.Context.get(0)
    n, m, h, ad = 66, 2, 4, 8
    D = h * ad
    for seed in (0x5EED0000ABCD1234, 1):
        rs = np.random.RandomState(7)
        fresh = sample_inputs(rs, n, m, h, ad, 0.0, [-1, -1], inject=False, seed=seed, off=off)
        got = run_sample(ctx, fresh)
        want_a, want_seq = _cem_sample(ctx, fresh, np.zeros((m, D), dtype=np.float32), np.tile(fresh["sigma0"], (m, h)))
        what = "seed=%#x offset=%#x" % (seed, off)
        assert np.array_equal(_bits(got["a_clip"]), _bits(want_a)), "a_clip (fresh envs): " + what
        assert np.array_equal(_bits(got["seq"]), _bits(want_seq)), "seq (fresh envs): " + what
        kept = sample_inputs(rs, n, m, h, ad, 0.0, [0, 0], inject=False, seed=seed, off=off)
        kept["std"] = (2.0 ** rs.randint(-4, 0, size=(m, D))).astype(np.float32)
        got = run_sample(ctx, kept)
        want_a, want_seq = _cem_sample(ctx, kept, kept["mean"], kept["std"])
        assert np.array_equal(_bits(got["a_clip"]), _bits(want_a)), "a_clip (kept mean and spread): " + what
        assert np.array_equal(_bits(got["seq"]), _bits(want_seq)), "seq (kept mean and spread): " + what
        assert len(np.unique(want_a)) > n * m * D // 4              # (not a degenerate comparison: most samples lie inside the bounds)


# ------------------------------------------------------------------------------------------------------------------------ refit
def run_refit(ctx, dev, inp, expect_rc=_lib.L2A_OK, alias=None, null=None, what=""):
    """One ``l2a_icem_refit`` call on uploaded ``dev['returns']`` / ``dev['a_clip']``; returns the outputs as host arrays."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad, K, Kk = inp["n"], inp["m"], inp["h"], inp["ad"], inp["K"], inp["Kk"]
    D = h * ad
    out = dict(work=_Out((m, max(K, 1)), torch.int32, -7), mean=_Out((m, D), torch.float32, NAN, init=_up(inp["mean0"])),
               std=_Out((m, D), torch.float32, NAN, init=_up(inp["std0"])), kept=_Out((m, max(Kk, 1), D), torch.float32, NAN),
               kc=_Out((m,), torch.int32, -7), out=_Out((m, ad + 4), torch.float32, NAN))
    ptr = {k: o.ptr() for k, o in out.items()}
    arg = dict(returns=_ptr(dev["returns"]), a_clip=_ptr(dev["a_clip"]), low=_ptr(dev["low"]), high=_ptr(dev["high"]))
    if alias is not None:
        ptr[alias[0]] = arg[alias[1]] if alias[1] in arg else ptr[alias[1]]
    if null is not None:
        (ptr if null in ptr else arg)[null] = None
    rc = ctx.lib.l2a_icem_refit(ctx.handle, arg["returns"], arg["a_clip"], arg["low"], arg["high"], n, m, h, ad, K, Kk, float(inp["alpha"]),
                                ptr["work"], ptr["mean"], ptr["std"], ptr["kept"], ptr["kc"], ptr["out"], _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    got = {k: o.host(k + " " + what) for k, o in out.items()}
    if expect_rc != _lib.L2A_OK:
        assert np.array_equal(_bits(got["mean"]), _bits(inp["mean0"])) and np.array_equal(_bits(got["std"]), _bits(inp["std0"])), what
        assert np.isnan(got["kept"]).all() and np.isnan(got["out"]).all() and np.all(got["kc"] == -7) and np.all(got["work"] == -7), \
            "output written by a refused call: " + what
        return rc
    return got


def refit_inputs(rs, n, m, h, ad, K, Kk, alpha=0.1, returns=None, pattern="distinct"):
    D = h * ad
    low, high = _bounds(ad)
    a_clip = np.clip((0.2 + 0.6 * rs.randn(n, m, D)).astype(np.float32), np.tile(low, h), np.tile(high, h))
    return dict(n=n, m=m, h=h, ad=ad, K=K, Kk=Kk, alpha=alpha, low=low, high=high, a_clip=a_clip,
                mean0=(0.7 * rs.randn(m, D)).astype(np.float32), std0=(0.05 + 0.6 * rs.rand(m, D)).astype(np.float32),
                returns=returns_pattern(pattern, rs, m, n) if returns is None else returns)


def upload_refit(inp):
    return {k: _up(inp[k]) for k in ("returns", "a_clip", "low", "high")}


def check_refit(got, inp, worst, what, ranked=None):
    n, m, ad, K, Kk = inp["n"], inp["m"], inp["ad"], inp["K"], inp["Kk"]
    ref = ir.refit(inp["mean0"], inp["std0"], inp["a_clip"], inp["returns"], K, Kk, inp["alpha"], inp["low"], inp["high"], ad, ranked=ranked)
    row = got["out"]
    assert np.array_equal(_bits(row[:, ad + 1].copy()), ref["index"].astype(np.int32)), "index: " + what
    assert np.array_equal(_bits(row[:, ad + 2].copy()), ref["Ke"].astype(np.int32)), "Ke: " + what
    assert np.array_equal(_bits(row[:, ad + 3].copy()), ref["valid"].astype(np.int32)), "valid: " + what
    live = ref["Ke"] > 0
    assert np.array_equal(_bits(row[live, ad].copy()), _bits(ref["best_return"][live])), "best return: " + what
    assert np.isnan(row[~live, ad]).all(), what
    assert np.array_equal(_bits(row[:, :ad].copy()), _bits(ref["action"])), "packed action: " + what
    assert np.array_equal(got["kc"], ref["kc"].astype(np.int32)), "kc: " + what
    for i in range(m):
        ke, kc = int(ref["Ke"][i]), int(ref["kc"][i])
        assert np.array_equal(got["work"][i, :ke], ref["elites"][i].astype(np.int32)), "elites of env %d: %s" % (i, what)
        assert np.all(got["work"][i, ke:] == -7), "work written beyond Ke: " + what
        if Kk > 0:
            assert np.array_equal(_bits(got["kept"][i, :kc]), _bits(ref["kept"][i])), "kept rows of env %d: %s" % (i, what)
            assert np.isnan(got["kept"][i, kc:]).all(), "kept rows written beyond kc: " + what
    if Kk == 0:
        assert np.isnan(got["kept"]).all(), what
    assert np.array_equal(_bits(got["mean"][~live]), _bits(inp["mean0"][~live])), "an env without elites: its mean was touched: " + what
    assert np.array_equal(_bits(got["std"][~live]), _bits(inp["std0"][~live])), "an env without elites: its std was touched: " + what
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all(), what
    B = max(float(np.max(np.abs(inp["a_clip"]))), float(np.max(np.abs(inp["mean0"]))), float(np.max(np.abs(inp["std0"]))))
    for i in np.flatnonzero(live):
        mean_bound, std_bound = ir.refit_bounds(int(ref["Ke"][i]), B)
        r = worst.note("mean", np.abs(got["mean"][i].astype(np.float64) - ref["mean"][i]), mean_bound)
        assert r <= 1.0, "mean off by %.3f of its bound %.3e: %s" % (r, mean_bound, what)
        r = worst.note("std", np.abs(got["std"][i].astype(np.float64) - ref["std"][i]), std_bound)
        assert r <= 1.0, "std off by %.3f of its bound %.3e: %s" % (r, std_bound, what)
    return ref


REFIT_N = (1, 2, 63, 64, 65, 511, 513, 4097)


@pytest.mark.parametrize("n", REFIT_N)
def test_refit_over_shapes_and_return_patterns(n):
    """Elite membership and order, ``Ke``, the valid count, the index, the kept rows and the packed action exactly the
    restatement's; mean and std within the derived bound; ``K`` in (1, 2, n, n + 3) (above 8192 the entry refuses: held to it),
    ``Kk`` in (0, 1, K); every return pattern of ``test_mppi_kernels_gpu.PATTERNS``."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n * 37)
    worst = Worst()
    some_dead = some_short = False
    shapes = ((3, 11), (30, 6)) if n < 4097 else ((3, 11),)
    for c, (h, ad) in enumerate(shapes):
        m = 3 if (c == 0 or n >= 511) else 1
        base = refit_inputs(rs, n, m, h, ad, 1, 0)
        dev = upload_refit(base)
        for pattern in PATTERNS:
            returns = returns_pattern(pattern, rs, m, n)
            dev["returns"] = _up(returns)
            ranked = ir.elites(returns, n + 3)
            for q, K in enumerate(sorted(set(min(k, 8192) for k in (1, 2, n, n + 3)))):
                Kk = (0, 1, K)[(q + c) % 3]
                inp = dict(base, K=K, Kk=Kk, returns=returns, alpha=(0.1, 0.0, 0.75)[q % 3])
                what = "refit n=%d m=%d h=%d ad=%d K=%d Kk=%d alpha=%g %s" % (n, m, h, ad, K, Kk, inp["alpha"], pattern)
                ref = check_refit(run_refit(ctx, dev, inp, what=what), inp, worst, what, ranked=ranked)
                some_dead = some_dead or bool((ref["Ke"] == 0).any())
                some_short = some_short or bool(((ref["Ke"] > 0) & (ref["Ke"] < min(K, n))).any())
            _same_on_device(dev["returns"], returns, "returns n=%d %s" % (n, pattern))
        _same_on_device(dev["a_clip"], base["a_clip"], "a_clip n=%d" % n)
    assert some_dead, "no env without a valid candidate"
    assert some_short or n == 1, "no env with fewer valid candidates than K"
    worst.report("icem refit n=%d" % n)


def test_refit_is_deterministic_and_equal_across_envs():
    """The same inputs give the same bits run after run (the grid is the entry point's, not the caller's: there is one), and envs
    with equal returns and samples - other workgroups, other rows of the grid - get equal results."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(11)
    n, m, h, ad, K = 513, 2, 30, 6, 51
    inp = refit_inputs(rs, n, m, h, ad, K, 15)
    inp["a_clip"] = np.ascontiguousarray(np.broadcast_to(inp["a_clip"][:, :1], inp["a_clip"].shape))
    inp["returns"] = np.ascontiguousarray(np.broadcast_to(rs.choice([-1.5, 0.25, 7.0, np.nan], size=(1, n)).astype(np.float32), (m, n)))
    inp["mean0"][1], inp["std0"][1] = inp["mean0"][0], inp["std0"][0]
    dev = upload_refit(inp)
    runs = [run_refit(ctx, dev, inp) for _ in range(3)]
    for g in runs[1:]:
        for k in ("work", "mean", "std", "kept", "kc", "out"):
            assert np.array_equal(_bits(g[k]), _bits(runs[0][k])), k
    for k in ("work", "mean", "std", "kept", "kc", "out"):
        assert np.array_equal(_bits(runs[0][k][0]), _bits(runs[0][k][1])), k
    check_refit(runs[0], inp, Worst(), "determinism case")


def test_sample_is_deterministic():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(15)
    inp = sample_inputs(rs, 65, 3, 7, 6, 0.5, [1, 0, -1], Kk=3, kc=[3, 1, 2], add_mean=1, inject=False, seed=5, off=1 << 33)
    runs = [run_sample(ctx, inp) for _ in range(2)]
    for k in runs[0]:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k


# --------------------------------------------------------------------------------------------------------------- argument errors
def test_sample_argument_errors_write_nothing():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(12)
    E = _lib.L2A_EINVAL

    def case(n=5, m=2, h=3, ad=4, rho=0.5, Kk=2, **kw):
        return run_sample(ctx, sample_inputs(rs, n, m, h, ad, rho, [0] * m, Kk=Kk, kc=[1] * m), expect_rc=E, **kw)

    for rho in (1.0, -2.0 ** -20, 1.5, NAN):
        assert case(rho=rho) == E
    assert case(ad=17) == E
    assert case(ad=0) == E
    assert case(n=0) == E
    assert case(m=0) == E
    assert case(h=0) == E
    assert case(Kk=8193) == E
    assert case(Kk=-1) == E
    for pair in (("mean_out", "mean"), ("std_out", "std"), ("mean_out", "std"), ("a_clip", "z"), ("seq", "kept")):
        assert case(alias=pair) == E, pair
    for name in ("mean", "std", "kept", "kc", "shift", "sigma0", "low", "high", "mean_out", "std_out", "a_clip"):
        assert case(null=name) == E, name


def test_refit_argument_errors_write_nothing():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(13)
    E = _lib.L2A_EINVAL

    def case(n=9, m=2, h=3, ad=4, K=3, Kk=2, alpha=0.1, **kw):
        inp = refit_inputs(rs, n, m, h, ad, K, Kk, alpha=alpha)
        dev = upload_refit(inp)
        rc = run_refit(ctx, dev, inp, expect_rc=E, what="n=%d ad=%d K=%d Kk=%d alpha=%g %s" % (n, ad, K, Kk, alpha, kw), **kw)
        for k in ("returns", "a_clip", "low", "high"):
            _same_on_device(dev[k], inp[k], k)
        return rc

    for alpha in (1.0, -2.0 ** -20, NAN):
        assert case(alpha=alpha) == E
    assert case(ad=17) == E
    assert case(ad=0) == E
    assert case(n=0) == E
    assert case(m=0) == E
    assert case(h=0) == E
    assert case(n=1, m=65536, h=1, ad=1, K=1, Kk=1) == E
    assert case(K=0, Kk=0) == E
    assert case(K=8193) == E
    assert case(K=3, Kk=4) == E
    assert case(Kk=-1) == E
    for pair in (("mean", "std"), ("kept", "a_clip"), ("out", "returns"), ("kc", "work")):
        assert case(alias=pair) == E, pair
    for name in ("returns", "a_clip", "low", "high", "work", "mean", "std", "kept", "kc", "out"):
        assert case(null=name) == E, name


def test_refit_lds_limit_in_n():
    """The budget is stated: ``n_it * 4`` bytes (the ranking) and ``K * 4 + L2A_ICEM_REFIT_STATIC_LDS`` (the statistics) within the
    device's ``lds_per_block``; ``K <= 8192`` keeps the second inside any LDS of 34 KiB or more, so the edge is in ``n_it``.  The
    largest ``n_it`` that fits runs and is right (64 valid candidates among NaN, so that the restatement stays small); one more is
    refused with nothing written."""
    ctx = _lib.Context.get(0)
    lds = int(ctx.info()["lds_per_block"])
    n0 = lds // 4
    assert 8192 * 4 + ir.REFIT_STATIC_LDS <= lds
    rs = np.random.RandomState(14)
    worst = Worst()
    for n in (n0, n0 + 1):
        returns = np.full((1, n), np.nan, dtype=np.float32)
        returns[0, rs.choice(n, size=64, replace=False)] = rs.randn(64).astype(np.float32)
        returns[0, n - 1] = 100.0
        inp = refit_inputs(rs, n, 1, 1, 2, 8, 3, returns=returns)
        dev = upload_refit(inp)
        what = "refit at the LDS limit n=%d" % n
        if n == n0:
            ref = check_refit(run_refit(ctx, dev, inp, what=what), inp, worst, what)
            assert ref["index"][0] == n - 1
        else:
            assert run_refit(ctx, dev, inp, expect_rc=_lib.L2A_EINVAL, what=what) == _lib.L2A_EINVAL
    worst.report("icem refit n=%d (LDS limit)" % n0)
