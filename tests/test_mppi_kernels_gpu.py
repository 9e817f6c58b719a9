"""The two reward-weighted (MPPI) planner kernels of ``csrc/l2a_mppi.hip`` (``l2a_mppi_sample_k``, ``l2a_mppi_update_k``) against
``tests/mppi_reference.py``, a plain NumPy restatement pinned by ``tests/test_mppi_reference.py``.  The C entry points are called
directly; every output starts from a sentinel and sits between 64 guard words (``test_cem_kernels_gpu._Out``); the inputs are checked
unchanged.

Bounds (derived, none measured and then set): samples from injected normals bit for bit (``sample_f32``: the kernel's operation
order in ``np.float32`` arithmetic); samples from the Philox stream within ``PHILOX_ATOL sigma_k + 4 2^-24 (|mu'| + U / beta)`` of
the float64 restatement fed the float64 Box-Muller normals; the update's index, valid count and ``Rmax`` exact, its mean and
effective sample size within ``mppi_reference.update_bounds``.  Every test prints the worst error / bound ratio it saw (``-s``)."""

import ctypes

import numpy as np
import pytest

import mppi_pass_cases as pc
import mppi_reference as mr
from learning_to_adapt_amd import _lib
from test_cem_kernels_gpu import PHILOX_ATOL, Worst, _Out, _ull, _up, returns_pattern

pytestmark = pytest.mark.gpu

NAN = float("nan")
PATTERNS = ("distinct", "three", "equal", "nan", "ninf", "pinf", "pm_inf", "one_finite", "zeros", "denormal", "overflow", "cluster",
            "mixed")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _bounds(ad):
    return np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)


def _same_on_device(dev, host, what):
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(host)), "input changed: " + what


# ---------------------------------------------------------------------------------------------------------------------- harness
def run_sample(ctx, inp, with_seq=True, expect_rc=_lib.L2A_OK, alias=False):
    """One ``l2a_mppi_sample`` call; returns ``mean_out`` / ``a_clip`` / ``seq`` as host arrays (guards checked).  With an error
    expected: every output must still hold its sentinel."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad = inp["n"], inp["m"], inp["h"], inp["ad"]
    D = h * ad
    what = "sample n=%d m=%d h=%d ad=%d beta=%g shift=%s inject=%d seq=%d" % (n, m, h, ad, inp["beta"], list(inp["shift"]),
                                                                            inp["z"] is not None, with_seq)
    keys = ("mean", "shift", "sigma", "low", "high", "z")
    dev = {k: (_up(inp[k]) if inp[k] is not None else None) for k in keys}
    out = dict(mean_out=_Out((m, D), torch.float32, NAN), a_clip=_Out((n, m, D), torch.float32, NAN),
               seq=_Out((h, m * n, ad), torch.float32, NAN))
    mean_out_ptr = _ptr(dev["mean"]) if alias else out["mean_out"].ptr()
    rc = ctx.lib.l2a_mppi_sample(ctx.handle, _ptr(dev["z"]), _ull(inp.get("seed", 0)), _ull(inp.get("off", 0)), _ptr(dev["mean"]),
                                 _ptr(dev["shift"]), _ptr(dev["sigma"]), float(inp["beta"]), _ptr(dev["low"]), _ptr(dev["high"]),
                                 n, m, h, ad, mean_out_ptr, out["a_clip"].ptr(), out["seq"].ptr() if with_seq else None,
                                 _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    host = {k: o.host(k + " " + what) for k, o in out.items()}
    for k in keys:
        if inp[k] is not None:
            _same_on_device(dev[k], inp[k], k + " " + what)
    if expect_rc != _lib.L2A_OK:
        assert all(np.isnan(v).all() for v in host.values()), "output written by a refused call: " + what
        return rc
    if not with_seq:
        assert np.isnan(host["seq"]).all(), "seq written though NULL was passed: " + what
    return host


def sample_inputs(rs, n, m, h, ad, beta, shift, inject=True, zero_sigma=None, seed=0, off=0):
    D = h * ad
    low, high = _bounds(ad)
    sigma = (0.1 + 0.5 * rs.rand(ad)).astype(np.float32)
    if zero_sigma is not None:
        sigma[zero_sigma] = 0.0
    mean = (0.7 * rs.randn(m, D)).astype(np.float32)            # beyond both bounds in some dimensions
    z = rs.randn(n, m, D).astype(np.float32) if inject else None
    return dict(n=n, m=m, h=h, ad=ad, beta=beta, shift=np.asarray(shift, dtype=np.int32), mean=mean, sigma=sigma, low=low, high=high,
                z=z, seed=seed, off=off)


def run_update(ctx, dev, n, m, h, ad, kappa, mean0, expect_rc=_lib.L2A_OK, what=""):
    """One ``l2a_mppi_update`` call on uploaded ``dev['returns']`` / ``dev['a_clip']``; returns ``mean`` / ``out`` host arrays."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    D = h * ad
    mean = _Out((m, D), torch.float32, NAN, init=_up(mean0))
    out = _Out((m, ad + 4), torch.float32, NAN)
    rc = ctx.lib.l2a_mppi_update(ctx.handle, _ptr(dev["returns"]), _ptr(dev["a_clip"]), n, m, h, ad, float(kappa), mean.ptr(), out.ptr(),
                                 _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    got = dict(mean=mean.host("mean " + what), out=out.host("out " + what))
    if expect_rc != _lib.L2A_OK:
        assert np.array_equal(_bits(got["mean"]), _bits(mean0)) and np.isnan(got["out"]).all(), "output written by a refused call: " + what
        return rc
    return got


def check_update(got, returns, a_clip, mean0, n, m, h, ad, kappa, worst, what):
    ref = mr.result_row(mean0, a_clip, returns, kappa, ad)
    row = got["out"]
    idx = _bits(row[:, ad + 1].copy())
    valid = _bits(row[:, ad + 3].copy())
    assert np.array_equal(idx, ref["index"].astype(np.int32)), "index %s != %s: %s" % (idx, ref["index"], what)
    assert np.array_equal(valid, ref["valid"].astype(np.int32)), "valid %s != %s: %s" % (valid, ref["valid"], what)
    rmax = row[:, ad].copy()
    live = ref["valid"] > 0
    assert np.array_equal(_bits(rmax[live]), _bits(ref["rmax"][live])), "Rmax differs: " + what
    assert np.isnan(rmax[~live]).all(), what
    assert np.array_equal(_bits(got["mean"][~live]), _bits(mean0[~live])), "a degenerate env's mean was touched: " + what
    assert np.array_equal(_bits(row[:, :ad].copy()), _bits(got["mean"][:, :ad].copy())), "the result row's action is not mu[i, 0, :]: " + what
    assert np.all(row[~live, ad + 2] == 0.0), what
    assert np.isfinite(got["mean"]).all(), what
    B = float(np.max(np.abs(a_clip)))
    mean_bound, rel = mr.update_bounds(n, kappa, B, mr.sum_chain(n))
    if live.any():
        r = worst.note("mean", np.abs(got["mean"][live].astype(np.float64) - ref["mean"][live]), mean_bound)
        assert r <= 1.0, "mean off by %.3f of its bound %.3e: %s" % (r, mean_bound, what)
        r = worst.note("ess", np.abs(row[live, ad + 2].astype(np.float64) - ref["ess"][live]), rel * ref["ess"][live])
        assert r <= 1.0, "ESS off by %.3f of its bound: %s" % (r, what)


# ------------------------------------------------------------------------------------------------- sample with injected normals
SAMPLE_N = (1, 2, 63, 64, 65, 257)
SHIFTS3 = ([-1, 1, 0], [1, 0, -1], [0, -1, 1], [1, 1, 1], [0, 0, 0], [-1, -1, 1])


@pytest.mark.parametrize("beta", [1.0, 0.6, 2.0 ** -10])
@pytest.mark.parametrize("ad", [1, 6, 16])
@pytest.mark.parametrize("h", [1, 2, 7])
def test_sample_with_injected_normals_bit_for_bit(h, ad, beta):
    """``mean_out``, ``a_clip`` and ``seq`` equal ``sample_f32`` bit for bit: mixed shift vectors (all three values in one call at
    m = 3), one dimension with sigma = 0, means beyond both bounds, with and without ``seq``."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(1000 * h + 10 * ad + int(beta * 7))
    c = 0
    on_low = on_high = False
    for n in SAMPLE_N:
        for m in (1, 3):
            shift = SHIFTS3[c % 6] if m == 3 else [(-1, 1, 0)[c % 3]]
            zero_sigma = (c % ad) if c % 2 == 0 else None
            with_seq = c % 4 != 3
            c += 1
            inp = sample_inputs(rs, n, m, h, ad, beta, shift, zero_sigma=zero_sigma)
            got = run_sample(ctx, inp, with_seq=with_seq)
            want_mean, want_a, want_seq = mr.sample_f32(inp["mean"], inp["shift"], inp["z"], inp["sigma"], beta, inp["low"],
                                                        inp["high"], n, m, h, ad)
            what = "n=%d m=%d h=%d ad=%d beta=%g shift=%s" % (n, m, h, ad, beta, shift)
            assert np.array_equal(_bits(got["mean_out"]), _bits(want_mean)), "mean_out: " + what
            assert np.array_equal(_bits(got["a_clip"]), _bits(want_a)), "a_clip: " + what
            if with_seq:
                assert np.array_equal(_bits(got["seq"]), _bits(want_seq)), "seq: " + what
            on_low = on_low or bool((want_a == np.tile(inp["low"], h)).any())
            on_high = on_high or bool((want_a == np.tile(inp["high"], h)).any())
    assert on_low and on_high, "no sub-case put a sample on each bound"


@pytest.mark.parametrize("h,ad", pc.SHAPES)
def test_sample_over_a_horizon_of_several_passes(h, ad):
    """The horizon goes through the LDS tiles in passes of ``512 // A`` steps; the filter state, the normal's element index, the
    shifted mean's read ahead and the three stores all cross the pass boundary.  Every case of ``mppi_pass_cases.CASES`` at this
    ``(h, A)`` - the table ``tests/test_mppi_pass_cases.py`` proves to reject a reset state, a clamp at the pass end and a dropped
    ``t0 * A`` - with the table's own seeds: ``mean_out``, ``a_clip`` and ``seq`` equal ``sample_f32`` bit for bit."""
    ctx = _lib.Context.get(0)
    assert h > pc.PASS_STEPS(ad)
    on_low = on_high = False
    mine = [k for k, c in enumerate(pc.CASES) if (c[0], c[1]) == (h, ad)]
    assert len(mine) == pc.PER_SHAPE
    for k in mine:
        _, _, n, m, shift, beta, zero_sigma, with_seq = pc.CASES[k]
        inp = pc.inputs(k)
        got = run_sample(ctx, inp, with_seq=with_seq)
        want_mean, want_a, want_seq = mr.sample_f32(inp["mean"], inp["shift"], inp["z"], inp["sigma"], beta, inp["low"], inp["high"],
                                                    n, m, h, ad)
        what = "case %d: n=%d m=%d h=%d ad=%d beta=%g shift=%s zero_sigma=%s" % (k, n, m, h, ad, beta, shift, zero_sigma)
        assert np.array_equal(_bits(got["mean_out"]), _bits(want_mean)), "mean_out: " + what
        assert np.array_equal(_bits(got["a_clip"]), _bits(want_a)), "a_clip: " + what
        if with_seq:
            assert np.array_equal(_bits(got["seq"]), _bits(want_seq)), "seq: " + what
        on_low = on_low or bool((want_a == np.tile(inp["low"], h)).any())
        on_high = on_high or bool((want_a == np.tile(inp["high"], h)).any())
    assert on_low and on_high, "no sub-case put a sample on each bound"


# ---------------------------------------------------------------------------------------------------- sample with Philox normals
@pytest.mark.parametrize("off", [0, (1 << 32) - 1000, (1 << 40) + 12345])
def test_sample_with_philox_normals(off):
    """4224 elements per launch (the one at 2^32 - 1000 crosses into the counter's high word) under two seeds against the float64
    restatement fed the float64 Box-Muller normals; two launches over the candidates' halves equal one launch, bit for bit."""
    ctx = _lib.Context.get(0)
    worst = Worst()
    n, m, h, ad = 66, 2, 4, 8
    D = h * ad
    for seed in (0x5EED0000ABCD1234, 1):
        for beta in (0.6, 1.0):
            rs = np.random.RandomState(7)
            inp = sample_inputs(rs, n, m, h, ad, beta, [1, 0], inject=False, zero_sigma=3, seed=seed, off=off)
            got = run_sample(ctx, inp)
            what = "seed=%#x offset=%#x beta=%g" % (seed, off, beta)
            z = mr.philox_normal(seed, mr.philox_indices(off, n * m * D)).reshape(n, m, D)
            want_mean, want_a, want_seq = mr.sample(inp["mean"], inp["shift"], z, inp["sigma"], beta, inp["low"], inp["high"], n, m, h, ad)
            assert np.array_equal(got["mean_out"].astype(np.float64), want_mean), what
            sig = np.tile(inp["sigma"].astype(np.float64), h)
            U = float(np.max(np.abs(z * sig)))
            bound = PHILOX_ATOL * sig[None, None] + 4 * 2.0 ** -24 * (np.abs(want_mean)[None] + U / float(np.float32(beta)))
            r = worst.note("a_clip", np.abs(got["a_clip"].astype(np.float64) - want_a), np.broadcast_to(bound, want_a.shape))
            assert r <= 1.0, "a_clip off by %.3f of its bound: %s" % (r, what)
            assert np.array_equal(_bits(got["seq"]), _bits(got["a_clip"]).reshape(-1)[mr.seq_index(n, m, h, ad)]), what
            halves = []
            for part in range(2):           # offsets advance by rows
                half = dict(inp, n=n // 2, off=off + part * (n // 2) * m * D)
                g2 = run_sample(ctx, half)
                assert np.array_equal(_bits(g2["mean_out"]), _bits(got["mean_out"])), what
                halves.append(g2["a_clip"])
            assert np.array_equal(_bits(np.concatenate(halves)), _bits(got["a_clip"])), "two half launches differ from one: " + what
    worst.report("mppi Philox offset=%#x" % off)


@pytest.mark.parametrize("off", [0, (1 << 32) - 1000, (1 << 40) + 12345])
@pytest.mark.parametrize("n,m,h,ad", [(6, 2, 40, 16), (5, 3, 90, 6)])
def test_sample_with_philox_normals_over_several_passes(n, m, h, ad, off):
    """Two passes (32 + 8 steps at A = 16, 85 + 5 at A = 6): the Philox counter of an element picks up ``t0 * A`` in the second
    one.  Against the float64 restatement fed the float64 Box-Muller normals under two seeds, within the bound of
    ``test_sample_with_philox_normals``, which does not depend on ``h``: a step's normal is off by at most ``PHILOX_ATOL sigma_k``
    and the filter's weights ``beta (1 - beta)^(t - s)`` sum to at most 1, so that term does not grow; the recurrence
    ``nz = beta u + (1 - beta) nz`` rounds three times per step (``|nz| <= U``), and the roundings of earlier steps are damped by
    ``1 - beta`` per step - a geometric sum of at most ``2 2^-24 U / beta``; the last add and ``mu'`` itself take the rest.  Two
    launches over the candidates' halves equal one launch, bit for bit."""
    ctx = _lib.Context.get(0)
    worst = Worst()
    D = h * ad
    assert h > pc.PASS_STEPS(ad)
    shift = [1, 0, -1][:m]
    for seed in (0x5EED0000ABCD1234, 1):
        for beta in (0.6, 1.0):
            rs = np.random.RandomState(7)
            inp = sample_inputs(rs, n, m, h, ad, beta, shift, inject=False, zero_sigma=3, seed=seed, off=off)
            got = run_sample(ctx, inp)
            what = "n=%d m=%d h=%d ad=%d seed=%#x offset=%#x beta=%g" % (n, m, h, ad, seed, off, beta)
            z = mr.philox_normal(seed, mr.philox_indices(off, n * m * D)).reshape(n, m, D)
            want_mean, want_a, want_seq = mr.sample(inp["mean"], inp["shift"], z, inp["sigma"], beta, inp["low"], inp["high"], n, m, h, ad)
            assert np.array_equal(got["mean_out"].astype(np.float64), want_mean), what
            sig = np.tile(inp["sigma"].astype(np.float64), h)
            U = float(np.max(np.abs(z * sig)))
            bound = PHILOX_ATOL * sig[None, None] + 4 * 2.0 ** -24 * (np.abs(want_mean)[None] + U / float(np.float32(beta)))
            r = worst.note("a_clip", np.abs(got["a_clip"].astype(np.float64) - want_a), np.broadcast_to(bound, want_a.shape))
            assert r <= 1.0, "a_clip off by %.3f of its bound: %s" % (r, what)
            assert np.array_equal(_bits(got["seq"]), _bits(got["a_clip"]).reshape(-1)[mr.seq_index(n, m, h, ad)]), what
            halves = []
            for lo, hi in ((0, n // 2), (n // 2, n)):           # offsets advance by rows
                half = dict(inp, n=hi - lo, off=off + lo * m * D)
                g2 = run_sample(ctx, half)
                assert np.array_equal(_bits(g2["mean_out"]), _bits(got["mean_out"])), what
                halves.append(g2["a_clip"])
            assert np.array_equal(_bits(np.concatenate(halves)), _bits(got["a_clip"])), "two half launches differ from one: " + what
    worst.report("mppi Philox several passes n=%d m=%d h=%d ad=%d offset=%#x" % (n, m, h, ad, off))


# ------------------------------------------------------------------------------------------------------------------------ update
UPDATE_N = (1, 2, 63, 64, 65, 511, 513, 4097)
UPDATE_D = ((1, 1), (31, 1), (2, 16), (3, 11), (30, 6))
KAPPAS = (2.0 ** -10, 1.0, 1e3)


@pytest.mark.parametrize("h,ad", UPDATE_D)
@pytest.mark.parametrize("n", UPDATE_N)
def test_update_over_shapes_temperatures_and_return_patterns(n, h, ad):
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n * 37 + h * ad)
    worst = Worst()
    D = h * ad
    low, high = _bounds(ad)
    for m in (1, 3):
        a_clip = np.clip((0.2 + 0.6 * rs.randn(n, m, D)).astype(np.float32), np.tile(low, h), np.tile(high, h))
        mean0 = (0.3 * rs.randn(m, D)).astype(np.float32)
        a_dev = _up(a_clip)
        for pattern in PATTERNS:
            returns = returns_pattern(pattern, rs, m, n)
            dev = dict(returns=_up(returns), a_clip=a_dev)
            for kappa in KAPPAS:
                what = "update n=%d m=%d h=%d ad=%d kappa=%g %s" % (n, m, h, ad, kappa, pattern)
                got = run_update(ctx, dev, n, m, h, ad, kappa, mean0, what=what)
                check_update(got, returns, a_clip, mean0, n, m, h, ad, kappa, worst, what)
            _same_on_device(dev["returns"], returns, "returns n=%d %s" % (n, pattern))
        _same_on_device(a_dev, a_clip, "a_clip n=%d m=%d" % (n, m))
    worst.report("mppi update n=%d D=%d" % (n, D))


def test_update_is_deterministic_and_equal_across_an_envs_workgroups():
    """The same inputs give the same bits run after run; envs with equal returns and samples (six workgroups each) get equal rows."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(11)
    n, m, h, ad = 513, 2, 30, 6
    D = h * ad
    one = rs.uniform(-1, 1, size=(n, 1, D)).astype(np.float32)
    a_clip = np.ascontiguousarray(np.broadcast_to(one, (n, m, D)))
    returns = np.ascontiguousarray(np.broadcast_to((rs.randn(1, n) * 3).astype(np.float32), (m, n)))
    mean0 = np.zeros((m, D), dtype=np.float32)
    dev = dict(returns=_up(returns), a_clip=_up(a_clip))
    runs = [run_update(ctx, dev, n, m, h, ad, 1.0, mean0) for _ in range(3)]
    for g in runs[1:]:
        assert np.array_equal(_bits(g["mean"]), _bits(runs[0]["mean"])) and np.array_equal(_bits(g["out"]), _bits(runs[0]["out"]))
    assert np.array_equal(_bits(runs[0]["mean"][0]), _bits(runs[0]["mean"][1]))
    assert np.array_equal(_bits(runs[0]["out"][0]), _bits(runs[0]["out"][1]))


# --------------------------------------------------------------------------------------------------------------- argument errors
def test_sample_argument_errors_write_nothing():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(12)
    for beta in (0.0, -0.5, 1.0 + 2.0 ** -20, NAN):
        assert run_sample(ctx, sample_inputs(rs, 5, 2, 3, 4, beta, [0, 1]), expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_sample(ctx, sample_inputs(rs, 5, 2, 3, 17, 0.6, [0, 1]), expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_sample(ctx, sample_inputs(rs, 5, 2, 3, 4, 0.6, [0, 1]), expect_rc=_lib.L2A_EINVAL, alias=True) == _lib.L2A_EINVAL


def test_update_argument_errors_write_nothing():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(13)

    def refused(n, m, h, ad, kappa):
        a_clip = rs.uniform(-1, 1, size=(n, m, h * ad)).astype(np.float32)
        dev = dict(returns=_up(rs.randn(m, n).astype(np.float32)), a_clip=_up(a_clip))
        mean0 = rs.randn(m, h * ad).astype(np.float32)
        return run_update(ctx, dev, n, m, h, ad, kappa, mean0, expect_rc=_lib.L2A_EINVAL, what="n=%d ad=%d kappa=%g" % (n, ad, kappa))

    for kappa in (0.0, -1.0, float("inf"), NAN):
        assert refused(5, 2, 3, 4, kappa) == _lib.L2A_EINVAL
    assert refused(5, 2, 3, 17, 1.0) == _lib.L2A_EINVAL


def test_update_lds_limit_in_n():
    """The budget is stated: ``n * 4`` bytes plus ``L2A_MPPI_UPDATE_STATIC_LDS`` within the device's ``lds_per_block``.  The largest
    ``n`` that fits runs and is right; one more is refused with nothing written."""
    ctx = _lib.Context.get(0)
    lds = int(ctx.info()["lds_per_block"])
    n0 = (lds - mr.UPDATE_STATIC_LDS) // 4
    assert n0 * 4 + mr.UPDATE_STATIC_LDS <= lds < (n0 + 1) * 4 + mr.UPDATE_STATIC_LDS
    rs = np.random.RandomState(14)
    worst = Worst()
    for n in (n0, n0 + 1):
        a_clip = rs.uniform(-1, 1, size=(n, 1, 2)).astype(np.float32)
        returns = rs.randn(1, n).astype(np.float32)
        mean0 = np.zeros((1, 2), dtype=np.float32)
        dev = dict(returns=_up(returns), a_clip=_up(a_clip))
        what = "update at the LDS limit n=%d" % n
        if n == n0:
            check_update(run_update(ctx, dev, n, 1, 1, 2, 1.0, mean0, what=what), returns, a_clip, mean0, n, 1, 1, 2, 1.0, worst, what)
        else:
            assert run_update(ctx, dev, n, 1, 1, 2, 1.0, mean0, expect_rc=_lib.L2A_EINVAL, what=what) == _lib.L2A_EINVAL
    worst.report("mppi update n=%d (LDS limit)" % n0)
