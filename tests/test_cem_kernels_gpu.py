"""The five cross-entropy-method kernels of ``csrc/l2a_cem.hip`` (``l2a_cem_sample_k``, ``l2a_cem_rank_k``, ``l2a_cem_stats_k``, the
fused ``l2a_cem_refit_sample_k``, ``l2a_cem_pick_k``) against ``tests/cem_reference.py``, a plain float64 restatement pinned by
``tests/test_cem_reference.py``.  The C entry points are called directly; every output starts from a sentinel (NaN / -7) and sits
between 64 guard words; every case runs both readings, and wherever a refit is involved all three ways through the library:
``l2a_cem_refit`` + ``l2a_cem_sample``, ``l2a_cem_refit_sample`` with distinct buffers, and ``l2a_cem_refit_sample`` in place.
Each way is compared with the reference, never with another way (``tests/test_cem_refit_sample.py`` does that, bit for bit).

Bounds (derived, ``cem_reference.stats_bounds``): elite rows exact; ``|mean - ref| <= gamma B`` and ``|std - ref| <= 2 gamma B``
with ``gamma = (ceil(cnt / 32) + 16) 2^-24`` and ``B`` the largest input magnitude; samples from injected normals within two fp32
roundings, ``2^-23 (|mean| + |z std|)``; the clip and the rollout's candidate tensor bit for bit; Philox normals within 2e-5
absolute of the float64 Box-Muller (the project's bound for the device's fp32 ``logf`` / ``cosf``).  Every test prints the worst
error / bound ratio it saw (``-s`` shows them)."""

import ctypes

import numpy as np
import pytest

import cem_reference as cr
from learning_to_adapt_amd import _lib
from test_cem_refit_sample import _returns

pytestmark = pytest.mark.gpu

GUARD = 64
F_GUARD = 12345.0
I_GUARD = 0x5A5A5A5A
ENTRIES = ("split", "fused", "in_place")
PHILOX_ATOL = 2e-5

PATTERNS = ("distinct", "three", "outlier", "equal", "nan", "ninf", "pinf", "pm_inf", "one_finite", "zeros", "denormal", "overflow",
            "cluster", "mixed")


def returns_pattern(name, rs, m, n):
    """Seeded returns ``[m, n]`` (fp32) of the named kind."""
    if name == "distinct":
        r = rs.randn(m, n) * 10
    elif name == "three":                               # three distinct values only
        r = rs.choice([-1.5, 0.25, 7.0], size=(m, n))
    elif name == "outlier":                             # one value plus a single outlier: almost all of n in one bin
        r = np.full((m, n), 2.5)
        for i in range(m):
            r[i, (n // 2 + i) % n] = 1000.0
    elif name == "equal":
        r = np.full((m, n), 1.5)
    elif name == "nan":
        r = np.full((m, n), np.nan)
    elif name == "ninf":
        r = np.full((m, n), -np.inf)
    elif name == "pinf":
        r = np.full((m, n), np.inf)
    elif name == "pm_inf":
        r = rs.choice([np.inf, -np.inf], size=(m, n))
    elif name == "one_finite":
        r = np.full((m, n), np.nan)
        for i in range(m):
            r[i, (n // 3 + i) % n] = 0.75
    elif name == "zeros":                               # +0.0 and -0.0 interleaved: one tie class
        r = np.where((np.arange(n) + np.arange(m)[:, None]) % 2 == 0, 0.0, -0.0)
    elif name == "denormal":                            # the whole range below the smallest normal for small n: the bin scale is inf
        r = np.stack([1e-40 * rs.permutation(n) for _ in range(m)])
    elif name == "overflow":                            # max - min overflows fp32: the bin scale is 0
        r = rs.uniform(-3e38, 3e38, size=(m, n))
        r[:, 0], r[:, n - 1] = 3e38, -3e38
    elif name == "cluster":                             # a tight cluster: 1e6 + a few ulps, with repeats
        r = (np.float32(1e6) + rs.randint(0, 8, size=(m, n)).astype(np.float32) * np.spacing(np.float32(1e6))).astype(np.float64)
    elif name == "mixed":
        r = _returns(rs, m, n, "mixed")
    else:
        raise KeyError(name)
    return np.ascontiguousarray(r, dtype=np.float32)


# --------------------------------------------------------------------------------------------------------------------- harness
class _Out:
    """A device output of ``shape`` between two runs of guard words, pre-filled with a sentinel (or ``init``)."""

    def __init__(self, shape, dtype, fill, init=None):
        import torch
        self.size = int(np.prod(shape))
        self.guard = I_GUARD if dtype is torch.int32 else F_GUARD
        self.flat = torch.full((self.size + 2 * GUARD,), self.guard, dtype=dtype, device="cuda:0")
        self.view = self.flat[GUARD:GUARD + self.size].view(*shape)
        if init is not None:
            self.view.copy_(init)
        else:
            self.view.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def host(self, what):
        h = self.flat.cpu().numpy()
        assert np.all(h[:GUARD] == self.guard) and np.all(h[GUARD + self.size:] == self.guard), "guard words overwritten: " + what
        return h[GUARD:GUARD + self.size].reshape(tuple(self.view.shape)).copy()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ull(x):
    return ctypes.c_ulonglong(int(x) & 0xFFFFFFFFFFFFFFFF)


def make_inputs(rs, n, m, h, ad, k, reference, alpha, lo, hi, pattern="mixed", inject=True, returns=None, a_in=None, mean0=None,
                seed=0x5EED0000ABCD1234, off=977):
    """One CEM iteration boundary's inputs (host arrays)."""
    D = h * ad
    low, high = np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)
    if returns is None:
        returns = returns_pattern(pattern, rs, m, n)
    if a_in is None:                                    # samples as an iteration leaves them: clipped, many at a bound
        a_in = cr.clip((0.2 + 0.6 * rs.randn(n, m, D)).astype(np.float32), low, high, h)
    if mean0 is None:
        mean0 = (0.3 * rs.randn(m, D)).astype(np.float32)
    z = rs.randn(n, m, D).astype(np.float32) if inject else None
    return dict(n=n, m=m, h=h, ad=ad, D=D, k=k, reference=bool(reference), alpha=float(alpha), lo=lo, hi=hi, returns=returns,
                a_in=np.ascontiguousarray(a_in, dtype=np.float32), mean0=np.ascontiguousarray(mean0, dtype=np.float32), z=z, low=low,
                high=high, seed=seed, off=off, pattern=pattern)


def describe(inp, entry=""):
    return "%s n=%d m=%d h=%d ad=%d k=%d reference=%d alpha=%g shard=(%d, %d) inject=%d %s" % (
        entry, inp["n"], inp["m"], inp["h"], inp["ad"], inp["k"], inp["reference"], inp["alpha"], inp["lo"], inp["hi"],
        inp["z"] is not None, inp["pattern"])


def upload(inp):
    return {key: (_up(inp[key]) if inp[key] is not None else None) for key in ("returns", "a_in", "mean0", "z", "low", "high")}


def run_boundary(ctx, inp, dev, entry, expect_rc=_lib.L2A_OK):
    """One iteration boundary through ``entry``; returns the outputs as host arrays (guards checked), or the return code when
    ``expect_rc`` is an error (then: no output may have been written)."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    lib = ctx.lib
    n, m, h, ad, D, k, ref = inp["n"], inp["m"], inp["h"], inp["ad"], inp["D"], inp["k"], int(inp["reference"])
    lo, hi = inp["lo"], inp["hi"]
    nsel = hi - lo
    stream = _stream_ptr(torch.device("cuda:0"))
    nan = float("nan")
    in_place = entry == "in_place"
    out = dict(rows=_Out((m * k,), torch.int32, -7),
               mean=_Out((m, D), torch.float32, nan, init=None if entry == "fused" else dev["mean0"]),
               std=_Out((m, D), torch.float32, nan),
               a_clip=_Out((n, m, D), torch.float32, nan, init=dev["a_in"] if in_place else None),
               a_raw=_Out((n, m, D), torch.float32, nan),
               seq=_Out((h, m * nsel, ad), torch.float32, nan))
    seq_ptr = out["seq"].ptr() if nsel > 0 else None
    what = describe(inp, entry)
    if entry == "split":
        rc = lib.l2a_cem_refit(ctx.handle, _ptr(dev["returns"]), _ptr(dev["a_in"]), n, m, D, k, ref, inp["alpha"], out["rows"].ptr(),
                               out["mean"].ptr(), out["std"].ptr(), stream)
        if rc == _lib.L2A_OK and expect_rc == _lib.L2A_OK:
            rc = lib.l2a_cem_sample(ctx.handle, _ptr(dev["z"]), _ull(inp["seed"]), _ull(inp["off"]), out["mean"].ptr(), out["std"].ptr(),
                                    _ptr(dev["low"]), _ptr(dev["high"]), n, m, h, ad, ref, lo, hi, out["a_clip"].ptr(),
                                    out["a_raw"].ptr(), seq_ptr, stream)
    else:
        src = out["a_clip"].ptr() if in_place else _ptr(dev["a_in"])
        mean_in = None if in_place else _ptr(dev["mean0"])
        rc = lib.l2a_cem_refit_sample(ctx.handle, _ptr(dev["returns"]), src, n, m, h, ad, k, ref, inp["alpha"], _ptr(dev["z"]),
                                      _ull(inp["seed"]), _ull(inp["off"]), _ptr(dev["low"]), _ptr(dev["high"]), lo, hi,
                                      out["rows"].ptr(), mean_in, out["mean"].ptr(), out["std"].ptr(), out["a_clip"].ptr(),
                                      out["a_raw"].ptr(), seq_ptr, stream)
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, lib.l2a_last_error(ctx.handle).decode())
    host = {key: o.host(key + " " + what) for key, o in out.items()}
    for key in ("returns", "a_in", "mean0", "z", "low", "high"):          # the inputs are read only
        if inp[key] is not None:
            assert np.array_equal(dev[key].cpu().numpy().view(np.int32), inp[key].view(np.int32)), "input %s changed: %s" % (key, what)
    if expect_rc != _lib.L2A_OK:
        assert np.all(host["rows"] == -7) and np.isnan(host["std"]).all() and np.isnan(host["a_raw"]).all() and \
            np.isnan(host["seq"]).all(), "output written by a refused call: " + what
        assert np.array_equal(host["mean"].view(np.int32), inp["mean0"].view(np.int32)) or np.isnan(host["mean"]).all(), what
        assert np.isnan(host["a_clip"]).all() or np.array_equal(host["a_clip"].view(np.int32), inp["a_in"].view(np.int32)), what
        return rc
    return host


class Worst:
    """Worst error / bound ratio per quantity."""

    def __init__(self):
        self.ratio = {}

    def note(self, key, err, bound):
        r = float(np.max(err / bound)) if np.size(err) else 0.0
        self.ratio[key] = max(self.ratio.get(key, 0.0), r)
        return r

    def report(self, title):
        print("\n[cem] %s: worst error / bound " % title + ", ".join("%s %.3f" % kv for kv in sorted(self.ratio.items())))


def check_samples(got, inp, mean, std, worst, what):
    """``a_raw`` / ``a_clip`` / ``seq`` of a launch that drew with the fp32 ``mean`` / ``std`` (the library's own) against the reference."""
    n, m, h, ad, D, ref, lo, hi = inp["n"], inp["m"], inp["h"], inp["ad"], inp["D"], inp["reference"], inp["lo"], inp["hi"]
    for key in ("a_raw", "a_clip", "seq"):
        assert np.isfinite(got[key]).all(), "%s holds its sentinel or a non-finite value: %s" % (key, what)
    slack = 0.0
    if inp["z"] is not None:
        z = inp["z"].astype(np.float64)
    else:       # the library's Philox normals: each within 2e-5 of the float64 Box-Muller
        z = cr.philox_normal(inp["seed"], cr.philox_indices(inp["off"], n * m * D)).reshape(n, m, D)
        slack = PHILOX_ATOL * np.abs(std.astype(np.float64))[None]
    want_raw, _, _ = cr.sample(mean, std, z, inp["low"], inp["high"], n, m, h, ad, ref, lo, hi)
    bound = 2.0 ** -23 * (np.abs(mean.astype(np.float64))[None] + np.abs(z * std.astype(np.float64)[None])) + slack
    err = np.abs(got["a_raw"].astype(np.float64) - want_raw)
    # (a bound of 0 - mean 0 and std 0 - demands the exact 0)
    r = worst.note("a_raw", np.where(bound > 0, err, np.where(err > 0, 2.0, 0.0)), np.where(bound > 0, bound, 1.0))
    assert r <= 1.0, "a_raw off by %.3f of its bound: %s" % (r, what)
    want_clip = cr.clip(got["a_raw"], inp["low"], inp["high"], h)
    assert np.array_equal(got["a_clip"].view(np.int32), want_clip.view(np.int32)), "a_clip is not clip(a_raw): " + what
    src = got["a_raw"] if ref else got["a_clip"]
    idx = cr.seq_index(n, m, h, ad, ref, lo, hi)
    assert np.array_equal(got["seq"].view(np.int32), src.reshape(-1).view(np.int32)[idx]), "seq is not the reading's permutation: " + what


def check_boundary(got, inp, worst, what):
    """Every output of one iteration boundary against the float64 reference."""
    m, k, ref = inp["m"], inp["k"], inp["reference"]
    want_mean, want_std, want_rows = cr.refit(inp["mean0"], inp["a_in"], inp["returns"], k, inp["alpha"], ref)
    rows = got["rows"].reshape(m, k)
    if ref:
        assert np.array_equal(np.sort(rows, axis=1), np.sort(want_rows, axis=1)), "elite positions differ: " + what
    else:
        assert np.array_equal(rows, want_rows), "elite rows differ: " + what
    mean_bound, std_bound = cr.stats_bounds(m * k if ref else k, inp["a_in"], inp["mean0"])
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all(), what
    r = worst.note("mean", np.abs(got["mean"].astype(np.float64) - want_mean), mean_bound)
    assert r <= 1.0, "mean off by %.3f of its bound %.3e: %s" % (r, mean_bound, what)
    r = worst.note("std", np.abs(got["std"].astype(np.float64) - want_std), std_bound)
    assert r <= 1.0, "std off by %.3f of its bound %.3e: %s" % (r, std_bound, what)
    check_samples(got, inp, got["mean"], got["std"], worst, what)


def run_and_check(ctx, inp, worst, entries=ENTRIES):
    dev = upload(inp)
    for entry in entries:
        check_boundary(run_boundary(ctx, inp, dev, entry), inp, worst, describe(inp, entry))


SHARDS = (lambda n: (0, n), lambda n: (0, 1), lambda n: (n - 1, n), lambda n: (n // 3, 2 * n // 3), lambda n: (n // 2, n // 2))


# ------------------------------------------------------------------------------------------------------------------------ rank
RANK_N = (1, 2, 63, 64, 65, 127, 129, 511, 513, 1025, 4097)
RANK_CASES = sorted({(n, p) for n in (65, 513, 4097) for p in PATTERNS} | {(n, p) for n in RANK_N for p in ("distinct", "three")})


@pytest.mark.parametrize("n,pattern", RANK_CASES)
def test_rank_matches_stable_argsort(n, pattern):
    """Elite rows exact: n > 1024 wraps l2a_cem_rank_k's 1024 waves, n > 512 strides the fused launch's threads; ties, one-bin
    populations, +-inf / NaN envs, -0.0, denormal and overflowing ranges."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n * 31 + PATTERNS.index(pattern))
    worst = Worst()
    c = 0
    for m in (1, 3):
        returns = returns_pattern(pattern, rs, m, n)
        for k in sorted({min(max(x, 1), n) for x in (1, 2, n // 10, n - 1, n)}):
            for reference in (True, False):
                if (m if reference else 1) * k > 8192:
                    continue                            # (refused: test_one_row_beyond_the_lds_array_is_refused)
                lo, hi = SHARDS[c % 5](n)
                c += 1
                inp = make_inputs(rs, n, m, 1, 2, k, reference, 0.1, lo, hi, pattern=pattern, returns=returns)
                run_and_check(ctx, inp, worst)
    worst.report("rank n=%d %s" % (n, pattern))


# ------------------------------------------------------------------------------------------------------------------ statistics
SHAPES_D = ((1, 1), (1, 31), (4, 8), (3, 11), (5, 13), (30, 6))        # (h, act_dim): D = 1, 31, 32, 33, 65, 180
ALPHAS = (0.0, 0.1, 1.0)


@pytest.mark.parametrize("cnt", [1, 7, 8, 9, 24, 25, 31, 32, 33, 40, 57, 64, 65])
def test_statistics_at_the_ends_of_the_accumulator_loop(cnt):
    """One env, ``cnt`` elites: every tail length of the four-accumulator loop (``q + 24 < cnt``), crossed with two widths ``D``."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(500 + cnt)
    worst = Worst()
    c = cnt
    for reference in (True, False):
        for rep in range(2):
            h, ad = SHAPES_D[c % 6]
            n = cnt + (0 if rep == 0 else 5 + cnt % 3)
            lo, hi = SHARDS[c % 5](n)
            inp = make_inputs(rs, n, 1, h, ad, cnt, reference, ALPHAS[c % 3], lo, hi, pattern="distinct", inject=(c % 2 == 0))
            run_and_check(ctx, inp, worst)
            c += 1
    worst.report("statistics cnt=%d" % cnt)


@pytest.mark.parametrize("h,ad", SHAPES_D)
def test_statistics_over_dimension_blocks_and_pooled_envs(h, ad):
    """``D`` on both sides of l2a_cem_stats_k's 32-dimension workgroups, three envs pooled (33 and 99 rows) or on their own."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(600 + h * ad)
    worst = Worst()
    c = h + ad
    for k in (11, 33):
        for reference in (True, False):
            n = 70
            lo, hi = SHARDS[c % 5](n)
            inp = make_inputs(rs, n, 3, h, ad, k, reference, ALPHAS[c % 3], lo, hi, pattern="mixed", inject=(c % 2 == 0))
            run_and_check(ctx, inp, worst)
            c += 1
    for reference in (True, False):                     # one env, 65 elites: a full round of the loop plus a tail
        inp = make_inputs(rs, 130, 1, h, ad, 65, reference, 0.1, 0, 130, pattern="three")
        run_and_check(ctx, inp, worst)
    worst.report("statistics D=%d" % (h * ad))


@pytest.mark.parametrize("ad", [1, 6, 63, 64, 65])
def test_statistics_across_the_fused_launch_act_dim_limit(ad):
    """The fused launch gives each action dimension 8 of its 512 threads: ``act_dim`` up to 64 runs fused, 65 is the fallback."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(700 + ad)
    worst = Worst()
    n, m, h, k = 90, 2, 2, 9
    for reference in (True, False):
        assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, n, m, h, ad, k, int(reference)) == (1 if ad <= 64 else 0)
        for alpha in ALPHAS:
            inp = make_inputs(rs, n, m, h, ad, k, reference, alpha, n // 3, 2 * n // 3, pattern="mixed", inject=(alpha != 0.1))
            run_and_check(ctx, inp, worst)
    worst.report("statistics act_dim=%d" % ad)


@pytest.mark.parametrize("reference", [True, False])
def test_statistics_of_elites_all_clipped_to_one_bound(reference):
    """Every elite sits on the upper bound: the true std is 0, the mean the bound."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(41)
    worst = Worst()
    n, m, h, ad = 200, 2, 3, 4
    low, high = np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)
    a_in = cr.clip((5.0 + rs.randn(n, m, h * ad)).astype(np.float32), low, high, h)
    assert np.array_equal(a_in, np.broadcast_to(np.tile(high, h), a_in.shape))
    for k in (20, 57):
        inp = make_inputs(rs, n, m, h, ad, k, reference, 0.1, 0, n, pattern="distinct", a_in=a_in)
        run_and_check(ctx, inp, worst)
    worst.report("statistics clipped elites")


@pytest.mark.parametrize("reference", [True, False])
def test_statistics_of_8192_pooled_rows_and_the_largest_arrays(reference):
    """Exactly the LDS array's 8192 elite rows (m = 2, k = 4096 pooled; per env 4096), and n = 4097, m = 3, D = 180."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(43)
    worst = Worst()
    inp = make_inputs(rs, 4096, 2, 1, 2, 4096, reference, 0.1, 0, 4096, pattern="mixed")
    run_and_check(ctx, inp, worst)
    inp = make_inputs(rs, 4097, 3, 30, 6, 409, reference, 0.1, 1365, 2731, pattern="distinct", inject=False)
    run_and_check(ctx, inp, worst)
    worst.report("statistics 8192 rows / 4097 x 3 x 180")


def test_one_row_beyond_the_lds_array_is_refused():
    """m = 2, k = n = 4097: 8194 pooled rows.  Both entry points return L2A_EINVAL and write nothing; per env (4097 rows) it runs."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(44)
    worst = Worst()
    inp = make_inputs(rs, 4097, 2, 1, 2, 4097, True, 0.1, 0, 4097, pattern="distinct")
    dev = upload(inp)
    for entry in ENTRIES:
        assert run_boundary(ctx, inp, dev, entry, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    inp = make_inputs(rs, 4097, 2, 1, 2, 4097, False, 0.1, 0, 4097, pattern="distinct")
    run_and_check(ctx, inp, worst)
    worst.report("statistics 4097 rows per env")


# --------------------------------------------------------------------------------------------------------------------- samples
def run_sample(ctx, inp, mean, std):
    """``l2a_cem_sample`` alone with the given fp32 ``mean`` / ``std``."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad, D, lo, hi = inp["n"], inp["m"], inp["h"], inp["ad"], inp["D"], inp["lo"], inp["hi"]
    nan = float("nan")
    out = dict(a_clip=_Out((n, m, D), torch.float32, nan), a_raw=_Out((n, m, D), torch.float32, nan),
               seq=_Out((h, m * (hi - lo), ad), torch.float32, nan))
    mean_d, std_d, low_d, high_d = _up(mean), _up(std), _up(inp["low"]), _up(inp["high"])
    z_d = _up(inp["z"]) if inp["z"] is not None else None
    ctx.check(ctx.lib.l2a_cem_sample(ctx.handle, _ptr(z_d), _ull(inp["seed"]), _ull(inp["off"]), _ptr(mean_d), _ptr(std_d), _ptr(low_d),
                                     _ptr(high_d), n, m, h, ad, int(inp["reference"]), lo, hi, out["a_clip"].ptr(), out["a_raw"].ptr(),
                                     out["seq"].ptr() if hi > lo else None, _stream_ptr(torch.device("cuda:0"))), "l2a_cem_sample")
    torch.cuda.synchronize()
    return {key: o.host(key + " " + describe(inp, "sample")) for key, o in out.items()}


@pytest.mark.parametrize("n,m,h,ad", [(37, 3, 5, 4), (257, 1, 1, 1), (64, 2, 3, 7), (1, 2, 2, 3)])
def test_sample_with_injected_normals_over_shards(n, m, h, ad):
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n + m + h + ad)
    worst = Worst()
    for reference in (True, False):
        for shard in SHARDS:
            lo, hi = shard(n)
            if hi > n or lo < 0 or hi < lo:
                continue
            inp = make_inputs(rs, n, m, h, ad, 1, reference, 0.0, lo, hi)
            mean = (0.3 * rs.randn(m, h * ad)).astype(np.float32)
            std = (0.1 + rs.rand(m, h * ad)).astype(np.float32)
            check_samples(run_sample(ctx, inp, mean, std), inp, mean, std, worst, describe(inp, "sample"))
    worst.report("sample n=%d m=%d h=%d ad=%d" % (n, m, h, ad))


@pytest.mark.parametrize("n", [129, 4097])
def test_fused_launch_candidate_slices(n):
    """h = 1 with distinct buffers: the fused launch cuts the candidates into 2 (n = 129) and 64 (n = 4097) slices on a 256-CU
    part, n divisible by neither; every element of every slice must be there, in both readings and under shards."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n)
    worst = Worst()
    c = 0
    for m in (1, 3):
        for reference in (True, False):
            for inject in (True, False):
                lo, hi = SHARDS[c % 5](n)
                c += 1
                inp = make_inputs(rs, n, m, 1, 3, max(n // 10, 1), reference, 0.1, lo, hi, pattern="mixed", inject=inject)
                assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, n, m, 1, 3, inp["k"], int(reference)) == 1
                run_and_check(ctx, inp, worst, entries=("fused",))
    worst.report("slices n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------- Philox
PHILOX_SEEDS = (0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x1234567887654321)
PHILOX_OFFSETS = (0, (1 << 32) - 1000, 1 << 32, (1 << 40) + 12345, 1 << 63)


def _philox_inputs(n, seed, off):
    """m = 1, h = 4, act_dim = 8; wide bounds.  For the fused launch: returns that rank the candidates 0, 1, 2, ..., samples of
    +1 (even rows) and -1 (odd rows), an even elite count, mean 0 and alpha 1 - the refit is mean 0, std 1 exactly."""
    h, ad = 4, 8
    inp = make_inputs(np.random.RandomState(0), n, 1, h, ad, 10, False, 1.0, 0, n, pattern="descending", inject=False,
                      returns=-np.arange(n, dtype=np.float32)[None],
                      a_in=np.broadcast_to(np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None, None], (n, 1, h * ad)),
                      mean0=np.zeros((1, h * ad)), seed=seed, off=off)
    inp["low"], inp["high"] = np.full(ad, -1e9, dtype=np.float32), np.full(ad, 1e9, dtype=np.float32)
    return inp


def _check_normals(got, seed, off, worst, what):
    """Every element of a launch with mean 0, std 1 against the float64 normal of its counter."""
    idx = cr.philox_indices(off, got.size)
    want = cr.philox_normal(seed, idx)
    err = np.abs(got.reshape(-1).astype(np.float64) - want)
    worst.note("normal", err, PHILOX_ATOL)
    bad = np.nonzero(~(err <= PHILOX_ATOL))[0]
    if bad.size:
        u1, u2 = cr.philox_uniforms(seed, idx[bad[:5]])
        raise AssertionError("%s: %d normals beyond %.0e; first: %s" % (what, bad.size, PHILOX_ATOL, [
            dict(element=int(e), counter=int(idx[e]), u1=float(a), u2=float(b), got=float(got.reshape(-1)[e]), want=float(want[e]))
            for e, a, b in zip(bad[:5], u1, u2)]))


@pytest.mark.parametrize("off", PHILOX_OFFSETS)
def test_philox_normals_of_every_element(off):
    """Every element of a launch (4160 of them: the launch at 2^32 - 1000 crosses into the counter's high word) under five seeds,
    through l2a_cem_sample and through the fused launch; two launches at ``off`` and ``off + total`` are one launch of twice the
    candidates, bit for bit."""
    ctx = _lib.Context.get(0)
    worst = Worst()
    n = 130
    for seed in PHILOX_SEEDS:
        inp = _philox_inputs(n, seed, off)
        total = n * inp["D"]
        assert total >= 4000
        zero, one = np.zeros((1, inp["D"]), dtype=np.float32), np.ones((1, inp["D"]), dtype=np.float32)
        what = "seed=%#x offset=%#x" % (seed, off)
        halves = {"sample": [], "fused": []}
        for part in range(2):
            inp = _philox_inputs(n, seed, off + part * total)
            got = run_sample(ctx, inp, zero, one)
            check_samples(got, inp, zero, one, worst, what)
            _check_normals(got["a_clip"], seed, off + part * total, worst, "l2a_cem_sample " + what)
            halves["sample"].append(got["a_clip"])
            assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, n, 1, inp["h"], inp["ad"], inp["k"], 0) == 1
            got = run_boundary(ctx, inp, upload(inp), "fused")
            assert np.all(got["mean"] == 0.0) and np.all(got["std"] == 1.0), what
            check_boundary(got, inp, worst, what)
            _check_normals(got["a_clip"], seed, off + part * total, worst, "l2a_cem_refit_sample " + what)
            halves["fused"].append(got["a_clip"])
        both = _philox_inputs(2 * n, seed, off)
        got = {"sample": run_sample(ctx, both, zero, one)["a_clip"], "fused": run_boundary(ctx, both, upload(both), "fused")["a_clip"]}
        for key in ("sample", "fused"):
            assert np.array_equal(got[key].view(np.int32), np.concatenate(halves[key]).view(np.int32)), key + " " + what
    worst.report("Philox offset=%#x" % off)


# ------------------------------------------------------------------------------------------------- fused / fallback boundary in n
def largest_fused_n(ctx, m, h, ad, reference, upper=40000):
    """Bisect ``l2a_cem_refit_sample_fused`` for the largest fused ``n`` with ``k = n // 10``."""
    fused = lambda n: ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, n, m, h, ad, max(n // 10, 1), int(reference)) == 1  # noqa: E731
    lo, hi = 1, upper
    assert fused(lo) and not fused(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fused(mid):
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("reference", [True, False])
def test_fused_fallback_boundary_in_n(reference):
    """The largest ``n`` the fused launch takes (its LDS budget) and the first one the fallback takes, both against the reference."""
    ctx = _lib.Context.get(0)
    worst = Worst()
    n0 = largest_fused_n(ctx, 1, 2, 2, reference)
    print("\n[cem] largest fused n (m = 1, h = 2, act_dim = 2, k = n // 10, reference = %d): %d" % (reference, n0))
    rs = np.random.RandomState(n0)
    for n in (n0, n0 + 1):
        assert ctx.lib.l2a_cem_refit_sample_fused(ctx.handle, n, 1, 2, 2, n // 10, int(reference)) == (1 if n == n0 else 0)
        inp = make_inputs(rs, n, 1, 2, 2, n // 10, reference, 0.1, n // 3, 2 * n // 3, pattern="mixed", inject=(n == n0))
        run_and_check(ctx, inp, worst)
    worst.report("fused boundary n=%d" % n0)


# ------------------------------------------------------------------------------------------------------------------------ pick
PICK_PATTERNS = ("nan", "ninf", "nan_last", "tie_ends", "pinf")


def _pick_returns(name, rs, m, n):
    r = rs.randn(m, n).astype(np.float32)
    if name == "nan":
        r[:] = np.nan
    elif name == "ninf":
        r[:] = -np.inf
    elif name == "nan_last":
        r[:, n - 1] = np.nan
    elif name == "tie_ends":
        r[:, 0] = r[:, n - 1] = 50.0
    elif name == "pinf":
        r[:, (2 * n) // 3] = np.inf
        r[:, n - 1] = np.inf
    return r


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_pick_matches_numpy_argmax(n, m):
    """Index, return, first action, mean and std copies exact; ``l2a_cem_pick_act``'s dense actions hold the same bits."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(1000 * m + n)
    stream = _stream_ptr(torch.device("cuda:0"))
    for D, ad in ((5, 5), (7, 1), (256, 256), (300, 256)):
        assert D == 256 or (2 * m * D) % 256 != 0
        cand = rs.randn(n, m, D).astype(np.float32)
        mean, std = rs.randn(m, D).astype(np.float32), rs.rand(m, D).astype(np.float32)
        cand_d, mean_d, std_d = _up(cand), _up(mean), _up(std)
        for pattern in PICK_PATTERNS:
            returns = _pick_returns(pattern, rs, m, n)
            ret_d = _up(returns)
            for reference in (True, False):
                what = "n=%d m=%d D=%d ad=%d %s reference=%d" % (n, m, D, ad, pattern, reference)
                want_idx, want_ret, want_act = cr.pick(returns, cand, n, m, D, ad, reference)
                W = ad + 2
                for with_act in (False, True):
                    out = _Out((m * W + 2 * m * D,), torch.float32, float("nan"))
                    act = _Out((m, ad), torch.float32, float("nan"))
                    if with_act:
                        rc = ctx.lib.l2a_cem_pick_act(ctx.handle, _ptr(ret_d), _ptr(cand_d), _ptr(mean_d), _ptr(std_d), n, m, D, ad,
                                                      int(reference), out.ptr(), act.ptr(), stream)
                    else:
                        rc = ctx.lib.l2a_cem_pick(ctx.handle, _ptr(ret_d), _ptr(cand_d), _ptr(mean_d), _ptr(std_d), n, m, D, ad,
                                                  int(reference), out.ptr(), stream)
                    ctx.check(rc, "l2a_cem_pick")
                    torch.cuda.synchronize()
                    host, act_h = out.host(what), act.host(what)
                    head = host[:m * W].reshape(m, W)
                    assert np.array_equal(head[:, ad + 1].copy().view(np.int32), want_idx.astype(np.int32)), what
                    assert np.array_equal(head[:, ad].copy().view(np.int32), want_ret.copy().view(np.int32)), what
                    assert np.array_equal(head[:, :ad].copy().view(np.int32), want_act.copy().view(np.int32)), what
                    assert np.array_equal(host[m * W:m * W + m * D].view(np.int32), mean.reshape(-1).view(np.int32)), what
                    assert np.array_equal(host[m * W + m * D:].view(np.int32), std.reshape(-1).view(np.int32)), what
                    if with_act:
                        assert np.array_equal(act_h.view(np.int32), want_act.copy().view(np.int32)), what
                    else:
                        assert np.isnan(act_h).all()
