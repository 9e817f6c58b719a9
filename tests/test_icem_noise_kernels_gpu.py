"""``l2a_icem_sample_noise`` / ``l2a_icem_sample_noise_shard`` (``csrc/l2a_icem.hip``: ``l2a_icem_sample_noise_k``, the iCEM sample with
``nz = M z`` in place of the AR(1) recurrence) against ``tests/icem_noise_reference.py``, a plain NumPy restatement pinned by
``tests/test_icem_noise_reference.py``.  The C entry points are called directly; every output starts from NaN and sits between 64
guard words; the inputs - the matrix among them - are checked unchanged.

Nothing is left to a tolerance: samples from injected normals and injected random non-symmetric matrices bit for bit
(``sample_noise_f32``; a transposed read cannot pass), ``M = I`` equal to ``l2a_icem_sample`` at ``rho = 0`` as values on the Philox
stream, the power-law matrix on the Philox stream bit for bit from the normals that call read back, every window of the shard
entry bit for bit the unsharded call's rows."""

import ctypes

import numpy as np
import pytest

import icem_noise_reference as nr
from learning_to_adapt_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD, F_GUARD = 64, 12345.0
KEYS = ("mean", "std", "kept", "kc", "shift", "sigma0", "low", "high", "z", "noise")
OUTS = ("mean_out", "std_out", "a_clip", "seq")
SHIFTS3 = ([-1, 1, 0], [1, 0, -1], [0, -1, 1], [1, 1, 1], [0, 0, 0], [-1, -1, 1])
VECTORS = list(SHIFTS3) + [[-1], [1], [0]]
SAMPLE_N = (1, 2, 63, 64, 65, 257)
K_SAMPLE = 4
# odd and even h | strides 32, 33 and 64 floats (where an LDS row without padding would meet itself on one bank) | (128, 16): one
# row per workgroup fills the whole 2048-float tile | (1, 1), (4, 6), (7, 16), (30, 6): 4, 4, 2 and 1 rows per workgroup
SHAPES = [(1, 1), (2, 16), (3, 11), (4, 6), (7, 16), (30, 6), (32, 8), (33, 8), (64, 3), (128, 16), (128, 1)]
FULL_WORK = 1 << 21         # n * h * h * A up to which a case runs every (Kk, shift vector) pair; above it one walk over the vectors
HEAVY_WORK = 1 << 25        # ... above which (n_it = 257 at h = 128, A = 16 only) the walk takes two of the six mixed vectors


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _ull(x):
    return ctypes.c_ulonglong(int(x) & 0xFFFFFFFFFFFFFFFF)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Out(object):
    """A device fp32 output of ``shape`` between two runs of guard words, pre-filled with NaN."""

    def __init__(self, shape):
        import torch
        self.size = int(np.prod(shape))
        self.shape = tuple(shape)
        self.flat = torch.full((self.size + 2 * GUARD,), F_GUARD, dtype=torch.float32, device="cuda:0")
        self.flat[GUARD:GUARD + self.size].fill_(NAN)

    def ptr(self):
        return ctypes.c_void_p(self.flat.data_ptr() + 4 * GUARD)

    def host(self, what):
        h = self.flat.cpu().numpy()
        assert np.all(h[:GUARD] == F_GUARD) and np.all(h[GUARD + self.size:] == F_GUARD), "guard words overwritten: " + what
        return h[GUARD:GUARD + self.size].reshape(self.shape).copy()


# ---------------------------------------------------------------------------------------------------------------------- harness
def run(ctx, inp, entry="noise", window=None, with_seq=True, expect_rc=_lib.L2A_OK, alias=None, null=None):
    """One call of ``l2a_icem_sample_noise`` (``entry="noise"``; with ``window = (lo, hi)``: ``l2a_icem_sample_noise_shard``) or of
    ``l2a_icem_sample`` (``entry="ar1"``, ``inp["rho"]``); the four outputs as host arrays, guards checked, inputs checked unchanged.
    With an error expected every output must still hold NaN.  ``alias = (output, input)`` passes the input's buffer as that output,
    ``null`` names an argument passed as NULL.  A window's ``seq`` is allocated at exactly ``h * m * (hi - lo) * A`` floats."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    n, m, h, ad, Kk = inp["n"], inp["m"], inp["h"], inp["ad"], inp["Kk"]
    D = h * ad
    what = "%s n=%d m=%d h=%d ad=%d Kk=%d kc=%s shift=%s add_mean=%d inject=%d seq=%d window=%s" % (
        entry, n, m, h, ad, Kk, None if inp["kc"] is None else list(inp["kc"]), list(inp["shift"]), inp["add_mean"],
        inp["z"] is not None, with_seq, window)
    dev = {k: (_up(inp[k]) if inp.get(k) is not None else None) for k in KEYS}
    width = max(n, 1)
    if window is not None:
        lo, hi = window
        width = max(hi - lo, 1) if 0 <= lo <= hi <= n else 1
    out = dict(mean_out=_Out((m, D)), std_out=_Out((m, D)), a_clip=_Out((max(n, 1), m, D)), seq=_Out((h, m * width, ad)))
    ptr = {k: o.ptr() for k, o in out.items()}
    if not with_seq:
        ptr["seq"] = None
    arg = {k: _ptr(dev[k]) for k in KEYS}
    if alias is not None:
        ptr[alias[0]] = arg[alias[1]]
    if null is not None:
        (ptr if null in ptr else arg)[null] = None
    head = (ctx.handle, arg["z"], _ull(inp.get("seed", 0)), _ull(inp.get("off", 0)), arg["mean"], arg["std"], arg["kept"], arg["kc"],
            arg["shift"], arg["sigma0"])
    mid = (arg["low"], arg["high"], n, m, h, ad, Kk, int(inp["add_mean"]))
    tail = (ptr["mean_out"], ptr["std_out"], ptr["a_clip"], ptr["seq"], _stream_ptr(torch.device("cuda:0")))
    if entry == "ar1":
        rc = ctx.lib.l2a_icem_sample(*(head + (float(inp["rho"]),) + mid + tail))
    elif window is None:
        rc = ctx.lib.l2a_icem_sample_noise(*(head + (arg["noise"],) + mid + tail))
    else:
        rc = ctx.lib.l2a_icem_sample_noise_shard(*(head + (arg["noise"],) + mid + (window[0], window[1]) + tail))
    torch.cuda.synchronize()
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    host = {k: o.host(k + " " + what) for k, o in out.items()}
    for k in KEYS:
        if inp.get(k) is not None:
            assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(inp[k])), "input changed: %s %s" % (k, what)
    if expect_rc != _lib.L2A_OK:
        assert all(np.isnan(v).all() for v in host.values()), "output written by a refused call: " + what
        return rc
    if not with_seq:
        assert np.isnan(host["seq"]).all(), "seq written though NULL was passed: " + what
    return host


def _bounds(ad):
    return np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)


def inputs(rs, n, m, h, ad, shift, Kk=0, kc=None, add_mean=0, inject=True, seed=0, off=0, noise=None, zero_sigma=None):
    """``noise = None``: a random dense matrix, not symmetric, scaled so that the sums stay of order one."""
    D = h * ad
    low, high = _bounds(ad)
    sigma0 = (0.1 + 0.5 * rs.rand(ad)).astype(np.float32)
    if zero_sigma is not None:
        sigma0[zero_sigma] = 0.0
    mean = (0.7 * rs.randn(m, D)).astype(np.float32)            # beyond both bounds in some dimensions
    std = (0.05 + 0.6 * rs.rand(m, D)).astype(np.float32)
    kept = np.clip((0.5 * rs.randn(m, Kk, D)).astype(np.float32), np.tile(low, h), np.tile(high, h)) if Kk > 0 else None
    z = rs.randn(max(n, 1), m, D).astype(np.float32) if inject else None
    if noise is None:
        noise = (rs.randn(max(h, 1), max(h, 1)) / np.sqrt(max(h, 1))).astype(np.float32)
    return dict(n=n, m=m, h=h, ad=ad, Kk=Kk, add_mean=add_mean, shift=np.asarray(shift, dtype=np.int32), mean=mean, std=std, kept=kept,
                kc=None if Kk == 0 else np.asarray(kc, dtype=np.int32), sigma0=sigma0, low=low, high=high, z=z, seed=seed, off=off,
                noise=np.ascontiguousarray(noise, dtype=np.float32), rho=0.0)


def want(inp, z=None):
    return nr.sample_noise_f32(inp["mean"], inp["std"], inp["kept"], inp["kc"], inp["shift"], inp["z"] if z is None else z, inp["sigma0"],
                               inp["noise"], inp["low"], inp["high"], inp["n"], inp["m"], inp["h"], inp["ad"], inp["Kk"], inp["add_mean"])


def check(got, inp, with_seq, what, z=None):
    mu, sd, a, seq = want(inp, z)
    assert np.array_equal(_bits(got["mean_out"]), _bits(mu)), "mean_out: " + what
    assert np.array_equal(_bits(got["std_out"]), _bits(sd)), "std_out: " + what
    assert np.array_equal(_bits(got["a_clip"]), _bits(a)), "a_clip: " + what
    if with_seq:
        assert np.array_equal(_bits(got["seq"]), _bits(seq)), "seq: " + what
    return a


# ------------------------------------------------------------------------------------------------- injected normals and matrices
def sub_cases(ni, n, full, heavy=False):
    """``(m, Kk, shift, kc, add_mean, with_seq)``.  ``full``: every ``Kk`` in (0, 1, K) x every one of the six mixed shift vectors at
    m = 3 and the three shifts at m = 1; otherwise (the largest shapes, where the NumPy restatement's ``n m D h`` products set the
    test's time) one walk over the nine vectors with ``Kk`` moving on with the vector and with ``n_it`` (``heavy``: over the three
    m = 1 vectors and two of the six mixed ones - the other four meet that shape at the smaller ``n_it``).  Env i's stored count walks
    (0, 1, Kk) with the indices of ``n_it``, the vector and i; the mean row and a NULL ``seq`` follow the (vector, Kk) index."""
    out = []
    for vi, shift in enumerate(VECTORS):
        for ki, Kk in enumerate((0, 1, K_SAMPLE)):
            if not full and ki != (vi + ni) % 3:
                continue
            if heavy and len(shift) == 3 and vi % 3 != ni % 3:
                continue
            idx = vi * 3 + ki
            kc = [int((0, 1, Kk)[(ni + vi + i) % 3]) for i in range(len(shift))]
            out.append((len(shift), Kk, list(shift), kc, (idx // 4 + (0 if full else ni)) % 2, (idx + (0 if full else ni)) % 4 != 3))
    return out


def test_sub_cases_cover_what_they_claim():
    vectors = {tuple(v) for v in VECTORS}
    for ni, n in enumerate(SAMPLE_N):
        cs = sub_cases(ni, n, True)
        assert {(Kk, tuple(sh)) for _, Kk, sh, _, _, _ in cs} == {(Kk, v) for Kk in (0, 1, K_SAMPLE) for v in vectors}
        assert {(am, ws) for _, _, _, _, am, ws in cs} == {(0, True), (0, False), (1, True), (1, False)}
    walk = [c for ni, n in enumerate(SAMPLE_N) for c in sub_cases(ni, n, False)]
    assert {(Kk, tuple(sh)) for _, Kk, sh, _, _, _ in walk} == {(Kk, v) for Kk in (0, 1, K_SAMPLE) for v in vectors}
    assert {(am, ws) for _, _, _, _, am, ws in walk} == {(0, True), (0, False), (1, True), (1, False)}
    for ni, n in enumerate(SAMPLE_N):
        cs = sub_cases(ni, n, False)
        assert {tuple(sh) for _, _, sh, _, _, _ in cs} == vectors and {am for _, _, _, _, am, _ in cs} == {0, 1}
    heavy = sub_cases(5, 257, False, heavy=True)
    assert {tuple(sh) for _, _, sh, _, _, _ in heavy} == {tuple(VECTORS[2]), tuple(VECTORS[5]), (-1,), (1,), (0,)}
    assert {Kk for _, Kk, _, _, _, _ in heavy} == {0, 1, K_SAMPLE} and {am for _, _, _, _, am, _ in heavy} == {0, 1}


@pytest.mark.parametrize("n", SAMPLE_N)
@pytest.mark.parametrize("h,ad", SHAPES)
def test_sample_with_injected_normals_and_matrices_bit_for_bit(h, ad, n):
    """``mean_out``, ``std_out``, ``a_clip`` and ``seq`` equal ``sample_noise_f32`` bit for bit with a fresh random non-symmetric
    matrix per sub-case (``sub_cases``): mixed shift vectors, kept rows with counts in (0, 1, Kk) - at ``n_it`` = 1 and 2 that is
    ``kc >= n_it`` -, the mean row and a NULL ``seq`` on and off, means beyond both bounds, and in every third sub-case one dimension
    with ``sigma0 = 0``."""
    ctx = _lib.Context.get(0)
    ni = SAMPLE_N.index(n)
    rs = np.random.RandomState(100000 * h + 1000 * ad + n)
    on_low = on_high = False
    work = n * h * h * ad
    for c, (m, Kk, shift, kc, add_mean, with_seq) in enumerate(sub_cases(ni, n, work <= FULL_WORK, work > HEAVY_WORK)):
        inp = inputs(rs, n, m, h, ad, shift, Kk=Kk, kc=kc, add_mean=add_mean, zero_sigma=(c % ad) if c % 3 == 0 else None)
        what = "n=%d m=%d h=%d ad=%d Kk=%d kc=%s shift=%s add_mean=%d" % (n, m, h, ad, Kk, kc, shift, add_mean)
        a = check(run(ctx, inp, with_seq=with_seq), inp, with_seq, what)
        on_low = on_low or bool((a == np.tile(inp["low"], h)).any())
        on_high = on_high or bool((a == np.tile(inp["high"], h)).any())
    assert on_low and on_high, "no sub-case put a sample on each bound"


def test_a_transposed_matrix_is_told_apart():
    """The restatement with ``M^T`` differs from the kernel's output on ``M``: the bit-for-bit tests would catch a transposed read."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(41)
    inp = inputs(rs, 9, 2, 7, 3, [0, -1])
    got = run(ctx, inp)
    check(got, inp, True, "M")
    a_t = want(dict(inp, noise=np.ascontiguousarray(inp["noise"].T)))[2]
    assert not np.array_equal(_bits(a_t), _bits(got["a_clip"]))


# ------------------------------------------------------------------------------------------------------------ the Philox stream
@pytest.mark.parametrize("off", [0, (1 << 32) - 5, 1 << 40])
def test_identity_is_the_white_ar1_sample_and_powerlaw_uses_the_same_normals(off):
    """``z = NULL``: with ``M = I`` the outputs equal ``l2a_icem_sample`` at ``rho = 0`` on the same seed and offset as values - that
    entry is held to ``l2a_cem_sample`` bit for bit elsewhere, so the stream is positional and CEM's (the launch at 2^32 - 5 crosses
    into the counter's high word).  On fresh envs with ``sigma0 = 1`` and bounds far away that call's ``a_clip`` IS the stream's
    normals; the power-law matrix (``l2a_icem_noise_matrix``) on the same stream then equals ``sample_noise_f32`` applied to them,
    bit for bit."""
    ctx = _lib.Context.get(0)
    n, m, h, ad = 66, 2, 7, 8
    D = h * ad
    M = np.empty((h, h), dtype=np.float32)
    assert ctx.lib.l2a_icem_noise_matrix(h, 2.0, M.ctypes.data) == _lib.L2A_OK
    exact = nr.noise_matrix(h, 2.0)
    assert np.all(np.abs(M.astype(np.float64) - exact) <= 2.0 ** -23 * np.abs(exact) + 1e-15)
    for seed in (0x5EED0000ABCD1234, 1):
        rs = np.random.RandomState(7)
        what = "seed=%#x offset=%#x" % (seed, off)
        for shift, Kk, kc, add_mean in (([-1, 0], 0, None, 0), ([1, 0], 3, [2, 3], 1)):
            inp = inputs(rs, n, m, h, ad, shift, Kk=Kk, kc=kc, add_mean=add_mean, inject=False, seed=seed, off=off, noise=np.eye(h))
            got, ar1 = run(ctx, inp), run(ctx, inp, entry="ar1")
            for k in OUTS:
                assert np.array_equal(got[k], ar1[k]) and not np.isnan(got[k]).any(), "%s (M = I): %s" % (k, what)
        # the normals themselves: mu' = 0, sd' = 1, no clip
        raw = inputs(rs, n, m, h, ad, [-1, -1], inject=False, seed=seed, off=off, noise=np.eye(h))
        raw["sigma0"] = np.ones(ad, dtype=np.float32)
        raw["low"], raw["high"] = np.full(ad, -1e9, dtype=np.float32), np.full(ad, 1e9, dtype=np.float32)
        z = run(ctx, raw, entry="ar1")["a_clip"]
        assert len(np.unique(z)) > n * m * D // 2 and abs(float(z.std()) - 1.0) < 0.1
        for shift, Kk, kc, add_mean in (([-1, 0], 0, None, 0), ([1, 0], 3, [2, 3], 1)):
            inp = inputs(rs, n, m, h, ad, shift, Kk=Kk, kc=kc, add_mean=add_mean, inject=False, seed=seed, off=off, noise=M)
            check(run(ctx, inp), inp, True, "power-law on the stream: " + what, z=z)


# ------------------------------------------------------------------------------------------------------------------ shard entry
SHARD_SHAPES = [(13, 3, 5, 6), (40, 2, 4, 8), (9, 2, 128, 16)]
SHARD_KC = {3: [3, 4, 2], 2: [2, 4]}
SHARD_SHIFT = {3: [1, 0, -1], 2: [1, 0]}


def windows(n):
    """name -> [lo, hi): all rows, odd cuts, one row, an empty window, kept rows only, the window that holds the add_mean row."""
    return dict(full=(0, n), inner=(3, 8), one=(5, 6), empty=(7, 7), kept=(0, 2), mean=(n - 3, n))


@pytest.mark.parametrize("inject", [True, False], ids=["injected", "philox"])
@pytest.mark.parametrize("shape", SHARD_SHAPES, ids=lambda s: "n%d_m%d_h%d_A%d" % s)
def test_every_window_matches_the_unsharded_call(shape, inject):
    n, m, h, ad = shape
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(n + 10 * h)
    inp = inputs(rs, n, m, h, ad, SHARD_SHIFT[m], Kk=4, kc=SHARD_KC[m], add_mean=1, inject=inject, seed=0x5EED0000ABCD1234,
                 off=0 if inject else 977 * n * m * h * ad)
    full = run(ctx, inp)
    assert not np.isnan(full["seq"]).any()
    if inject:
        check(full, inp, True, "unsharded")
    seq_rows = full["seq"].reshape(h, m, n, ad)
    for name, (lo, hi) in windows(n).items():
        got = run(ctx, inp, window=(lo, hi), with_seq=not (name == "empty" and inject))
        for key in ("a_clip", "mean_out", "std_out"):
            assert np.array_equal(_bits(got[key]), _bits(full[key])), (name, key)
        if hi == lo:
            assert np.isnan(got["seq"]).all(), "an empty window wrote seq_local"
            continue
        rows = np.ascontiguousarray(seq_rows[:, :, lo:hi, :]).reshape(h, m * (hi - lo), ad)
        assert np.array_equal(_bits(got["seq"]), _bits(rows)), (name, lo, hi)


# -------------------------------------------------------------------------------------------------------------- reproducibility
def test_runs_and_identical_envs_give_the_same_bits():
    """Two runs: equal bits.  Three envs with the same state, shift and kept rows and - injected - the same normals sit in
    different workgroups and at different rows of a workgroup: equal bits again (an element's sum depends on its matrix row and
    its normals only)."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(15)
    n, m, h, ad, Kk = 65, 3, 7, 6, 3
    inp = inputs(rs, n, m, h, ad, [1, 0, -1], Kk=Kk, kc=[3, 1, 2], add_mean=1, inject=False, seed=5, off=1 << 33)
    runs = [run(ctx, inp) for _ in range(2)]
    for k in OUTS:
        assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
    same = inputs(rs, n, m, h, ad, [0, 0, 0], Kk=Kk, kc=[2, 2, 2], add_mean=1)
    for k in ("mean", "std", "kept"):
        same[k] = np.ascontiguousarray(np.broadcast_to(same[k][:1], same[k].shape))
    same["z"] = np.ascontiguousarray(np.broadcast_to(same["z"][:, :1], same["z"].shape))
    got = run(ctx, same)
    check(got, same, True, "identical envs")
    for i in (1, 2):
        assert np.array_equal(_bits(got["a_clip"][:, i]), _bits(got["a_clip"][:, 0])), i
        assert np.array_equal(_bits(got["mean_out"][i]), _bits(got["mean_out"][0])), i
        assert np.array_equal(_bits(got["std_out"][i]), _bits(got["std_out"][0])), i
    seq = got["seq"].reshape(h, m, n, ad)
    assert np.array_equal(_bits(seq[:, 1]), _bits(seq[:, 0])) and np.array_equal(_bits(seq[:, 2]), _bits(seq[:, 0]))


# --------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_write_nothing():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(12)
    E = _lib.L2A_EINVAL

    def case(n=5, m=2, h=3, ad=4, Kk=2, window=None, **kw):
        return run(ctx, inputs(rs, n, m, h, ad, [0] * m, Kk=Kk, kc=[1] * m), window=window, expect_rc=E, **kw)

    for window in (None, (1, 4)):
        assert case(ad=17, window=window) == E
        assert case(ad=0, window=window) == E
        assert case(n=0, window=None if window is None else (0, 0)) == E
        assert case(m=0, window=window) == E
        assert case(h=0, window=window) == E
        assert case(h=129, ad=1, window=window) == E
        assert case(Kk=8193, window=window) == E
        assert case(Kk=-1, window=window) == E
        for pair in (("mean_out", "mean"), ("std_out", "std"), ("mean_out", "std"), ("a_clip", "z"), ("seq", "kept"),
                     ("mean_out", "noise"), ("std_out", "noise"), ("a_clip", "noise"), ("seq", "noise")):
            assert case(alias=pair, window=window) == E, pair
        for name in ("mean", "std", "kept", "kc", "shift", "sigma0", "low", "high", "noise", "mean_out", "std_out", "a_clip"):
            assert case(null=name, window=window) == E, name
    for window in ((-1, 4), (3, 6), (4, 3)):
        assert case(window=window) == E, window
    assert case(window=(0, 4), with_seq=False) == E         # a window that holds candidates needs its tensor
    # h = 128 is inside the limit
    inp = inputs(rs, 2, 1, 128, 1, [0])
    check(run(ctx, inp), inp, True, "h = 128")
