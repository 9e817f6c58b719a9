"""Policy priors on the GPU: the matrix-core kernel (``l2a_policy_mlp_k``, ``l2a_policy_act``) bit for bit against the fp32
restatement of its operation sequence (``tests/policy_reference.py``) and within the project's bar of the float64 oracle, its
Philox normal stream against ``l2a_mppi_sample``'s, and the closed-loop proposal (``l2a_policy_propose``): the identity that
needs no oracle, the untouched rows, the two indexings, shards, the float64 closed-loop oracle and the refusals.

The worst ``|got - want| / max(1, |want|)`` against float64 the tests print is recorded in DESIGN section 4.16 (bar 1e-4)."""

import ctypes

import numpy as np
import pytest
import torch

import cases
import cem_reference as cr
import policy_reference as pr
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativePolicyModel, NativeValueModel, _ptr, _stream_ptr

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
PHILOX_ATOL = 2e-5  # a device normal against the host's (tests/test_cem_kernels_gpu.py)
DIMS = [(1, 1), (17, 6), (20, 6), (41, 9), (64, 16)]
NETS = [((64,), "relu"), ((256, 256), "relu"), ((512, 64, 128), "tanh")]
NET_IDS = ["64_relu", "256x256_relu", "512x64x128_tanh"]
SMALL_ROWS = (1, 15, 16, 17, 33)


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """Bit equality, every NaN counted as one value."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs: " + what
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), "%d of %d words differ (first at %s: got %r, want %r): %s" % (
        bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0], what)


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_TANH = {}


def _device_tanh():
    """The device's own ``tanhf`` as the library's units compile it, elementwise on an fp32 array: a value network of one input
    whose unit 0 passes it through (kernel 1, bias 0), read back by an output kernel that picks that unit - every other operation
    of ``l2a_value_mlp_k`` on the way is exact (x - 0, * 1, fma(1, x, 0), + 0).  A zero keeps its sign, as tanh does."""
    if "fn" not in _TANH:
        vm = NativeValueModel(1, (64,), "tanh")
        w0, wo = np.zeros((1, 64), np.float32), np.zeros((64, 1), np.float32)
        w0[0, 0] = wo[0, 0] = 1.0
        vm.set_weights([w0, np.zeros(64, np.float32), wo, np.zeros(1, np.float32)])
        vm.set_norm(None)

        def fn(v):
            v = np.ascontiguousarray(v, dtype=np.float32)
            out = vm.predict(_dev(v.reshape(-1, 1))).cpu().numpy().reshape(v.shape)
            return np.where(v == 0, v, out)
        _TANH["vm"], _TANH["fn"] = vm, fn
    return _TANH["fn"]


def _hidden_fn(act):
    return _device_tanh() if act == "tanh" else None


_POLICIES = {}


def _policy(od, ad, hidden, act):
    key = (od, ad, hidden, act)
    if key not in _POLICIES:
        params, norm = pr.policy_weights(od, ad, hidden), pr.policy_norm(od, ad)
        native = NativePolicyModel(od, ad, hidden, act)
        native.set_weights(params)
        native.set_norm(norm)
        _POLICIES[key] = (native, params, norm)
    return _POLICIES[key]


def _box(ad, seed=0):
    """sigma (mixed: zeros in between), low, high with ``low == high`` in the last dimension when there is more than one."""
    rs = np.random.RandomState(900 + ad + seed)
    sigma = (0.05 + 0.3 * rs.rand(ad)).astype(np.float32)
    sigma[1::3] = 0.0
    low, high = np.full(ad, -0.45, np.float32), np.full(ad, 0.5, np.float32)
    if ad > 1:
        low[-1] = high[-1] = 0.125
    return sigma, low, high


def _act(native, states, sigma, low, high, z=None, seed=0, offset=0):
    out = native.act(_dev(states), _dev(sigma), _dev(low), _dev(high), z=_dev(z) if z is not None else None, seed=seed, offset=offset)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------
# 1. l2a_policy_act against the fp32 restatement and the float64 oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS, ids=NET_IDS)
@pytest.mark.parametrize("dims", DIMS, ids=["o%d_a%d" % d for d in DIMS])
def test_act_is_the_fp32_restatement_bit_for_bit(dims, net):
    od, ad = dims
    hidden, act = net
    native, params, norm = _policy(od, ad, hidden, act)
    sigma, low, high = _box(ad)
    hfn = _hidden_fn(act)
    worst = 0.0
    for rows in SMALL_ROWS:
        states = pr.states(40 + rows, rows, od, norm)
        z = np.random.RandomState(50 + rows).randn(rows, ad).astype(np.float32)
        z_in = z.copy()
        z_in[:, sigma == 0] = np.nan                    # never read where sigma == 0
        got = _act(native, states, sigma, low, high, z_in)
        _same(got, pr.act_f32(params, norm, act, states, sigma, low, high, z, hidden_fn=hfn), "rows=%d" % rows)
        assert np.isfinite(got).all()
        worst = max(worst, rel_err(got, pr.act64(params, norm, act, states, sigma, low, high, z)))
        if ad > 1:
            assert np.all(got[:, -1] == 0.125)          # low == high
    print("l2a_policy_act vs float64, obs %d act %d %s %s: %.2e" % (od, ad, hidden, act, worst))
    assert worst < RTOL


@pytest.mark.parametrize("net", NETS, ids=NET_IDS)
def test_act_gives_the_same_bits_under_every_rt(net):
    """Row counts that ``l2a_policy_model_geometry`` maps to every RT the widths allow on this device: the first and the last rows
    against the restatement, and a block of rows inside the big batch against the same rows launched on their own."""
    od, ad = 20, 6
    hidden, act = net
    native, params, norm = _policy(od, ad, hidden, act)
    sigma, low, high = _box(ad)
    hfn = _hidden_fn(act)
    cus = _cus()
    small = pr.states(77, 33, od, norm)
    z_small = np.random.RandomState(78).randn(33, ad).astype(np.float32)
    base = _act(native, small, sigma, low, high, z_small)
    seen = set()
    for rt in (1, 2, 4, 8):
        total = max(16 * cus * (rt // 2) + 1, 33 + 5)
        g = _lib.policy_model_geometry(od, ad, hidden, total, cus=cus)
        if g["RT"] != rt:
            continue                # (the accumulator budget caps this width below rt)
        seen.add(rt)
        big = pr.states(300 + rt, total, od, norm)
        zb = np.random.RandomState(310 + rt).randn(total, ad).astype(np.float32)
        big[5:38], zb[5:38] = small, z_small
        got = _act(native, big, sigma, low, high, zb)
        _same(got[5:38], base, "RT = %d: rows moved to another lane and tile" % rt)
        ends = np.r_[0:20, total - 20:total]
        _same(got[ends], pr.act_f32(params, norm, act, big[ends], sigma, low, high, zb[ends], hidden_fn=hfn), "RT = %d" % rt)
    cap = 32 // (max(hidden) // 64)
    assert seen == {rt for rt in (1, 2, 4, 8) if rt <= cap}, seen


def test_zero_sigma_reads_no_noise_and_non_finite_rows_stay_alone():
    od, ad, hidden, act = 17, 6, (64,), "relu"
    native, params, norm = _policy(od, ad, hidden, act)
    _, low, high = _box(ad)
    zero = np.zeros(ad, np.float32)
    states = pr.states(9, 35, od, norm)
    nan_z = np.full((35, ad), np.nan, np.float32)
    clean = _act(native, states, zero, low, high, None)
    _same(clean, pr.act_f32(params, norm, act, states, zero, low, high, None))
    _same(_act(native, states, zero, low, high, nan_z), clean, "sigma == 0 everywhere, z all NaN")
    assert np.isfinite(clean).all()
    # a NaN where sigma != 0 propagates through the clip
    sigma = zero.copy()
    sigma[2] = 0.1
    got = _act(native, states, sigma, low, high, nan_z)
    assert np.isnan(got[:, 2]).all() and np.isfinite(np.delete(got, 2, axis=1)).all()
    # rows with a NaN, or an inf, in the state: all-NaN actions, the neighbours keep their bits
    bad = states.copy()
    bad[3, od - 1] = np.inf
    bad[16, 0] = np.nan
    bad[34, 5] = -np.inf
    got = _act(native, bad, zero, low, high, None)
    assert np.isnan(got[[3, 16, 34]]).all()
    keep = np.delete(np.arange(35), [3, 16, 34])
    _same(got[keep], clean[keep], "neighbours of a non-finite row")


# ------------------------------------------------------------------------------------------
# 2. the Philox path
# ------------------------------------------------------------------------------------------
def _normals(rows, ad, seed, offset):
    """The kernel's own normals: a policy whose output is 0 everywhere, sigma = 1, bounds far away."""
    native = NativePolicyModel(20, ad, (64,), "relu")
    native.set_weights(pr.constant_weights(20, ad, (64,), np.zeros(ad)))
    native.set_norm(None)
    wide = np.full(ad, 1e30, np.float32)
    return _act(native, np.zeros((rows, 20), np.float32), np.ones(ad, np.float32), -wide, wide, None, seed=seed, offset=offset)


@pytest.mark.parametrize("ad", [1, 6, 16])
@pytest.mark.parametrize("seed,offset", [(0, 0), (0x5EED0000ABCD1234, 977), (12345, 2 ** 32 - 100), (7, 2 ** 40 + 3)])
def test_philox_stream(ad, seed, offset):
    rows = 300
    a = _normals(rows, ad, seed, offset)
    _same(_normals(rows, ad, seed, offset), a, "the same seed and offset")
    # offset + 1 element: the stream moves by one element
    b = _normals(rows, ad, seed, offset + 1)
    _same(b.reshape(-1)[:-1], a.reshape(-1)[1:], "offset shifted by one element")
    # a host restatement of Philox4x32-10 + Box-Muller (the device's logf / cosf are off by a few ulp of the host's)
    want = cr.philox_normal(seed, cr.philox_indices(offset, rows * ad)).reshape(rows, ad)
    assert np.max(np.abs(a.astype(np.float64) - want)) <= PHILOX_ATOL
    assert abs(float(np.mean(a))) < 0.2 and 0.8 < float(np.std(a)) < 1.2
    # l2a_mppi_sample at the same counters: zero mean (shift -1), sigma = 1, beta = 1, bounds far away -> its samples ARE the normals
    ctx = _lib.Context.get(0)
    n, m, h = rows, 1, 1
    wide = _dev(np.full(ad, 1e30, np.float32))
    neg_wide, ones, mean_in, fresh = -wide, _dev(np.ones(ad, np.float32)), _dev(np.zeros((m, h * ad), np.float32)), _dev(np.full(m, -1), np.int32)
    a_clip = torch.full((n, m, h * ad), np.nan, dtype=torch.float32, device="cuda:0")
    seq = torch.full((h, m * n, ad), np.nan, dtype=torch.float32, device="cuda:0")
    mean_out = torch.zeros((m, h * ad), dtype=torch.float32, device="cuda:0")
    rc = ctx.lib.l2a_mppi_sample(ctx.handle, None, ctypes.c_ulonglong(seed), ctypes.c_ulonglong(offset), _ptr(mean_in), _ptr(fresh),
                                 _ptr(ones), 1.0, _ptr(neg_wide), _ptr(wide), n, m, h, ad, _ptr(mean_out), _ptr(a_clip), _ptr(seq),
                                 _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    assert rc == _lib.L2A_OK, ctx.lib.l2a_last_error(ctx.handle).decode()
    _same(a_clip.cpu().numpy().reshape(rows, ad), a, "l2a_mppi_sample's normals")


# ------------------------------------------------------------------------------------------
# 3. l2a_policy_propose
# ------------------------------------------------------------------------------------------
N_TOTAL = 40
_MODELS = {}


def _model(mode, width):
    """A product model of ``tests/cases.py`` (a mean ensemble of two members, or three per-block sets), its oracle, a policy."""
    key = (mode, width)
    if key not in _MODELS:
        case = dict(env="half_cheetah", mode=mode, hidden=[width, width], E=2 if mode == "mean" else 3)
        env, model = cases.product_model(case)
        _, sets, norms = cases.recipe(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        hidden, act = (64, 64), "relu"
        params, norm = pr.policy_weights(od, ad, hidden, seed=8200), pr.policy_norm(od, ad, base=norms[0])
        policy = NativePolicyModel(od, ad, hidden, act)
        policy.set_weights(params)
        policy.set_norm(norm)
        _MODELS[key] = dict(case=case, env=env, native=model.planner_model(), model=model, sets=sets, norms=norms, od=od, ad=ad,
                            policy=policy, params=params, norm=norm, act=act)
    return _MODELS[key]


def _oracle(s, m):
    from oracle import OracleMLPDynamics
    case = s["case"]
    if case["mode"] == "per_block":         # env i <-> set i: the first m sets
        return OracleMLPDynamics(s["od"], s["ad"], s["sets"][:m], s["norms"][:m], mode="per_block", mlp_dtype=np.float64)
    return OracleMLPDynamics(s["od"], s["ad"], s["sets"], s["norms"], mode="mean", mlp_dtype=np.float64)


def _nan_fill(shape, tag):
    """Distinct NaN payloads: word e = 0x7FC00000 | tag << 20 | (e mod 2^20)."""
    count = int(np.prod(shape))
    words = (np.uint32(0x7FC00000) | np.uint32(tag << 20) | (np.arange(count, dtype=np.uint32) & np.uint32(0xFFFFF)))
    return torch.from_numpy(words.view(np.float32).reshape(shape).copy()).to("cuda:0")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _propose(s, obs0, m, n, n_pi, h, sigma, low, high, cand_offset=0, z=None, seed=0, offset=0, mirror=True):
    ad = s["ad"]
    seq = _nan_fill((h, m * n, ad), 1)
    mir = _nan_fill((N_TOTAL, m, h * ad), 2) if mirror else None
    seq0, mir0 = _words(seq).copy(), (_words(mir).copy() if mirror else None)
    s["native"].policy_propose(s["policy"], _dev(obs0), m, n, n_pi, h, seq, _dev(sigma), _dev(low), _dev(high), mirror=mir,
                               n_total=N_TOTAL, cand_offset=cand_offset, z=_dev(z) if z is not None else None, seed=seed, offset=offset)
    torch.cuda.synchronize()
    return seq, mir, seq0, mir0


def _env_box(s):
    ad = s["ad"]
    sigma = np.array([0.05, 0.0, 0.1, 0.02, 0.0, 0.08], dtype=np.float32)[:ad]
    return sigma, np.asarray(s["env"].action_space.low, np.float32), np.asarray(s["env"].action_space.high, np.float32)


@pytest.mark.parametrize("width", [32, 128, 256])
@pytest.mark.parametrize("mode", ["mean", "per_block"])
def test_propose_closed_loop_identity_untouched_rows_and_oracle(mode, width):
    s = _model(mode, width)
    native, policy, od, ad = s["native"], s["policy"], s["od"], s["ad"]
    sigma, low, high = _env_box(s)
    n = N_TOTAL
    worst = 0.0
    for m in (1, 3):
        obs0 = pr.states(60 + m, m, od, s["norm"])
        dyn = _oracle(s, m)
        for n_pi in (1, 5, 16, 21, 40):
            for h in (1, 2, 5):
                what = "%s width %d m=%d n_pi=%d h=%d" % (mode, width, m, n_pi, h)
                z = np.random.RandomState(1000 * m + 10 * n_pi + h).randn(h, m, n_pi, ad).astype(np.float32)
                before = native.policy_proposals
                seq, mir, seq0, mir0 = _propose(s, obs0, m, n, n_pi, h, sigma, low, high, z=z)
                assert native.policy_proposals == before + 1
                got = seq.cpu().numpy().reshape(h, m, n, ad)
                # rows with gj >= n_pi: every word unchanged, in seq and in mirror
                w_seq, w_mir = _words(seq).reshape(h, m, n, ad), _words(mir).reshape(N_TOTAL, m, h, ad)
                assert np.array_equal(w_seq[:, :, n_pi:], seq0.reshape(h, m, n, ad)[:, :, n_pi:]), what
                assert np.array_equal(w_mir[n_pi:], mir0.reshape(N_TOTAL, m, h, ad)[n_pi:]), what
                prop = np.ascontiguousarray(got[:, :, :n_pi])                   # [h, m, n_pi, ad]
                assert np.isfinite(prop).all(), what
                # mirror[(gj m + i), t, k] == seq[t, i n + gj, k]
                assert np.array_equal(w_mir[:n_pi].transpose(2, 1, 0, 3), w_seq[:, :, :n_pi]), what
                # closed loop: the policy on the model's own states of the proposed actions gives the proposed actions
                flat = prop.reshape(h, m * n_pi, ad)
                traj = native.rollout_traj(_dev(obs0), _dev(flat), m, n_pi, h).cpu().numpy()
                for t in range(h):
                    st = np.repeat(obs0, n_pi, axis=0) if t == 0 else traj[t - 1]
                    again = _act(policy, st, sigma, low, high, z[t].reshape(m * n_pi, ad))
                    _same(again, flat[t], what + " t=%d" % t)
                # the float64 closed-loop oracle
                want, _ = pr.propose64(dyn, s["params"], s["norm"], s["act"], obs0, n_pi, h, sigma, low, high, z)
                worst = max(worst, rel_err(flat, want))
    print("l2a_policy_propose vs float64 closed loop, %s width %d: %.2e" % (mode, width, worst))
    assert worst < RTOL


@pytest.mark.parametrize("noise", ["injected", "philox"])
@pytest.mark.parametrize("mode", ["mean", "per_block"])
def test_shards_reproduce_the_unsharded_rows(mode, noise):
    s = _model(mode, 128)
    ad, od = s["ad"], s["od"]
    sigma, low, high = _env_box(s)
    m, h, n_pi = 3, 3, 9
    obs0 = pr.states(71, m, od, s["norm"])
    z = np.random.RandomState(5).randn(h, m, n_pi, ad).astype(np.float32) if noise == "injected" else None
    kw = dict(z=z, seed=0xABCDEF12345, offset=4321)
    seq, mir, _, _ = _propose(s, obs0, m, N_TOTAL, n_pi, h, sigma, low, high, **kw)
    full, full_mir = seq.cpu().numpy().reshape(h, m, N_TOTAL, ad), _words(mir)
    for cand_offset, n_local in ((0, 3), (3, 4), (7, 33)):
        sq, mr_, sq0, mr0 = _propose(s, obs0, m, n_local, n_pi, h, sigma, low, high, cand_offset=cand_offset, **kw)
        own = max(0, min(n_local, n_pi - cand_offset))
        got = sq.cpu().numpy().reshape(h, m, n_local, ad)
        _same(got[:, :, :own], full[:, :, cand_offset:cand_offset + own], "shard at %d" % cand_offset)
        assert np.array_equal(_words(sq).reshape(h, m, n_local, ad)[:, :, own:], sq0.reshape(h, m, n_local, ad)[:, :, own:])
        w = _words(mr_).reshape(N_TOTAL, m, h * ad)
        assert np.array_equal(w[cand_offset:cand_offset + own], full_mir.reshape(N_TOTAL, m, h * ad)[cand_offset:cand_offset + own])
        rest = np.r_[0:cand_offset, cand_offset + own:N_TOTAL]
        assert np.array_equal(w[rest], mr0.reshape(N_TOTAL, m, h * ad)[rest])
    # a shard beyond n_pi: nothing launched, nothing written
    sq, mr_, sq0, mr0 = _propose(s, obs0, m, 20, n_pi, h, sigma, low, high, cand_offset=20, **kw)
    assert np.array_equal(_words(sq), sq0) and np.array_equal(_words(mr_), mr0)
    sq, mr_, sq0, mr0 = _propose(s, obs0, m, 31, n_pi, h, sigma, low, high, cand_offset=9, **kw)
    assert np.array_equal(_words(sq), sq0) and np.array_equal(_words(mr_), mr0)


def test_propose_without_a_mirror_and_with_philox_noise_repeats():
    s = _model("mean", 128)
    sigma, low, high = _env_box(s)
    m, h, n_pi = 2, 4, 7
    obs0 = pr.states(72, m, s["od"], s["norm"])
    a, none, _, _ = _propose(s, obs0, m, N_TOTAL, n_pi, h, sigma, low, high, seed=11, offset=5, mirror=False)
    b, mir, _, _ = _propose(s, obs0, m, N_TOTAL, n_pi, h, sigma, low, high, seed=11, offset=5)
    c, _, _, _ = _propose(s, obs0, m, N_TOTAL, n_pi, h, sigma, low, high, seed=11, offset=5 + h * m * n_pi * s["ad"])
    assert none is None and np.array_equal(_words(a), _words(b))
    assert not np.array_equal(_words(a), _words(c))                     # the next call's counters: other normals


def test_propose_refusals_touch_nothing():
    s = _model("per_block", 128)                                        # three sets
    native, policy, od, ad = s["native"], s["policy"], s["od"], s["ad"]
    lib, null = native.lib, ctypes.c_void_p()
    sigma, low, high = (_dev(x) for x in _env_box(s))
    m, n, h, n_pi = 3, N_TOTAL, 2, 5
    obs0 = _dev(pr.states(73, 4, od, s["norm"]))
    seq = _nan_fill((h, 4 * n, ad), 1)
    mir = _nan_fill((N_TOTAL, 4, h * ad), 2)
    seq0, mir0 = _words(seq).copy(), _words(mir).copy()
    other = NativePolicyModel(od, ad - 1, (64,), "relu")
    other_obs = NativePolicyModel(od - 1, ad, (64,), "relu")
    stream = _stream_ptr(torch.device("cuda:0"))

    def call(md=native.handle, pm=policy.handle, o=obs0, m_=m, n_=n, npi=n_pi, h_=h, off=0, sg=sigma, lo=low, hi=high, sq=seq, nt=N_TOTAL):
        p = lambda t: _ptr(t) if t is not None else null        # noqa: E731
        return lib.l2a_policy_propose(md, pm, p(o), m_, n_, npi, h_, off, null, 0, 0, p(sg), p(lo), p(hi), p(sq), _ptr(mir), nt, stream)

    before = native.policy_proposals
    for kw in (dict(pm=null), dict(o=None), dict(sg=None), dict(lo=None), dict(hi=None), dict(sq=None), dict(m_=0), dict(n_=0),
               dict(h_=0), dict(npi=0), dict(npi=N_TOTAL + 1), dict(off=-1), dict(off=1), dict(n_=N_TOTAL + 1), dict(pm=other.handle),
               dict(pm=other_obs.handle), dict(m_=4)):
        assert call(**kw) == _lib.L2A_EINVAL, kw
        assert lib.l2a_last_error(native.ctx.handle).decode(), kw
    assert call(md=null) == _lib.L2A_EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_words(seq), seq0) and np.array_equal(_words(mir), mir0)
    assert native.policy_proposals == before
    assert "n_sets" in (call(m_=4), lib.l2a_last_error(native.ctx.handle).decode())[1]
    # ... and the same call goes through once it is well-formed
    assert call() == _lib.L2A_OK
    torch.cuda.synchronize()
    assert not np.array_equal(_words(seq), seq0)
    # l2a_policy_act's own refusals
    out = torch.full((8, ad), -5.0, dtype=torch.float32, device="cuda:0")
    st = _dev(pr.states(74, 8, od, s["norm"]))
    for args in ((null, 8, _ptr(out)), (_ptr(st), 0, _ptr(out)), (_ptr(st), 8, null), (_ptr(st), 2 ** 30, _ptr(out))):
        assert lib.l2a_policy_act(policy.handle, args[0], args[1], null, 0, 0, _ptr(sigma), _ptr(low), _ptr(high), args[2],
                                  stream) == _lib.L2A_EINVAL
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == -5.0)
    fresh = NativePolicyModel(od, ad, (64,), "relu")
    assert lib.l2a_policy_act(fresh.handle, _ptr(st), 8, null, 0, 0, _ptr(sigma), _ptr(low), _ptr(high), _ptr(out), stream) == _lib.L2A_ESTATE
    assert "never set" in lib.l2a_last_error(native.ctx.handle).decode()
