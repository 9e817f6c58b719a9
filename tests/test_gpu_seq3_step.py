"""The static three-set step of the MFMA rollout kernel (csrc/l2a_mfma.h SEQ3, `l2a_set_seq3`) on the GPU: a mean ensemble of
five 2 x 512 sets under the shared-set tile split runs kernel instances that know their sequence - full, full, shared - at
compile time.  Same arithmetic in the same order: every plan must give the bits of the general tile-split instances (switch
off) and of the unsplit launch, twice, with a clean launch status, and agree with the float64 oracle.

Shapes: HalfCheetah's 20 + 6 (the O4 instance <2, 2>), 24 + 6 (<2, 2> without the four-unit output tile), 12 + 6 (<1, 2>) and
10 + 6 (<1, 1>): every instance of the unit.
Plans of a few candidate tiles (the member fan and the micro tiles, which would take plans this small, are switched off):
n = 16 (one tile), 40 (ragged last tile), 272 (17 tiles); h = 1, 2, 3 (both parities of the exchange regions, a step that is
first and last, the clamp of the last step's action request); m = 1, 2."""

import numpy as np
import pytest
import torch

from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativeModel
from learning_to_adapt_amd.envs.reward_spec import RewardSpec
from learning_to_adapt_amd.utils import synthetic
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

SHAPES = {"o4": (20, 6), "o24": (24, 6), "o12": (12, 6), "o10": (10, 6)}
DISCOUNT = 0.95
NS, HS = (16, 40, 272), (1, 2, 3)


def _model_parts(obs_dim, act_dim, hidden, E):
    low, high = -np.ones(act_dim), np.ones(act_dim)
    sets = [synthetic.make_weight_set(obs_dim, act_dim, hidden, 1000 + e) for e in range(E)]
    norms = [synthetic.make_norm(obs_dim, act_dim, low, high, 2000 + e) for e in range(E)]
    return sets, norms


def _spec(obs_dim):
    return RewardSpec.make(w_vel=1.0, dt=0.05, ctrl_coef=0.05, vel_index=obs_dim - 3)


def _inputs(obs_dim, act_dim, m, n, h, seed=0):
    rs = np.random.RandomState(4000 + seed)
    return rs.randn(m, obs_dim), rs.uniform(-1.0, 1.0, (h, m * n, act_dim))


def oracle_returns(obs_dim, act_dim, hidden, E, obs0, acts, n, mlp_dtype=np.float64):
    """float64 [m, n]: oracle.planner.rollout_returns (``mlp_dtype=np.float32``: the oracle's own fp32 network path)."""
    from oracle import OracleMLPDynamics
    from oracle.planner import rollout_returns
    sets, norms = _model_parts(obs_dim, act_dim, hidden, E)
    dyn = OracleMLPDynamics(obs_dim, act_dim, sets, norms, mode="mean" if E > 1 else "single", hidden_nonlinearity="relu",
                            mlp_dtype=mlp_dtype)
    return rollout_returns(dyn, _spec(obs_dim).evaluate, obs0, acts, n, DISCOUNT).reshape(len(obs0), n)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


class _Model(object):
    def __init__(self, obs_dim, act_dim, hidden=(512, 512), E=5):
        self.obs_dim, self.act_dim, self.hidden, self.E = obs_dim, act_dim, list(hidden), E
        self.native = NativeModel(obs_dim, act_dim, self.hidden, "relu", None, E, "mean" if E > 1 else "single")
        sets, norms = _model_parts(obs_dim, act_dim, self.hidden, E)
        for e in range(E):
            self.native.set_weights(e, sets[e])
            self.native.set_norm(e, norms[e])
        self.dev = self.native.device
        self.spec = _spec(obs_dim)

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def plan(self, obs0, acts, m, n, h):
        rets = torch.full((m, n), float("nan"), dtype=torch.float32, device=self.dev)
        best = torch.zeros((m,), dtype=torch.int64, device=self.dev)
        self.native.plan_rs(obs0, acts, m, n, h, DISCOUNT, self.spec, cand_offset=100, returns_out=rets, best_key=best)
        torch.cuda.synchronize()
        return rets.cpu().numpy(), best.cpu().numpy()

    def is_static(self, m, n, h, **policy):
        return _lib.plan_geometry(self.obs_dim, self.act_dim, self.hidden, self.E, "mean" if self.E > 1 else "single", m, n, h,
                                  fan=0, micro=0, **policy)["seq3"]


@pytest.fixture(scope="module", params=sorted(SHAPES))
def model(request):
    md = _Model(*SHAPES[request.param])
    yield md
    md.native.close()


class _policies(object):
    """The tile split alone: matrix-core kernel, no member fan, no micro tiles; everything back to its default afterwards."""

    def __enter__(self):
        self.ctx = _lib.Context.get(0)
        self.ctx.set_kernel("mfma")
        self.ctx.set_fan(0)
        self.ctx.set_micro(0)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_kernel("auto")
        self.ctx.set_fan(1)
        self.ctx.set_micro(1)
        self.ctx.set_split(1)
        self.ctx.set_batch(0)
        self.ctx.set_seq3(1)


def _same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def _six_launches(ctx, md, obs0, acts, m, n, h, what):
    """Static step on, off (general tile-split instances), unsplit - each twice; returns the first (returns, keys)."""
    out = []
    for seq3, split in ((1, 1), (0, 1), (1, 0)):
        ctx.set_seq3(seq3)
        ctx.set_split(split)
        for _ in range(2):
            out.append(md.plan(obs0, acts, m, n, h))
        ctx.launch_status()                                  # raises unless clean
    names = ("static", "static again", "general", "general again", "unsplit", "unsplit again")
    for name, o in zip(names[1:], out[1:]):
        assert _same_bits(out[0], o), "%s: %s differs from the static step" % (what, name)
    return out[0]


@pytest.mark.parametrize("m", (1, 2))
def test_static_step_gives_the_bits_of_the_general_split_and_the_unsplit_launch(model, m):
    md = model
    with _policies() as ctx:
        for n in NS:
            obs0, acts = _inputs(md.obs_dim, md.act_dim, m, n, max(HS), seed=n + m)
            for h in HS:
                assert md.is_static(m, n, h) and not md.is_static(m, n, h, seq3=0) and not md.is_static(m, n, h, split=0)
                got, _ = _six_launches(ctx, md, md.up(obs0), md.up(acts[:h]), m, n, h, "m=%d n=%d h=%d" % (m, n, h))
                assert not np.isnan(got).any()
                want = oracle_returns(md.obs_dim, md.act_dim, md.hidden, md.E, obs0, acts[:h], n)
                err = rel_err(got, want)
                print("m=%d n=%d h=%d: rel_err %.3g" % (m, n, h, err))
                assert err < RTOL


def test_reference_fp32_path_sits_inside_the_bar():
    """The oracle's own fp32 network against its float64 one, for the seeds above (no GPU work: the bar is not set by the
    kernel under test)."""
    for name in sorted(SHAPES):
        od, ad = SHAPES[name]
        for m in (1, 2):
            for n in NS:
                obs0, acts = _inputs(od, ad, m, n, max(HS), seed=n + m)
                for h in HS:
                    want = oracle_returns(od, ad, [512, 512], 5, obs0, acts[:h], n)
                    err = rel_err(oracle_returns(od, ad, [512, 512], 5, obs0, acts[:h], n, mlp_dtype=np.float32), want)
                    assert err < RTOL, (name, m, n, h, err)


def test_carry_over_two_chunks_equals_the_single_launch(model):
    md = model
    m, n, h = 2, 40, 3
    obs0, acts = _inputs(md.obs_dim, md.act_dim, m, n, h, seed=7)
    o, a = md.up(obs0), md.up(acts)
    with _policies() as ctx:
        assert md.is_static(m, n, 1) and md.is_static(m, n, 2)
        single = md.plan(o, a, m, n, h)
        ret_a = torch.empty((m, n), dtype=torch.float32, device=md.dev)
        ret_b = torch.empty((m, n), dtype=torch.float32, device=md.dev)
        state = torch.empty((m * n, md.obs_dim), dtype=torch.float32, device=md.dev)
        best = torch.zeros((m,), dtype=torch.int64, device=md.dev)
        md.native.plan_rs_chunk(o, False, a[:1].contiguous(), m, n, 1, 0, DISCOUNT, md.spec, cand_offset=100, returns_out=ret_a,
                                state_out=state)
        md.native.plan_rs_chunk(state, True, a[1:].contiguous(), m, n, 2, 1, DISCOUNT, md.spec, cand_offset=100, returns_in=ret_a,
                                returns_out=ret_b, best_key=best)
        torch.cuda.synchronize()
        ctx.launch_status()
    assert _same_bits(single, (ret_b.cpu().numpy(), best.cpu().numpy()))


def test_non_finite_candidates_keep_their_bits(model):
    """One candidate with an action of 1e30 (its control cost overflows: -inf) and one with a NaN action among 32; the state's
    padding lanes must stay exact zeros (inf x 0), as in test_gpu_nonfinite.py."""
    md = model
    m, n, h = 1, 32, 3
    obs0, acts = _inputs(md.obs_dim, md.act_dim, m, n, h, seed=9)
    acts[0, 5, 0] = 1e30
    acts[1, 21, 2] = np.nan
    with _policies() as ctx:
        assert md.is_static(m, n, h)
        out = {}
        for name, seq3, split in (("static", 1, 1), ("general", 0, 1), ("unsplit", 1, 0)):
            ctx.set_seq3(seq3)
            ctx.set_split(split)
            out[name] = md.plan(md.up(obs0), md.up(acts), m, n, h)
            ctx.launch_status()
    got = out["static"][0]
    assert np.isinf(got[0, 5]) and np.isnan(got[0, 21])
    assert np.isfinite(np.delete(got[0], [5, 21])).all()
    for name in ("general", "unsplit"):
        assert np.array_equal(np.isnan(got), np.isnan(out[name][0]))
        assert np.array_equal(got, out[name][0], equal_nan=True) and np.array_equal(out["static"][1], out[name][1]), name
        fin = ~np.isnan(got)
        assert got[fin].tobytes() == out[name][0][fin].tobytes(), name


def test_thirty_steps():
    """The ring's and the prefetch's steady state over many steps: a slip of the exchange tag or of the region parity that
    three steps cannot show."""
    md = _Model(*SHAPES["o4"])
    try:
        m, n, h = 1, 64, 30
        obs0, acts = _inputs(md.obs_dim, md.act_dim, m, n, h, seed=30)
        with _policies() as ctx:
            assert md.is_static(m, n, h)
            got, _ = _six_launches(ctx, md, md.up(obs0), md.up(acts), m, n, h, "h=30")
        err = rel_err(got, oracle_returns(md.obs_dim, md.act_dim, md.hidden, md.E, obs0, acts, n))
        print("h=30: rel_err %.3g" % err)
        assert err < RTOL
    finally:
        md.native.close()


@pytest.mark.parametrize("hidden,E,batch", [((512, 512), 3, 0), ((512, 512), 7, 0), ((512, 512), 5, 2), ((256, 256), 5, 0)],
                         ids=["E3", "E7", "E5-batch2", "E5-2x256"])
def test_neighbours_stay_on_the_general_path(hidden, E, batch):
    md = _Model(20, 6, hidden, E)
    try:
        m, n, h = 1, 40, 3
        obs0, acts = _inputs(20, 6, m, n, h, seed=E)
        out = []
        with _policies() as ctx:
            ctx.set_batch(batch)
            assert not md.is_static(m, n, h, batch=batch)
            for seq3 in (1, 0):
                ctx.set_seq3(seq3)
                out.append(md.plan(md.up(obs0), md.up(acts), m, n, h))
                ctx.launch_status()
        assert _same_bits(out[0], out[1])
        assert rel_err(out[0][0], oracle_returns(20, 6, list(hidden), E, obs0, acts, n)) < RTOL
    finally:
        md.native.close()
