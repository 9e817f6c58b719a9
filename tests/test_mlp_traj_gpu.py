"""The MLP planner's trajectory rollout on the GPU (``l2a_rollout_traj``: one launch of ``l2a_mlp_micro_k<UW, GACT, true>``, or the
carry chain): against the float64 oracle, the single launch against the chain bit for bit, guard rows, an unaligned ``traj_out``,
``cand_offset``, a diverged candidate, the bits of ``l2a_plan_rs_program`` / ``l2a_plan_rs_reward_model`` under both paths, shards
and the unsplit geometry, and ``MPCController`` on a program env at the GrBAL default geometry.

The plan sizes follow the device's real CU count; a row is skipped only where ``mlp_traj_geometry`` says the chain for it.  The
figures the tests print (maximum of ``|got - want| / max(1, |want|)``, bar 1e-4) are recorded in DESIGN section 4.8."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import cases
import cem_ties
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativeModel, NativeRewardModel
from learning_to_adapt_amd.policies import MPCController
from learning_to_adapt_amd.utils import synthetic
from mlp_traj_rows import ROWS, row_n
from oracle import OracleMLPDynamics
from oracle.planner import cem_plan, rollout_trace, rs_plan

gpu = pytest.mark.gpu       # (every test but the host-only check of the rows at the end of the file)

RTOL = 1e-4         # against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
MARGIN = 1e-3       # top-2 margin of the oracle's returns in the controller cases (a condition on the inputs)
GUARD, SENTINEL = 3, -777.25
OFFSET = 1000
DT = 0.05
RM_HIDDEN, RM_ACT = (128, 64), "tanh"


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _ctx():
    return _lib.Context.get(0)


def _cus():
    return _ctx().info()["compute_units"]           # read from the context, not assumed


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


@pytest.fixture(autouse=True)
def _policies(request):
    if request.node.get_closest_marker("gpu") is None:
        yield None
        return
    ctx = _ctx()
    yield ctx
    ctx.set_micro(1)
    ctx.set_split(0 if getattr(ctx, "split_degraded", False) else 1)


@functools.lru_cache(maxsize=None)
def _case(rid):
    """Model, inputs and the float64 trace of a row: built once, shared by the tests, never modified."""
    r = next(r for r in ROWS if r["id"] == rid)
    od, ad, m, h, E, mode = r["od"], r["ad"], r["m"], r["h"], r["E"], r["mode"]
    n = row_n(r, _cus())
    seed = 300 + [x["id"] for x in ROWS].index(rid)
    rs = np.random.RandomState(seed)
    low, high = -np.ones(ad), np.ones(ad)
    sets = [synthetic.make_weight_set(od, ad, list(r["hidden"]), seed + 10 * (e + 1)) for e in range(E)]
    norms = [synthetic.make_norm(od, ad, low, high, seed + 10 * (e + 1) + 1) for e in range(E)]
    dyn = OracleMLPDynamics(od, ad, sets, norms, mode=mode, hidden_nonlinearity=r["act"])
    obs0 = rs.randn(m, od).astype(np.float32)
    acts = rs.uniform(low, high, (h, m * n, ad)).astype(np.float32)
    prog = rpc.new_reward_program(od, ad, DT)
    want, states = rollout_trace(dyn, prog.evaluate, obs0.astype(np.float64), acts.astype(np.float64), n, 1.0)
    assert np.all(np.isfinite(states)), "the oracle's trajectory of %s is not finite" % rid
    states.setflags(write=False)
    native = NativeModel(od, ad, list(r["hidden"]), r["act"], None, E, mode)
    for e in range(E):
        native.set_weights(e, sets[e])
        native.set_norm(e, norms[e])
    rm = NativeRewardModel(od, ad, RM_HIDDEN, RM_ACT)
    rm.set_weights(rmc.reward_weights(od, ad, RM_HIDDEN))
    rm.set_norm(rmc.reward_norm(od, ad, base=norms[0]))
    return dict(id=rid, row=r, od=od, ad=ad, m=m, n=n, h=h, native=native, rm=rm, prog=prog, obs0=obs0, acts=acts, states=states,
                want=want.reshape(m, n))


def _geometry(c, micro):
    r = c["row"]
    return _lib.mlp_traj_geometry(c["od"], c["ad"], len(r["hidden"]), r["hidden"][0], r["mode"], r["E"], c["m"], c["n"], c["h"],
                                  micro=micro, cus=_cus())


def _single_or_skip(c):
    assert not _geometry(c, 0)["single"]
    if not _geometry(c, 2)["single"]:
        pytest.skip("%s: the geometry says the chain on %d CUs" % (c["id"], _cus()))


def _shard(c, lo, hi):
    m, n, h = c["m"], c["n"], c["h"]
    return np.ascontiguousarray(c["acts"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * (hi - lo), -1))


def _rollout(c, micro, cand_offset=0, shift=0, acts=None):
    """``l2a_rollout_traj`` into a buffer between guard rows (``shift`` floats off its 16-byte alignment): ``[h, m n, obs_dim]``."""
    ctx, native = _ctx(), c["native"]
    ctx.set_micro(micro)
    m, n, h, od = c["m"], c["n"], c["h"], c["od"]
    body = h * m * n * od
    full = torch.full((4 + body + 2 * GUARD * od,), SENTINEL, dtype=torch.float32, device="cuda:0")
    assert full.data_ptr() % 16 == 0
    start = shift + GUARD * od
    inner = full[start:start + body]
    inner.fill_(float("nan"))
    assert inner.data_ptr() % 16 == (4 * start) % 16
    native.rollout_traj(_dev(c["obs0"]), _dev(c["acts"] if acts is None else acts), m, n, h, cand_offset=cand_offset,
                        traj_out=inner.view(h, m * n, od))
    torch.cuda.synchronize()
    assert ctx.launch_status_value() == 0
    host = full.cpu().numpy()
    assert np.all(host[:start] == np.float32(SENTINEL)) and np.all(host[start + body:] == np.float32(SENTINEL)), "guard rows overwritten"
    return host[start:start + body].reshape(h, m * n, od)


def _plan(c, kind, micro, cand_offset=0, lo=None, hi=None, want_traj=True, split=None):
    ctx, native = _ctx(), c["native"]
    ctx.set_micro(micro)
    if split is not None:
        ctx.set_split(split)
    m, n, h = c["m"], c["n"], c["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    a = _shard(c, lo, hi)
    rets = torch.full((m, nl), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    traj = torch.full((h, m * nl, c["od"]), float("nan"), dtype=torch.float32, device="cuda:0") if want_traj else None
    args = (_dev(c["obs0"]), _dev(a), m, nl, h, 1.0)
    if kind == "program":
        native.plan_rs_program(*args, c["prog"], cand_offset=cand_offset, returns_out=rets, best_key=best, traj_out=traj)
    else:
        native.plan_rs_reward_model(*args, c["rm"], cand_offset=cand_offset, returns_out=rets, best_key=best, traj_out=traj)
    torch.cuda.synchronize()
    assert ctx.launch_status_value() == 0
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64), (traj.cpu().numpy() if want_traj else None)


# ------------------------------------------------------------------------------------------
# 1. the rollout against the float64 oracle; single launch = chain, bit for bit; guards, alignment, cand_offset
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_rollout_matches_the_oracle_and_both_paths_give_the_same_bits(rid):
    c = _case(rid)
    _single_or_skip(c)
    traj = _rollout(c, 2)
    assert not np.any(np.isnan(traj)), "rows left unwritten: %s" % np.unique(np.nonzero(np.isnan(traj))[1])[:8]
    err = rel_err(traj, c["states"])
    print("%s rollout_traj (single launch, %s): states %.3e against the float64 oracle" % (rid, _geometry(c, 2), err))
    assert err <= RTOL
    chain = _rollout(c, 0)
    print("%s chain: states %.3e" % (rid, rel_err(chain, c["states"])))
    assert np.all(np.isfinite(traj)) and np.array_equal(_bits(chain), _bits(traj)), "single launch differs from the carry chain"
    assert np.array_equal(_bits(_rollout(c, 2, shift=1)), _bits(traj)), "traj_out one float off its alignment"
    assert np.array_equal(_bits(_rollout(c, 2, cand_offset=OFFSET)), _bits(traj))         # cand_offset: nothing in the trajectory
    # the library's own buffer (traj_out NULL) feeds the plan entries: covered by want_traj=False below


# ------------------------------------------------------------------------------------------
# 2. the plan entries: policy 2 against policy 0, shards, the unsplit geometry
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["program", "model"])
@pytest.mark.parametrize("rid", [r["id"] for r in ROWS])
def test_plan_entries_keep_their_bits(rid, kind):
    c = _case(rid)
    _single_or_skip(c)
    n = c["n"]
    rets, keys, traj = _plan(c, kind, 0)
    if kind == "program":
        err = rel_err(rets, c["want"])
        print("%s program: returns %.3e against the float64 oracle" % (rid, err))
        assert err <= RTOL
    assert np.array_equal(keys, _want_keys(rets, 0))
    for kw in (dict(micro=2), dict(micro=2, want_traj=False), dict(micro=2, split=0), dict(micro=0, split=0)):
        r2, k2, t2 = _plan(c, kind, kw.pop("micro"), **kw)
        assert np.array_equal(_bits(r2), _bits(rets)) and np.array_equal(k2, keys), kw
        assert t2 is None or np.array_equal(_bits(t2), _bits(traj)), kw
    _ctx().set_split(0 if getattr(_ctx(), "split_degraded", False) else 1)
    if n >= 3:
        cut = (n // 2) | 1          # two shards cut at an odd candidate
        ra, ka, ta = _plan(c, kind, 2, cand_offset=OFFSET, lo=0, hi=cut)
        rb, kb, tb = _plan(c, kind, 2, cand_offset=OFFSET + cut, lo=cut, hi=n)
        assert np.array_equal(_bits(np.concatenate([ra, rb], axis=1)), _bits(rets))
        assert np.array_equal(np.maximum(ka, kb), _want_keys(rets, OFFSET))
        m, h, od = c["m"], c["h"], c["od"]
        both = np.concatenate([ta.reshape(h, m, cut, od), tb.reshape(h, m, n - cut, od)], axis=2).reshape(h, m * n, od)
        assert np.array_equal(_bits(both), _bits(traj))


@gpu
def test_entry_point_validates():
    c = _case(ROWS[0]["id"])
    native, lib = c["native"], _lib.load()
    m, n, h = c["m"], c["n"], c["h"]
    o, a = _dev(c["obs0"]), _dev(c["acts"])
    traj = torch.empty((h, m * n, c["od"]), dtype=torch.float32, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    null = ctypes.c_void_p()

    def rollout(obs=p(o), act=p(a), m_=m, n_=n, h_=h, off=0, out=p(traj)):
        return lib.l2a_rollout_traj(native.handle, obs, act, m_, n_, h_, off, out, null)

    for kw in (dict(obs=null), dict(act=null), dict(m_=0), dict(n_=0), dict(h_=0), dict(off=-1), dict(m_=1 << 15, n_=1 << 15),
               dict(off=0x7fffffff)):
        assert rollout(**kw) == _lib.L2A_EINVAL, kw
        assert len(lib.l2a_last_error(native.ctx.handle)) > 0
    for micro in (2, 0):
        _ctx().set_micro(micro)
        assert rollout() == _lib.L2A_OK and rollout(out=null) == _lib.L2A_OK      # (NULL: the model's own buffer)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 3. a diverged candidate
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rid", ["h512x2_o4_n37", "h512x2_mean3_above_cus"])
def test_a_diverged_candidate_stays_alone(rid):
    """Two actions of one candidate per env are +inf at step 0: its states are non-finite for the rest of the horizon, on the
    single launch and on the chain alike; every other candidate - its micro-tile neighbours included - keeps the bits it has in
    the undisturbed plan."""
    c = _case(rid)
    _single_or_skip(c)
    m, n, h = c["m"], c["n"], c["h"]
    victims = np.array([e * n + (5 + 9 * e) % n for e in range(m)])
    acts = c["acts"].copy()
    acts[0, victims, 0] = np.inf
    acts[0, victims, 1] = np.inf
    clean = _rollout(c, 2)
    others = np.ones(m * n, dtype=bool)
    others[victims] = False
    got = {}
    for micro in (2, 0):
        traj = got[micro] = _rollout(c, micro, acts=acts)
        assert not np.any(np.isfinite(traj[:, victims])), "the diverged candidate came back finite"
        assert np.array_equal(_bits(traj[:, others]), _bits(clean[:, others])), "a neighbour of the diverged candidate changed (micro %d)" % micro
    assert np.array_equal(np.isnan(got[2]), np.isnan(got[0])) and np.array_equal(got[2][:, others], got[0][:, others])


# ------------------------------------------------------------------------------------------
# 4. through the controller: a program env at the GrBAL default geometry (5 adapted 3 x 512 sets, n = 500), h cut to 3
# ------------------------------------------------------------------------------------------
GRBAL = dict(name="grbal_default_h3", E=5, env="ant", h=3, hidden=[512, 512, 512], m=5, mode="per_block", n=500, planner="rs")
SEED = 2            # (of seeds 0 .. 2 the one whose ORACLE returns keep the top-2 margin in both controller cases)


def _controller(**kw):
    env = rpc.program_env(GRBAL["env"])
    _, model = cases.product_model(GRBAL)
    kw.setdefault("use_cem", False)
    ctrl = MPCController(name="policy", env=env, dynamics_model=model, discount=1.0, n_candidates=GRBAL["n"], horizon=GRBAL["h"], **kw)
    obs = synthetic.make_obs0(GRBAL["m"], env.observation_space.shape[0])
    return env, model, ctrl, obs


def _margin(returns):
    top = np.sort(returns, axis=1)
    return float(np.min((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1]))))


@gpu
def test_controller_random_shooting_like_the_oracle():
    env, model, ctrl, obs = _controller(rng="numpy")
    assert ctrl._program()
    np.random.seed(SEED)
    want, best, returns, _ = rs_plan(cases.oracle_dynamics(GRBAL), env.reward, obs, env.action_space.low, env.action_space.high,
                                     GRBAL["n"], GRBAL["h"], 1.0)
    rng_next = np.random.uniform()
    print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
    assert _margin(returns) >= MARGIN
    np.random.seed(SEED)
    got, info = ctrl.get_actions(obs)
    assert np.random.uniform() == rng_next
    assert info == {} and model.planner_model().program_plans == 1
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert rel_err(ctrl.last_plan["best_return"], returns[np.arange(GRBAL["m"]), best]) <= RTOL


@gpu
def test_controller_cem_teacher_forced_like_the_oracle():
    """Every CEM iteration on its own (``cem_mode="reference"``), started from the ORACLE's mean / std of the previous one with
    the same normal draws, so that no rank tie can decide the outcome; the last iteration picks the oracle's candidate."""
    iters = 2
    env, model, ctrl, obs = _controller(rng="numpy", use_cem=True, num_cem_iters=iters, cem_mode="reference")
    m, n, h = GRBAL["m"], GRBAL["n"], GRBAL["h"]
    act_dim = env.action_space.shape[0]
    k = max(int(n * ctrl.percent_elites), 1)
    trace = []
    np.random.seed(SEED)
    want, best, returns = cem_plan(cases.oracle_dynamics(GRBAL), env.reward, obs, env.action_space.low, env.action_space.high, n, h,
                                   1.0, num_cem_iters=iters, percent_elites=ctrl.percent_elites, trace=trace)
    rng_next = np.random.uniform()
    print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
    assert _margin(returns) >= MARGIN
    clip_low = np.concatenate([env.action_space.low] * h)
    clip_high = np.concatenate([env.action_space.high] * h)
    np.random.seed(SEED)
    mean, std = np.zeros((m, h * act_dim)), np.ones((m, h * act_dim))
    for it in range(iters):
        _, _, mine, cand_a = ctrl._cem_iteration(obs, mean, std, k, clip_low, clip_high, 0, n, 1)
        err = rel_err(mine, trace[it]["returns"])
        print("CEM iteration %d: returns %.2e against the float64 oracle" % (it, err))
        assert err <= RTOL
        cem_ties.assert_flips_are_ties(mine, trace[it]["returns"], k, RTOL)
        mean, std = trace[it]["mean"], trace[it]["std"]             # teacher forcing
    assert np.random.uniform() == rng_next
    idx = np.argmax(mine, axis=1)
    assert np.array_equal(idx, best)
    np.testing.assert_array_equal(cand_a[np.arange(m), idx], want)
    assert model.planner_model().program_plans == iters


# ------------------------------------------------------------------------------------------
# 5. host only: on a 256-CU device at most two of the rows fall back to the chain (and so skip above)
# ------------------------------------------------------------------------------------------
def test_rows_take_the_single_launch_on_256_cus():
    chain = []
    for r in ROWS:
        n = row_n(r, 256)
        g = _lib.mlp_traj_geometry(r["od"], r["ad"], len(r["hidden"]), r["hidden"][0], r["mode"], r["E"], r["m"], n, r["h"], micro=2, cus=256)
        if not g["single"]:
            chain.append(r["id"])
    assert len(chain) <= 2, chain
    sizes = {r["id"]: _lib.mlp_traj_geometry(r["od"], r["ad"], len(r["hidden"]), r["hidden"][0], r["mode"], r["E"], r["m"], row_n(r, 256),
                                            r["h"], micro=2, cus=256)["micro_tiles"] for r in ROWS}
    assert sorted(set(sizes.values())) == [1, 2, 3], sizes          # workgroups of one, two and three micro tiles are all there
