"""The recurrent planner with a reward program or a learned reward model, on the GPU: the trajectory rollout
(``l2a_lstm_rollout_traj``: one launch of ``l2a_lstm_micro_k<UW, true>``, or the carry chain) against the float64 oracle, the
single launch against the chain bit for bit, the bits of the two plan entries, a diverged candidate, and ``RNNMPCController``.

The figures the tests print (maximum of ``|got - want| / max(1, |want|)``, bar 1e-4) are recorded in DESIGN section 4.10.
Sharding is covered by the two-shard bit test (shards cut at an odd candidate with ``cand_offset``), not by gloo ranks: a rank's
plan is exactly such a call, and the collective behind it is the one the existing distributed tests cover."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import cases
import cem_ties
import nonfinite_cases
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics import MLPRewardModel
from learning_to_adapt_amd.dynamics.native_lstm import NativeLSTM
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
from learning_to_adapt_amd.policies import RNNMPCController
from learning_to_adapt_amd.utils import synthetic
from oracle import LSTMStateTuple, OracleLSTMDynamics, OracleRNNStackDynamics
from oracle.rnn_planner import rnn_cem_plan, rnn_rollout_trace, rnn_rs_plan

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
MARGIN = 1e-3       # top-2 margin of the oracle's returns in every controller case (a condition on the inputs)
GUARD, SENTINEL = 3, -777.25
OFFSET = 1000
DT = 0.05
RM_HIDDEN, RM_ACT = (128, 64), "tanh"

#        id,            cell,   layers,     obs, act, m, n,    h, kernel, single launch under l2a_set_micro(2)
ROWS = [("u256_mt1", "lstm", (256,), 20, 6, 2, 37, 3, "auto", True),            # MT = 1, ragged last tile, 16-byte stores
        ("u256_mt3_2", "lstm", (256,), 41, 8, 5, 500, 2, "auto", True),         # workgroups of 3 and 2 micro tiles, dword stores, 3 obs tiles
        ("u512_mt2_1", "lstm", (512,), 17, 5, 1, 1100, 2, "auto", True),        # UW = 2, workgroups of 2 and 1 micro tile
        ("u256_limits", "lstm", (256,), 64, 16, 3, 70, 2, "auto", True),        # every dimension limit
        ("u128", "lstm", (128,), 20, 6, 2, 40, 3, "auto", False),               # chain: the tuned 16-candidate kernel
        ("u128_valu", "lstm", (128,), 20, 6, 2, 40, 3, "valu", False),          # chain: the VALU kernel
        ("gru256", "gru", (256,), 20, 6, 2, 40, 3, "auto", False),              # chain: the generic matrix-core kernel
        ("lstm2x256", "lstm", (256, 256), 20, 6, 2, 40, 3, "auto", False)]
SINGLE = [r for r in ROWS if r[-1]]


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _ctx():
    return _lib.Context.get(0)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def _want_keys(returns, cand_offset):
    """``l2a_key_encode`` of the NumPy arg-max (first maximum; a NaN is the maximum) of every env's returns."""
    return np.array([_encode(row[int(np.argmax(row))], cand_offset + int(np.argmax(row))) for row in returns], dtype=np.uint64)


@pytest.fixture(autouse=True)
def _policies():
    ctx = _ctx()
    yield ctx
    ctx.set_micro(1)
    ctx.set_kernel("auto")
    ctx.set_split(0 if getattr(ctx, "split_degraded", False) else 1)


def _flat_hidden(cell, layers):
    layers = layers if isinstance(layers, list) else [layers]
    if cell == "lstm":
        return np.concatenate([l.c for l in layers], axis=1), np.concatenate([l.h for l in layers], axis=1)
    h = np.concatenate(layers, axis=1)
    return np.zeros_like(h), h


@functools.lru_cache(maxsize=None)
def _case(rid):
    """Model, inputs and the float64 trace of a row: built once, shared by the tests, never modified."""
    _, cell, sizes, od, ad, m, n, h, kernel, single = next(r for r in ROWS if r[0] == rid)
    seed = 100 + [r[0] for r in ROWS].index(rid.replace("_valu", ""))
    rs = np.random.RandomState(seed)
    low, high = -np.ones(ad), np.ones(ad)
    generic = cell != "lstm" or len(sizes) > 1
    if generic:
        params = synthetic.make_rnn_stack_set(od, ad, list(sizes), cell, seed + 1)
    else:
        params = synthetic.make_lstm_set(od, ad, sizes[0], seed + 1)
    norm = synthetic.make_norm(od, ad, low, high, seed + 2)
    if generic:
        dyn = OracleRNNStackDynamics(od, ad, list(sizes), cell, params, norm, hidden_nonlinearity="tanh", dtype=np.float64)
    else:
        dyn = OracleLSTMDynamics(od, ad, params, norm, hidden_nonlinearity="tanh", dtype=np.float64)
    layers = []
    for u in sizes:
        c, hh = rs.randn(m, u).astype(np.float32), np.tanh(rs.randn(m, u)).astype(np.float32)
        layers.append(LSTMStateTuple(c, hh) if cell == "lstm" else hh)
    hid = layers if len(layers) > 1 else layers[0]
    obs0 = rs.randn(m, od).astype(np.float32)
    acts = rs.uniform(low, high, (h, m * n, ad)).astype(np.float32)
    prog = rpc.new_reward_program(od, ad, DT)
    rm_params, rm_norm = rmc.reward_weights(od, ad, RM_HIDDEN), rmc.reward_norm(od, ad, base=norm)
    rm_fn = rmc.reward_fn(rm_params, rm_norm, RM_ACT)
    want = {}
    states = None
    for disc in (1.0, 0.9):
        for name, fn in (("program", prog.evaluate), ("model", rm_fn)):
            ret, states, _ = rnn_rollout_trace(dyn, fn, obs0.astype(np.float64), hid, acts.astype(np.float64), n, disc)
            want[name, disc] = ret.reshape(m, n)
    assert np.all(np.isfinite(states)), "the oracle's trajectory of %s is not finite" % rid
    states.setflags(write=False)
    native = NativeLSTM(od, ad, list(sizes) if generic else sizes[0], "tanh", None, cell_type=cell)
    native.set_weights(params)
    native.set_norm(norm)
    rm = NativeRewardModel(od, ad, RM_HIDDEN, RM_ACT)
    rm.set_weights(rm_params)
    rm.set_norm(rm_norm)
    c_flat, h_flat = _flat_hidden(cell, hid)
    return dict(id=rid, od=od, ad=ad, m=m, n=n, h=h, kernel=kernel, single=single, units=sizes, native=native, rm=rm, prog=prog,
                obs0=obs0, acts=acts, c0=c_flat, h0=h_flat, states=states, want=want)


def _geometry(c, micro):
    cus = _ctx().info()["compute_units"]            # read from the context, not assumed
    if len(c["units"]) > 1 or c["native"].cell_type != "lstm" or c["kernel"] == "valu":
        return dict(single=False)
    return _lib.lstm_traj_geometry(c["od"], c["ad"], c["units"][0], c["m"], c["n"], c["h"], micro=micro, cus=cus)


def _shard(c, lo, hi):
    m, n, h = c["m"], c["n"], c["h"]
    return np.ascontiguousarray(c["acts"].reshape(h, m, n, -1)[:, :, lo:hi].reshape(h, m * (hi - lo), -1))


def _rollout(c, micro, cand_offset=0):
    """``l2a_lstm_rollout_traj`` into a buffer between guard rows: the trajectory ``[h, m n, obs_dim]``."""
    ctx, native = _ctx(), c["native"]
    ctx.set_micro(micro)
    ctx.set_kernel(c["kernel"])
    m, n, h, od = c["m"], c["n"], c["h"], c["od"]
    full = torch.full((h * m * n + 2 * GUARD, od), SENTINEL, dtype=torch.float32, device="cuda:0")
    inner = full[GUARD:GUARD + h * m * n]
    inner.fill_(float("nan"))
    native.rollout_traj(_dev(c["obs0"]), _dev(c["c0"]), _dev(c["h0"]), _dev(c["acts"]), m, n, h, cand_offset=cand_offset,
                        traj_out=inner.view(h, m * n, od))
    torch.cuda.synchronize()
    assert ctx.launch_status_value() == 0
    host = full.cpu().numpy()
    assert np.all(host[:GUARD] == np.float32(SENTINEL)) and np.all(host[-GUARD:] == np.float32(SENTINEL)), "guard rows overwritten"
    traj = host[GUARD:-GUARD].reshape(h, m * n, od)
    assert not np.any(np.isnan(traj)), "rows left unwritten: %s" % np.unique(np.nonzero(np.isnan(traj))[1])[:8]
    return traj


def _plan(c, kind, micro, discount=1.0, cand_offset=0, lo=None, hi=None, want_traj=True, split=None, acts=None):
    ctx, native = _ctx(), c["native"]
    ctx.set_micro(micro)
    ctx.set_kernel(c["kernel"])
    if split is not None:
        ctx.set_split(split)
    m, n, h = c["m"], c["n"], c["h"]
    lo, hi = (0, n) if lo is None else (lo, hi)
    nl = hi - lo
    a = _shard(c, lo, hi) if acts is None else acts
    rets = torch.full((m, nl), -123.5, dtype=torch.float32, device="cuda:0")
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    traj = torch.full((h, m * nl, c["od"]), float("nan"), dtype=torch.float32, device="cuda:0") if want_traj else None
    args = (_dev(c["obs0"]), _dev(c["c0"]), _dev(c["h0"]), _dev(a), m, nl, h, discount)
    if kind == "program":
        native.plan_rs_program(*args, c["prog"], cand_offset=cand_offset, returns_out=rets, best_key=best, traj_out=traj)
    else:
        native.plan_rs_reward_model(*args, c["rm"], cand_offset=cand_offset, returns_out=rets, best_key=best, traj_out=traj)
    torch.cuda.synchronize()
    assert ctx.launch_status_value() == 0
    return rets.cpu().numpy(), best.cpu().numpy().view(np.uint64), (traj.cpu().numpy() if want_traj else None), a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------
# 1. the rollout against the float64 oracle; 2. single launch = chain, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_rollout_matches_the_oracle_and_both_paths_give_the_same_bits(rid):
    c = _case(rid)
    assert _geometry(c, 2)["single"] == c["single"] and not _geometry(c, 0)["single"]
    traj = _rollout(c, 2)
    err = rel_err(traj, c["states"])
    print("%s rollout_traj (%s): states %.3e against the float64 oracle" % (rid, "single launch" if c["single"] else "chain", err))
    assert err <= RTOL
    assert np.array_equal(_bits(_rollout(c, 2, cand_offset=OFFSET)), _bits(traj))         # cand_offset: nothing in the trajectory
    if c["single"]:
        chain = _rollout(c, 0)
        print("%s chain: states %.3e" % (rid, rel_err(chain, c["states"])))
        assert np.all(np.isfinite(traj)) and np.array_equal(_bits(chain), _bits(traj)), "single launch differs from the carry chain"


# ------------------------------------------------------------------------------------------
# 3. the bits of the plan entries; 4. returns against the oracle
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["program", "model"])
@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_plan_entries(rid, kind):
    c = _case(rid)
    m, n, h = c["m"], c["n"], c["h"]
    obs_rows = np.repeat(c["obs0"], n, axis=0)
    base = None
    for disc in (1.0, 0.9):
        rets, keys, traj, a = _plan(c, kind, 2, disc)
        err = rel_err(rets, c["want"][kind, disc])
        print("%s %s discount %.1f: returns %.3e against the float64 oracle" % (rid, kind, disc, err))
        assert err <= RTOL
        # the returns ARE the scorer applied to the entry's own trajectory; keys = first maximum of the entry's own returns
        score_r = torch.full((m * n,), -123.5, dtype=torch.float32, device="cuda:0")
        score_k = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
        if kind == "program":
            _ctx().score_trajectory(_dev(c["obs0"]), _dev(traj), _dev(a), m, n, h, disc, c["prog"], returns_out=score_r, best_key=score_k)
            again = c["prog"].returns_f32(obs_rows, traj, a, disc)
            assert np.array_equal(_bits(rets.reshape(-1)), _bits(again)), "not RewardProgram.evaluate_f32 of the trajectory"
        else:
            c["rm"].score_trajectory(_dev(c["obs0"]), _dev(traj), _dev(a), m, n, h, disc, returns_out=score_r, best_key=score_k)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(score_r.cpu().numpy()), _bits(rets.reshape(-1)))
        assert np.array_equal(score_k.cpu().numpy().view(np.uint64), keys) and np.array_equal(keys, _want_keys(rets, 0))
        if disc == 1.0:
            base = (rets, keys, traj)
    rets, keys, traj = base
    # the library's own trajectory buffer; the chain (micro policy 0); the unsplit geometry: the same bits
    variants = [dict(micro=2, want_traj=False), dict(micro=0), dict(micro=2, split=0), dict(micro=0, split=0)]
    for kw in variants:
        r2, k2, t2, _ = _plan(c, kind, kw.pop("micro"), 1.0, **kw)
        assert np.array_equal(_bits(r2), _bits(rets)) and np.array_equal(k2, keys), kw
        assert t2 is None or np.array_equal(_bits(t2), _bits(traj)), kw
    _ctx().set_split(0 if getattr(_ctx(), "split_degraded", False) else 1)
    # two shards cut at an odd candidate
    cut = (n // 2) | 1
    for micro in (2, 0):
        ra, ka, _, _ = _plan(c, kind, micro, 1.0, cand_offset=OFFSET, lo=0, hi=cut, want_traj=False)
        rb, kb, _, _ = _plan(c, kind, micro, 1.0, cand_offset=OFFSET + cut, lo=cut, hi=n, want_traj=False)
        assert np.array_equal(_bits(np.concatenate([ra, rb], axis=1)), _bits(rets))
        assert np.array_equal(np.maximum(ka, kb), _want_keys(rets, OFFSET))


def test_entry_points_validate():
    c = _case("u256_mt1")
    native, lib = c["native"], _lib.load()
    m, n, h = c["m"], c["n"], c["h"]
    o, c0, h0, a = _dev(c["obs0"]), _dev(c["c0"]), _dev(c["h0"]), _dev(c["acts"])
    rets = torch.empty((m, n), dtype=torch.float32, device="cuda:0")
    traj = torch.empty((h, m * n, c["od"]), dtype=torch.float32, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    null = ctypes.c_void_p()

    def rollout(obs=p(o), cc=p(c0), hh=p(h0), act=p(a), m_=m, n_=n, h_=h, off=0, out=p(traj)):
        return lib.l2a_lstm_rollout_traj(native.handle, obs, cc, hh, act, m_, n_, h_, off, out, null)

    def program(obs=p(o), cc=p(c0), hh=p(h0), act=p(a), m_=m, n_=n, h_=h, off=0, ret=p(rets), prog=c["prog"]):
        return lib.l2a_lstm_plan_rs_program(native.handle, obs, cc, hh, act, m_, n_, h_, 1.0, ctypes.byref(prog), off, ret, null, null, null)

    def model(obs=p(o), cc=p(c0), hh=p(h0), act=p(a), m_=m, n_=n, h_=h, off=0, ret=p(rets), rm=c["rm"].handle):
        return lib.l2a_lstm_plan_rs_reward_model(native.handle, rm, obs, cc, hh, act, m_, n_, h_, 1.0, off, ret, null, null, null)

    for entry in (rollout, program, model):
        for kw in (dict(obs=null), dict(cc=null), dict(hh=null), dict(act=null), dict(m_=0), dict(n_=0), dict(h_=0), dict(off=-1),
                   dict(m_=1 << 15, n_=1 << 15), dict(off=0x7fffffff)):
            assert entry(**kw) == _lib.L2A_EINVAL, (entry.__name__, kw)
            assert len(lib.l2a_last_error(native.ctx.handle)) > 0
    assert rollout(out=null) == _lib.L2A_EINVAL and program(ret=null) == _lib.L2A_EINVAL and model(ret=null) == _lib.L2A_EINVAL
    assert model(rm=null) == _lib.L2A_EINVAL
    bad = rpc.new_reward_program(c["od"] + 40, c["ad"], DT)             # a range outside the observation
    assert program(prog=bad) == _lib.L2A_EINVAL
    for od, ad in ((c["od"] + 1, c["ad"]), (c["od"], c["ad"] + 1)):
        other = NativeRewardModel(od, ad, (64,), "relu")
        other.set_weights(rmc.reward_weights(od, ad, (64,)))
        with pytest.raises(_lib.L2AError, match=r"\(-1\).*the reward model is for obs_dim"):
            native.plan_rs_reward_model(o, c0, h0, a, m, n, h, 1.0, other, returns_out=rets)
    main = _lib.Context.get(0)
    try:
        _lib.Context._by_device[0] = _lib.Context(0)
        foreign = NativeRewardModel(c["od"], c["ad"], (64,), "relu")
    finally:
        _lib.Context._by_device[0] = main
    foreign.set_weights(rmc.reward_weights(c["od"], c["ad"], (64,)))
    with pytest.raises(_lib.L2AError, match=r"\(-1\).*another context"):
        native.plan_rs_reward_model(o, c0, h0, a, m, n, h, 1.0, foreign, returns_out=rets)
    torch.cuda.synchronize()
    assert rollout() == _lib.L2A_OK and program() == _lib.L2A_OK and model() == _lib.L2A_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------
# 5. a diverged candidate
# ------------------------------------------------------------------------------------------
def test_a_diverged_candidate_stays_alone():
    """a0 = a1 = +inf at step 0 (tests/nonfinite_cases.rnn_case): NaN states for the rest of the horizon.  The return of such a
    candidate is non-finite by the scorers' rule (NaN for the reward model, and a NaN wins the arg-max); every other candidate
    has the bits it has in a plan whose diverging actions are replaced by zeros - on the single launch and on the chain."""
    nc = nonfinite_cases.rnn_case("lstm", [256], m=2, n=100, h=3)
    od, ad, m, n, h = nc["obs_dim"], nc["act_dim"], nc["m"], nc["n"], nc["h"]
    native = NativeLSTM(od, ad, 256, "tanh", None)
    native.set_weights(nc["params"])
    native.set_norm(nc["norm"])
    rm = NativeRewardModel(od, ad, RM_HIDDEN, RM_ACT)
    rm.set_weights(rmc.reward_weights(od, ad, RM_HIDDEN))
    rm.set_norm(rmc.reward_norm(od, ad, base=nc["norm"]))
    zeros = np.zeros((m, 256), dtype=np.float32)
    c = dict(native=native, rm=rm, prog=rpc.new_reward_program(od, ad, DT), obs0=nc["obs0"].astype(np.float32), c0=zeros, h0=zeros,
             acts=nc["acts"].astype(np.float32), od=od, ad=ad, m=m, n=n, h=h, kernel="auto", units=(256,))
    bad = nc["pattern"] == nonfinite_cases.NAN
    assert bad.sum() == 2 * m and _geometry(c, 2)["single"]
    tame = np.where(np.isfinite(c["acts"]), c["acts"], np.float32(0.0))
    for kind in ("program", "model"):
        for micro in (2, 0):
            rets, keys, traj, _ = _plan(c, kind, micro, nc["discount"])
            ref, _, ref_traj, _ = _plan(c, kind, micro, nc["discount"], acts=tame)
            assert np.all(np.isfinite(ref)) and not np.any(np.isfinite(rets[bad])) and np.all(np.isfinite(rets[~bad]))
            assert np.array_equal(_bits(rets[~bad]), _bits(ref[~bad]))
            rows = bad.reshape(-1)
            assert np.all(np.isnan(traj[:, rows])) and np.array_equal(_bits(traj[:, ~rows]), _bits(ref_traj[:, ~rows]))
            if kind == "model":
                assert np.all(np.isnan(rets[bad]))
                assert np.array_equal(keys, _want_keys(rets, 0))        # NaN sorts highest: the first diverged candidate


# ------------------------------------------------------------------------------------------
# 6. through the controller
# ------------------------------------------------------------------------------------------
CID = "hc_rnn_rs_m2_n64_h4_reset_s0"


class _PredictOnly(object):
    """What a user's own reward model looks like to the controller: nothing but ``predict``."""

    def __init__(self, model):
        self.model, self.calls = model, 0

    def predict(self, obs, act, nxt):
        self.calls += 1
        return self.model.predict(obs, act, nxt)


def _hidden(case, seed=5):
    rs = np.random.RandomState(seed)
    return LSTMStateTuple(rs.randn(case["m"], case["units"]).astype(np.float32),
                          np.tanh(rs.randn(case["m"], case["units"])).astype(np.float32))


def _controller(reward, wrap=False, **kw):
    case, seed = cases.split_id(CID)
    env, model = cases.product_rnn_model(case)
    rm = None
    if reward == "program":
        env = rpc.program_env(case["env"])
        _, model = cases.product_rnn_model(case)
    else:
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        rm = MLPRewardModel(name="rew", env=env, hidden_sizes=RM_HIDDEN, hidden_nonlinearity=RM_ACT, init_seed=0)
        rm.set_params(rmc.reward_weights(od, ad, RM_HIDDEN))
        rm.set_normalization(rmc.reward_norm(od, ad, base=cases.rnn_recipe(case)[2]))
        kw.update(reward_model=_PredictOnly(rm) if wrap else rm, use_reward_model=True, native_reward_model=True)
    ctrl = RNNMPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0),
                            n_candidates=case["n"], horizon=case["h"], **kw)
    ctrl._hidden_state = _hidden(case)
    fn = env.reward_spec.evaluate if reward == "program" else rmc.model_reward_fn(rm)
    return case, seed, env, model, rm, ctrl, fn


def _margin(returns):
    top = np.sort(returns, axis=1)
    return float(np.min((top[:, -1] - top[:, -2]) / np.maximum(1.0, np.abs(top[:, -1]))))


@pytest.mark.parametrize("reward", ["program", "model"])
def test_controller_random_shooting_like_the_oracle(reward):
    case, seed, env, model, rm, ctrl, fn = _controller(reward, rng="numpy")
    assert ctrl._fusable() and ctrl._program()
    obs, hid = cases.load_golden(CID)["obs"][0], _hidden(case)
    dyn = cases.oracle_rnn_dynamics(case)
    np.random.seed(seed)
    want, best, returns, nxt = rnn_rs_plan(dyn, fn, obs, hid, env.action_space.low, env.action_space.high, case["n"], case["h"],
                                           case.get("discount", 1.0))
    rng_next = np.random.uniform()
    print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
    assert _margin(returns) >= MARGIN
    np.random.seed(seed)
    got, info = ctrl.get_actions(obs)
    assert np.random.uniform() == rng_next
    native = model.planner_model()
    assert info == {} and (native.program_plans, native.reward_model_plans) == ((1, 0) if reward == "program" else (0, 1))
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    assert rel_err(ctrl.last_plan["best_return"], returns[np.arange(case["m"]), best]) <= RTOL
    # the controller's own state: the advance kernel's result for the chosen action - what the default fused path enqueues behind
    # its plan - and the oracle's step at the bar of the recurrent parity tests (tests/test_rnn.py)
    c1, h1 = native.advance(_dev(obs), _dev(want), _dev(hid.c), _dev(hid.h))
    assert np.array_equal(_bits(ctrl._hidden_state.c), _bits(c1.cpu().numpy()))
    assert np.array_equal(_bits(ctrl._hidden_state.h), _bits(h1.cpu().numpy()))
    np.testing.assert_allclose(ctrl._hidden_state.c, nxt.c, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(ctrl._hidden_state.h, nxt.h, rtol=1e-4, atol=2e-5)
    if reward == "model":
        # the same plan through a wrapper that exposes only `predict`: the unfused loop, the same candidate
        _, _, _, model2, _, plain, _ = _controller(reward, wrap=True, rng="numpy")
        assert plain._native_reward_model() is None and not plain._fusable()
        np.random.seed(seed)
        got2, _ = plain.get_actions(obs)
        assert plain.reward_model.calls == case["h"] and model2.planner_model().reward_model_plans == 0
        np.testing.assert_array_equal(got2, want)


@pytest.mark.parametrize("reward", ["program", "model"])
def test_controller_cem_teacher_forced_like_the_oracle(reward):
    """Every CEM iteration on its own (``cem_mode="reference"``), started from the ORACLE's mean / std of the previous one with
    the same normal draws, so that no rank tie can decide the outcome; the last iteration picks the oracle's candidate."""
    iters = 2
    case, seed, env, model, rm, ctrl, fn = _controller(reward, rng="numpy", use_cem=True, num_cem_iters=iters, cem_mode="reference")
    obs, hid = cases.load_golden(CID)["obs"][0], _hidden(case)
    m, n, h = case["m"], case["n"], case["h"]
    act_dim = env.action_space.shape[0]
    k = max(int(n * ctrl.percent_elites), 1)
    trace = []
    np.random.seed(seed)
    want, best, returns, _ = rnn_cem_plan(cases.oracle_rnn_dynamics(case), fn, obs, hid, env.action_space.low, env.action_space.high,
                                          n, h, case.get("discount", 1.0), num_cem_iters=iters, percent_elites=ctrl.percent_elites,
                                          trace=trace)
    rng_next = np.random.uniform()
    print("top-2 margin of the oracle's returns: %.3e" % _margin(returns))
    assert _margin(returns) >= MARGIN
    clip_low = np.concatenate([env.action_space.low] * h)
    clip_high = np.concatenate([env.action_space.high] * h)
    np.random.seed(seed)
    mean, std = np.zeros((m, h * act_dim)), np.ones((m, h * act_dim))
    for it in range(iters):
        _, _, mine, cand_a = ctrl._cem_iteration(obs, mean, std, k, clip_low, clip_high, 0, n, 1)
        err = rel_err(mine, trace[it]["returns"])
        print("CEM iteration %d (%s): returns %.2e against the float64 oracle" % (it, reward, err))
        assert err <= RTOL
        cem_ties.assert_flips_are_ties(mine, trace[it]["returns"], k, RTOL)
        mean, std = trace[it]["mean"], trace[it]["std"]             # teacher forcing
    assert np.random.uniform() == rng_next
    idx = np.argmax(mine, axis=1)
    assert np.array_equal(idx, best)
    np.testing.assert_array_equal(cand_a[np.arange(m), idx], want)
    native = model.planner_model()
    assert (native.program_plans if reward == "program" else native.reward_model_plans) == iters
    # and the public call, both modes: it raised before
    for mode in ("reference", "fixed"):
        _, _, _, model2, _, c2, _ = _controller(reward, rng="numpy", use_cem=True, num_cem_iters=2, cem_mode=mode)
        np.random.seed(seed)
        got, _ = c2.get_actions(obs)
        n2 = model2.planner_model()
        assert got.shape == (m, act_dim) and (n2.program_plans if reward == "program" else n2.reward_model_plans) == 2
