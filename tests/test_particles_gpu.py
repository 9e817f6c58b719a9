"""Particle plans on the GPU (``csrc/l2a_particles.hip``, ``l2a_plan_rs_particles`` and siblings, ``MPCController(
ensemble_planning="particles")``) against ``tests/particle_reference.py``.

Bounds (derived, none measured and then set): the scorer alone is bit-equal to ``score_f32`` (every NaN counting as the same NaN:
``_canon``); the member returns are bit-equal to
``l2a_plan_rs`` on a per-block model of the same weight sets; against the float64 oracle every member return lies within the
project's bar, 1e-4 of max |R|, and every score within ``(1 + lambda)`` times that (the mean is an average and std is 1-Lipschitz
in the sup norm of the member errors); a chosen index is a witnessed tie when its oracle score is within twice that bound of the
oracle's maximum.  Every test prints the maxima it measured (``-s``)."""

import ctypes

import numpy as np
import pytest

import cases
import particle_reference as pr
import reward_model_cases as rmc
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs.synthetic_env import SyntheticEnv
from learning_to_adapt_amd.utils import synthetic

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
OD, AD = 20, 6
WIDTHS = ((128, 128), (256, 256), (32, 32))        # smallest MFMA width, micro tiles, VALU
MEMBERS = (2, 3, 5)
SHAPES = [(n, h, m) for n in (16, 50, 500) for h in (1, 7) for m in (1, 3)]
BAR = 1e-4
KEY_SENTINEL = -0x0123456789ABCDEF
GUARD = 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _canon(a):
    """The bits of an fp32 array with every NaN replaced by one NaN: which NaN an operation returns (sign, payload) is the one thing
    IEEE 754 leaves to the implementation - x86 and gfx950 differ on inf - inf and sqrt(NaN) - and nothing downstream reads it (the
    keys pack every NaN alike)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.int32(0x7fc00000), a.view(np.int32))


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class _Out:
    """A device output between two runs of guard words, pre-filled with a sentinel (NaN for floats)."""

    def __init__(self, shape, keys=False):
        import torch
        self.keys = keys
        self.size = int(np.prod(shape))
        self.fill = KEY_SENTINEL if keys else NAN
        self.guard = KEY_SENTINEL + 1 if keys else -12345.0
        self.flat = torch.full((self.size + 2 * GUARD,), self.guard, dtype=torch.int64 if keys else torch.float32, device="cuda:0")
        self.view = self.flat[GUARD:GUARD + self.size].view(*shape)
        self.view.fill_(self.fill)

    def host(self, what):
        h = self.flat.cpu().numpy()
        assert np.all(h[:GUARD] == self.guard) and np.all(h[GUARD + self.size:] == self.guard), "guard words overwritten: " + what
        return h[GUARD:GUARD + self.size].reshape(tuple(self.view.shape)).copy()

    def untouched(self, what):
        h = self.host(what)
        return bool(np.all(h == self.fill)) if self.keys else bool(np.isnan(h).all())


_MODELS = {}


def native_model(hidden, E, mode="mean"):
    """A ``NativeModel`` holding the recipe's E members (shared among the tests: nothing writes to it)."""
    from learning_to_adapt_amd.dynamics.native_model import NativeModel
    key = (tuple(hidden), E, mode)
    if key not in _MODELS:
        env = SyntheticEnv("half_cheetah")
        sets, norms = synthetic.make_members(env, hidden, E)
        model = NativeModel(OD, AD, hidden, "relu", None, E, mode)
        for e in range(E):
            model.set_weights(e, sets[e])
            model.set_norm(e, norms[e])
        _MODELS[key] = (env, sets, norms, model)
    return _MODELS[key]


def plan_inputs(seed, n, h, m):
    """Observations float64 ``[m, O]`` and candidate actions float64 ``[h, m n, A]`` as parity-mode random shooting draws them."""
    from oracle import planner
    env = SyntheticEnv("half_cheetah")
    np.random.seed(seed)
    obs = synthetic.make_obs0(m, OD)
    return obs, planner.sample_rs_actions(env.action_space.low, env.action_space.high, n, m, h)


def run_plan(model, obs, actions, n, h, m, lam, reward, cand_offset=0, discount=1.0, expect_rc=_lib.L2A_OK, E=None,
             out_n=None):
    """One particle plan through the C entry that ``reward`` selects; host copies of the four outputs (guards checked).  ``out_n``:
    candidates the outputs are allocated for (a refused call with an absurd ``n``)."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel, _ptr, _stream_ptr
    from learning_to_adapt_amd.envs import RewardProgram
    E = model.n_sets if E is None else E
    on = n if out_n is None else out_n
    out = dict(score=_Out((m, on)), spread=_Out((m, on)), members=_Out((m, E, on)), keys=_Out((m,), keys=True))
    obs_d, act_d = _up(np.asarray(obs, dtype=np.float32)), _up(np.asarray(actions, dtype=np.float32))
    tail = (ctypes.c_float(lam), cand_offset, _ptr(out["score"].view), _ptr(out["spread"].view), _ptr(out["members"].view),
            _ptr(out["keys"].view), _stream_ptr(torch.device("cuda:0")))
    head = (_ptr(obs_d), _ptr(act_d), m, n, h, float(discount))
    lib = model.lib
    if isinstance(reward, NativeRewardModel):
        rc = lib.l2a_plan_rs_particles_reward_model(model.handle, reward.handle, *(head + tail))
    elif isinstance(reward, RewardProgram):
        rc = lib.l2a_plan_rs_particles_program(model.handle, *(head + (ctypes.byref(reward),) + tail))
    else:
        rc = lib.l2a_plan_rs_particles(model.handle, *(head + (ctypes.byref(reward),) + tail))
    torch.cuda.synchronize()
    what = "plan n=%d h=%d m=%d lambda=%g offset=%d" % (n, h, m, lam, cand_offset)
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, lib.l2a_last_error(model.ctx.handle).decode())
    if expect_rc != _lib.L2A_OK:
        assert all(o.untouched(k + " " + what) for k, o in out.items()), "output written by a refused call: " + what
        return rc
    assert model.ctx.launch_status_value() == 0, what
    return {k: o.host(k + " " + what) for k, o in out.items()}


def run_score(ctx, R, lam, cand_offset=0, expect_rc=_lib.L2A_OK, which=("score", "spread", "keys")):
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    m, E, n = R.shape
    R_d = _up(R)
    out = dict(score=_Out((m, n)), spread=_Out((m, n)), keys=_Out((m,), keys=True))
    ptr = {k: (_ptr(o.view) if k in which else None) for k, o in out.items()}
    rc = ctx.lib.l2a_particle_score(ctx.handle, _ptr(R_d), m, E, n, ctypes.c_float(lam), cand_offset, ptr["score"], ptr["spread"],
                                    ptr["keys"], _stream_ptr(torch.device("cuda:0")))
    torch.cuda.synchronize()
    what = "score m=%d E=%d n=%d lambda=%r offset=%d" % (m, E, n, lam, cand_offset)
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    assert np.array_equal(_bits(R_d.cpu().numpy()), _bits(R)), "input changed: " + what
    for k, o in out.items():
        if k not in which or expect_rc != _lib.L2A_OK:
            assert o.untouched(k + " " + what), "%s written though it was not asked for: %s" % (k, what)
    return rc if expect_rc != _lib.L2A_OK else {k: o.host(k + " " + what) for k, o in out.items()}


def check_score(ctx, R, lam, cand_offset=0):
    got = run_score(ctx, R, lam, cand_offset)
    score, std = pr.score_f32(R, lam)
    what = "m=%d E=%d n=%d lambda=%g" % (R.shape + (lam,))
    assert np.array_equal(_canon(got["score"]), _canon(score)), "score: " + what
    assert np.array_equal(_canon(got["spread"]), _canon(std)), "spread: " + what
    assert np.array_equal(got["keys"].view(np.uint64), pr.keys(score, cand_offset)), "keys: " + what
    return got


# ------------------------------------------------------------------------------------------------------------ 1. scorer alone
@pytest.mark.parametrize("E", [1, 2, 3, 5, 8])
def test_scorer_is_bit_equal_to_the_fp32_restatement(E):
    """Random tables over n = 1 .. 1025 (one lane, one wave, ragged workgroups, five workgroups per env), m = 1 and 3, five values
    of lambda, offsets; then the same launch with one output at a time."""
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(50 + E)
    c = 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025):
        for m in (1, 3):
            lam = (0.0, 1.0, 0.37, 4.0, -1.5)[c % 5]
            off = (0, 25, 0x7fffffff - n)[c % 3]
            c += 1
            R = pr.random_table(rs, m, E, n, scale=(3.0, 1e-3, 1e4)[c % 3], offset=(0.0, 50.0, -2e4)[c % 3])
            check_score(ctx, R, lam, off)
    R = pr.random_table(rs, 3, E, 300)
    whole = run_score(ctx, R, 1.0, 7)
    for which in ("score", "spread", "keys"):
        one = run_score(ctx, R, 1.0, 7, which=(which,))
        assert np.array_equal(one[which].view(np.int32), whole[which].view(np.int32)), which        # (the same device: NaNs included)


def test_scorer_crafted_rows():
    ctx = _lib.Context.get(0)
    rs = np.random.RandomState(3)
    n = 300
    # exact ties across candidates: the best score four times, in two workgroups - the lowest index wins
    R = pr.random_table(rs, 2, 3, n)
    for j in (290, 17, 256, 40):
        R[:, :, j] = np.array([9.0, 7.0, 8.0], dtype=np.float32)[None]
    for lam in (0.0, 1.0):
        got = check_score(ctx, R, lam, cand_offset=11)
        assert [_lib.key_decode(int(k))[1] for k in got["keys"]] == [11 + 17, 11 + 17]
    # identical members: the spread is exactly 0 and the score the common value, whatever lambda
    # (E a power of two: the sum E x and its division by E are exact.  Any other E rounds E x, the mean may miss x by an ulp and
    #  the spread is then a few ulps of |x|, not 0 - in the kernel as in the restatement: E = 5 is held to the bits alone)
    for E in (2, 4):
        R = np.repeat(pr.random_table(rs, 2, 1, n), E, axis=1)
        got = check_score(ctx, R, 4.0)
        assert np.all(got["spread"] == 0.0) and np.array_equal(_bits(got["score"]), _bits(R[:, 0]))
    R = np.repeat(pr.random_table(rs, 2, 1, n), 5, axis=1)
    got = check_score(ctx, R, 4.0)
    assert np.all(got["spread"] <= pr.score_bound(R, 0.0))
    # a NaN in one member: that candidate's score is NaN and it is the arg-max (the first of two)
    R = pr.random_table(rs, 2, 3, n)
    R[0, 1, 200] = NAN
    R[0, 2, 77] = NAN
    got = check_score(ctx, R, 1.0)
    assert np.isnan(got["score"][0, 77]) and np.isnan(got["score"][0, 200]) and _lib.key_decode(int(got["keys"][0]))[1] == 77
    assert np.isfinite(got["score"][1]).all()
    # +inf and -inf members
    R = pr.random_table(rs, 1, 3, n)
    R[0, 0, 5] = INF                    # mean +inf, std NaN
    R[0, 1, 6] = -INF                   # mean -inf, std NaN
    R[0, 0, 7], R[0, 2, 7] = INF, -INF  # mean NaN
    R[0, :, 8] = INF                    # every member +inf: mean +inf, std NaN (inf - inf)
    got = check_score(ctx, R, 1.0)
    assert np.isnan(got["score"][0, [5, 6, 7, 8]]).all() and np.isnan(got["spread"][0, [5, 6, 7, 8]]).all()
    # lambda = 0: the score is the mean itself, so a +inf mean stays +inf and wins over every finite score
    got = check_score(ctx, R, 0.0)
    assert got["score"][0, 5] == INF and got["score"][0, 8] == INF and got["score"][0, 6] == -INF and np.isnan(got["score"][0, 7])
    R[0, :, 7] = 0.0
    got = check_score(ctx, R, 0.0, cand_offset=1000)
    assert _lib.key_decode(int(got["keys"][0])) == (INF, 1005)
    # E = 1: the member itself, spread 0;  n = 1
    R = pr.random_table(rs, 3, 1, 70)
    got = check_score(ctx, R, 2.0)
    assert np.array_equal(_bits(got["score"]), _bits(R[:, 0])) and np.all(got["spread"] == 0.0)
    check_score(ctx, pr.random_table(rs, 3, 4, 1), 1.0, cand_offset=9)


def test_scorer_refusals_write_nothing():
    ctx = _lib.Context.get(0)
    R = pr.random_table(np.random.RandomState(4), 2, 3, 40)
    for lam in (NAN, INF, -INF):
        assert run_score(ctx, R, lam, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_score(ctx, R, 1.0, cand_offset=-1, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_score(ctx, R, 1.0, cand_offset=0x7fffffff - 39, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_score(ctx, R, 1.0, which=(), expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL


def test_scorer_is_deterministic():
    ctx = _lib.Context.get(0)
    R = pr.random_table(np.random.RandomState(6), 3, 5, 1025)
    runs = [run_score(ctx, R, 1.0) for _ in range(3)]
    for g in runs[1:]:
        assert all(np.array_equal(g[k].view(np.int32), runs[0][k].view(np.int32)) for k in g)


# ------------------------------------------------------------------------------------------------- 2. expansion and routing
def per_block_member_returns(pb, obs, actions, n, h, m, E, plan):
    """``[m, E, n]``: per env one per-block request of E blocks on ``pb`` (the same E sets), inputs expanded with torch."""
    import torch
    obs_d = _up(np.asarray(obs, dtype=np.float32))
    act_d = _up(np.asarray(actions, dtype=np.float32)).view(h, m, n, AD)
    rows = []
    for i in range(m):
        obs_x = obs_d[i:i + 1].expand(E, OD).contiguous()
        act_x = act_d[:, i:i + 1].expand(h, E, n, AD).contiguous().view(h, E * n, AD)
        ret = torch.full((E, n), NAN, dtype=torch.float32, device="cuda:0")
        plan(pb, obs_x, act_x, ret)
        rows.append(ret)
    torch.cuda.synchronize()
    return torch.stack(rows).cpu().numpy()


@pytest.mark.parametrize("E", MEMBERS)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_member_returns_equal_per_block_plans_bit_for_bit(hidden, E):
    env, _, _, mean_model = native_model(hidden, E)
    pb = native_model(hidden, E, "per_block")[3]
    spec = env.reward_spec
    for c, (n, h, m) in enumerate(SHAPES):
        obs, actions = plan_inputs(100 + c, n, h, m)
        lam = (0.0, 1.0, 4.0)[c % 3]
        got = run_plan(mean_model, obs, actions, n, h, m, lam, spec, cand_offset=(0, 13)[c % 2], discount=(1.0, 0.95)[c % 2])
        want = per_block_member_returns(pb, obs, actions, n, h, m, E,
                                        lambda mdl, o, a, r: mdl.plan_rs(o, a, E, n, h, (1.0, 0.95)[c % 2], spec, returns_out=r))
        what = "hidden=%s E=%d n=%d h=%d m=%d" % (hidden, E, n, h, m)
        assert np.array_equal(_bits(got["members"]), _bits(want)), "member returns: " + what
        score, std = pr.score_f32(got["members"], lam)
        assert np.array_equal(_bits(got["score"]), _bits(score)) and np.array_equal(_bits(got["spread"]), _bits(std)), what
        assert np.array_equal(got["keys"].view(np.uint64), pr.keys(score, (0, 13)[c % 2])), "keys: " + what


@pytest.mark.parametrize("kind", ["program", "reward_model"])
def test_program_and_reward_model_entries_equal_per_block_plans(kind):
    from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
    hidden, E, n, h = (256, 256), 3, 50, 7
    env, _, _, mean_model = native_model(hidden, E)
    pb = native_model(hidden, E, "per_block")[3]
    if kind == "program":
        reward = rpc.new_reward_program(OD, AD, env.dt)
        plan = lambda mdl, o, a, r: mdl.plan_rs_program(o, a, E, n, h, 0.95, reward, returns_out=r)     # noqa: E731
    else:
        reward = NativeRewardModel(OD, AD, (64,), "relu")
        reward.set_weights(rmc.reward_weights(OD, AD, (64,)))
        reward.set_norm(rmc.reward_norm(OD, AD))
        plan = lambda mdl, o, a, r: mdl.plan_rs_reward_model(o, a, E, n, h, 0.95, reward, returns_out=r)    # noqa: E731
    for m in (1, 3):
        obs, actions = plan_inputs(200 + m, n, h, m)
        got = run_plan(mean_model, obs, actions, n, h, m, 1.0, reward, cand_offset=5, discount=0.95)
        want = per_block_member_returns(pb, obs, actions, n, h, m, E, plan)
        assert np.array_equal(_bits(got["members"]), _bits(want)), "%s m=%d" % (kind, m)
        score, std = pr.score_f32(got["members"], 1.0)
        assert np.array_equal(_bits(got["score"]), _bits(score)) and np.array_equal(_bits(got["spread"]), _bits(std))
        assert np.array_equal(got["keys"].view(np.uint64), pr.keys(score, 5))


# ------------------------------------------------------------------------------------------------------ 3. against the oracle
_PRODUCT = {}


def particle_controller(env, sets, norms, hidden, E, n, h, planner="rs", **kw):
    """A particle-planning ``MPCController`` on the package's model of the recipe (one model per width and ensemble size)."""
    case = dict(env="half_cheetah", mode="mean", hidden=hidden, E=E, n=n, h=h, planner=planner, num_cem_iters=1)
    key = (tuple(hidden), E)
    if key not in _PRODUCT:
        _PRODUCT[key] = cases.product_model(case)
    penv, model = _PRODUCT[key]
    return cases.product_controller(case, model=model, env=penv, ensemble_planning="particles", **kw)


@pytest.mark.parametrize("E", MEMBERS)
@pytest.mark.parametrize("hidden", WIDTHS)
def test_plans_against_the_float64_oracle(hidden, E):
    """Member returns within 1e-4 of max |R|, scores within (1 + lambda) times that, the controller's index a witnessed tie of
    the oracle's scores, its action that candidate's float64 first action bit for bit (parity-mode random shooting)."""
    env, sets, norms, mean_model = native_model(hidden, E)
    worst_r = worst_s = 0.0
    for c, (n, h, m) in enumerate(SHAPES):
        lam = (1.0, 0.0, 4.0)[c % 3]
        obs, actions = plan_inputs(300 + c, n, h, m)
        R64 = pr.member_returns64(env, sets, norms, obs, actions, n)
        s64 = pr.score64(R64, lam)[0]
        scale = float(np.max(np.abs(R64)))
        got = run_plan(mean_model, obs, actions, n, h, m, lam, env.reward_spec)
        what = "hidden=%s E=%d n=%d h=%d m=%d lambda=%g" % (hidden, E, n, h, m, lam)
        err_r = float(np.max(np.abs(got["members"].astype(np.float64) - R64))) / scale
        err_s = float(np.max(np.abs(got["score"].astype(np.float64) - s64))) / scale
        worst_r, worst_s = max(worst_r, err_r), max(worst_s, err_s / (1 + lam))
        print("[particles] %s: member returns %.2e, scores %.2e of max |R|" % (what, err_r, err_s))
        assert err_r <= BAR, "member returns off by %.3e of max |R|: %s" % (err_r, what)
        assert err_s <= (1 + lam) * BAR, "scores off by %.3e of max |R|: %s" % (err_s, what)
        ctrl = particle_controller(env, sets, norms, hidden, E, n, h, risk_coef=lam, draw_ahead=False)
        np.random.seed(300 + c)
        act, _ = ctrl.get_actions(obs)
        idx = ctrl.last_plan["best_index"]
        first = actions[0].reshape(m, n, AD)
        for i in range(m):
            assert s64[i, idx[i]] >= np.max(s64[i]) - 2 * (1 + lam) * BAR * scale, "env %d chose %d, no tie of the oracle's: %s" % (i, idx[i], what)
            assert np.array_equal(act[i].view(np.int64), first[i, idx[i]].view(np.int64)), "action of env %d: %s" % (i, what)
        diag = ctrl.particle_diagnostics()
        assert np.array_equal(diag["index"], idx)
        assert np.array_equal(_bits(diag["member_returns"]), _bits(got["members"][np.arange(m), :, idx])), what
        assert np.array_equal(_bits(diag["std"]), _bits(got["spread"][np.arange(m), idx])), what
    print("[particles] hidden=%s E=%d: worst member return %.2e, worst score / (1 + lambda) %.2e of max |R|" % (hidden, E, worst_r, worst_s))


# ----------------------------------------------------------------------------------------------------- 4. risk changes the plan
@pytest.mark.parametrize("E,seed,want", pr.RISK_RECIPES)
def test_risk_changes_the_plan(E, seed, want):
    hidden = (128, 128)
    env, sets, norms, _ = native_model(hidden, E)
    obs = synthetic.make_obs0(1, OD)
    chosen = []
    for lam in pr.RISK_LAMBDAS:
        ctrl = particle_controller(env, sets, norms, hidden, E, 50, 7, risk_coef=lam, draw_ahead=False)
        np.random.seed(seed)
        ctrl.get_actions(obs)
        chosen.append(int(ctrl.last_plan["best_index"][0]))
    assert tuple(chosen) == tuple(want), "E=%d seed=%d: chose %s, the oracle %s" % (E, seed, chosen, want)
    assert chosen[0] != chosen[1]


# ------------------------------------------------------------------------------------------------------------------ 5. sharding
def test_two_shards_combine_to_the_unsharded_plan():
    hidden, E, n, h, m = (128, 128), 3, 50, 7, 3
    env, _, _, mean_model = native_model(hidden, E)
    obs, actions = plan_inputs(500, n, h, m)
    whole = run_plan(mean_model, obs, actions, n, h, m, 1.0, env.reward_spec)
    a4 = actions.reshape(h, m, n, AD)
    parts = []
    for lo, hi in ((0, 25), (25, 50)):
        local = np.ascontiguousarray(a4[:, :, lo:hi]).reshape(h, m * (hi - lo), AD)
        parts.append(run_plan(mean_model, obs, local, hi - lo, h, m, 1.0, env.reward_spec, cand_offset=lo))
    keys = np.maximum(parts[0]["keys"].view(np.uint64), parts[1]["keys"].view(np.uint64))
    assert np.array_equal(keys, whole["keys"].view(np.uint64))
    for k in ("score", "spread"):
        assert np.array_equal(_bits(np.concatenate([p[k] for p in parts], axis=1)), _bits(whole[k])), k
    assert np.array_equal(_bits(np.concatenate([p["members"] for p in parts], axis=2)), _bits(whole["members"]))


# ------------------------------------------------------------------------------------------- 6. CEM and MPPI consume the score
@pytest.mark.parametrize("planner", ["cem", "mppi"])
def test_cem_and_mppi_plan_on_the_score(planner):
    import torch
    hidden, E, n, h, m, lam = (128, 128), 3, 50, 7, 3, 1.0
    env, sets, norms, mean_model = native_model(hidden, E)
    obs = synthetic.make_obs0(m, OD)
    torch.manual_seed(7)
    if planner == "cem":
        ctrl = particle_controller(env, sets, norms, hidden, E, n, h, planner="cem", rng="device", cem_mode="fixed", risk_coef=lam)
    else:
        ctrl = particle_controller(env, sets, norms, hidden, E, n, h, rng="device", use_mppi=True, risk_coef=lam)
    native = ctrl.dynamics_model.planner_model()
    plans0 = getattr(native, "particle_plans", 0)
    act, _ = ctrl.get_actions(obs)
    assert np.isfinite(act).all()
    assert native.particle_plans == plans0 + 1
    diag = ctrl.particle_diagnostics(tables=True)
    members = diag["member_returns_table"]
    assert members.shape == (m, E, n) and np.isfinite(members).all()
    table = ctrl.last_plan["returns"] if planner == "mppi" else diag["score_table"]     # what the planner's update consumed
    again = run_score(native.ctx, members, lam)
    assert np.array_equal(_bits(table), _bits(again["score"])), "the planner's returns are not the particle score"
    score, std = pr.score_f32(members, lam)
    assert np.array_equal(_bits(table), _bits(score)) and np.array_equal(_bits(diag["spread_table"]), _bits(std))
    idx = np.array([pr.argmax_nan_first(row) for row in score])
    assert np.array_equal(diag["index"], idx)
    assert np.array_equal(_bits(diag["member_returns"]), _bits(members[np.arange(m), :, idx]))
    assert np.array_equal(_bits(diag["std"]), _bits(std[np.arange(m), idx]))
    assert np.array_equal(_bits(diag["score"]), _bits(score[np.arange(m), idx]))
    # ... and the planner's own pick stands on that table: MPPI's result row, CEM's `l2a_cem_pick` behind its refit
    assert np.array_equal(ctrl.last_plan["best_index"], idx)
    assert np.array_equal(_bits(np.asarray(ctrl.last_plan["best_return"], dtype=np.float32)), _bits(score[np.arange(m), idx]))


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_plan_refusals_write_nothing():
    from learning_to_adapt_amd.dynamics.native_model import NativeModel
    env = SyntheticEnv("half_cheetah")
    obs, actions = plan_inputs(700, 16, 2, 1)
    single = native_model((32, 32), 1, "single")[3]
    per_block = native_model((32, 32), 2, "per_block")[3]
    mean_of_one = native_model((32, 32), 1, "mean")[3]
    for model in (single, per_block, mean_of_one):
        assert run_plan(model, obs, actions, 16, 2, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_EINVAL, E=2) == _lib.L2A_EINVAL
        assert "mean ensemble" in model.lib.l2a_last_error(model.ctx.handle).decode()
    good = native_model((32, 32), 2)[3]
    for lam in (NAN, INF):
        assert run_plan(good, obs, actions, 16, 2, 1, lam, env.reward_spec, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_plan(good, obs, actions, 16, 2, 1, 1.0, env.reward_spec, cand_offset=-1, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_plan(good, obs, actions, 0, 2, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_EINVAL, out_n=16) == _lib.L2A_EINVAL
    # m * E * n beyond the row limit: refused on the counts alone (the pointers are never read)
    assert run_plan(good, obs, actions, 1 << 29, 2, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_EINVAL, out_n=16) == _lib.L2A_EINVAL
    # an action tensor beyond one expansion launch (h m n A / 4 = 1.5 * 2^32 words): refused on the counts, before the model's
    # buffer would be grown to hold it
    assert run_plan(good, obs, actions, 1 << 28, 64, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_EINVAL, out_n=16) == _lib.L2A_EINVAL
    assert "expansion launch" in good.lib.l2a_last_error(good.ctx.handle).decode()
    unset = NativeModel(OD, AD, (32, 32), "relu", None, 2, "mean")
    assert run_plan(unset, obs, actions, 16, 2, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_ESTATE) == _lib.L2A_ESTATE
    run_plan(good, obs, actions, 16, 2, 1, 1.0, env.reward_spec)        # and the good model still plans
