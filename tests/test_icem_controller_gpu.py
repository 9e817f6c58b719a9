"""The iCEM planner through the controller on the GPU: ``MPCController(use_icem=True, rng="device")`` on the small golden-case
models (one MLP, one 5-member mean ensemble).

Every iteration is judged teacher-forced: the samples bit for bit against ``icem_reference.sample_f32`` on the product's OWN state
before the iteration (the normals are injected), the refit against ``icem_reference.refit`` on the product's own samples and
returns - elites, kept rows, counts, index, best return and action bits exactly, mean and spread within
``icem_reference.refit_bounds`` -, and the last iteration's returns against the float64 oracle (the project's bar, 1e-4 relative)."""

import numpy as np
import pytest
import torch

import cases
import icem_reference as ir
from learning_to_adapt_amd import _lib
from oracle import make_reward
from oracle.planner import rollout_returns

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # returns against the float64 oracle, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
MODELS = {"mlp": dict(cases.CASES["hc_rs_m3_n64_h5"]),
          "ens5": dict(cases.CASES["c2_hc_rs_n2000_h30_e5"], n=96, h=6)}        # the 5-member mean ensemble on a small plan
STATE = ("icem_means", "icem_stds", "icem_kept", "icem_kc", "icem_work")


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _obs(which):
    case = MODELS[which]
    return cases.load_golden("%s_s%d" % (case["name"], case["seeds"][0]))["obs0"]


def _controller(which, **kw):
    case = MODELS[which]
    return case, cases.product_controller(case, rng="device", use_icem=True, **kw)


def _inject(ctrl, zs):
    it = iter(zs)

    def hook(shape, device):
        z = next(it)
        assert tuple(z.shape) == tuple(shape), "the controller asked for normals %s, the test prepared %s" % (shape, z.shape)
        return torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(device)

    ctrl._icem_normal_device = hook


def _spy(ctrl, log):
    """Record, at every rollout (between an iteration's sample and its refit), the samples, the three state copies and - after the
    launch - the returns."""
    rollout = ctrl._rollout

    def spy(observations, seq, n_it, *args, **kw):
        snap = {k: ctrl._bufs[k].cpu().numpy().copy() for k in STATE}
        snap["a_clip"] = ctrl._bufs["icem_a_clip"].cpu().numpy()[:n_it].copy()
        snap["seq"] = seq.cpu().numpy().copy()
        out = rollout(observations, seq, n_it, *args, **kw)
        snap["returns"] = out[1].cpu().numpy().copy()
        log.append(snap)
        return out

    ctrl._rollout = spy


@pytest.fixture
def _fresh_split_state():
    ctx = _lib.Context.get(0)
    yield ctx
    ctx.set_spin_limit(0)
    ctx.set_split(1)
    ctx.split_degraded = False
    ctx.launch_status_value()


# ------------------------------------------------------------------------------------------------------ teacher-forced steps
@pytest.mark.parametrize("which", ["mlp", "ens5"])
def test_three_teacher_forced_steps_with_a_reset(which):
    case, ctrl = _controller(which, icem_keep=0.5, icem_iters=3)
    ctrl.icem_trace_returns = True
    obs = _obs(which)
    n, m, h = case["n"], case["m"], case["h"]
    ad = ctrl.action_space.shape[0]
    D = h * ad
    K, Kk, pops = ir.sizes(n, ctrl.percent_elites, ctrl.icem_keep, ctrl.icem_decay, ctrl.icem_iters)
    assert (K, Kk, pops) == ctrl._icem_sizes() and Kk >= 1 and pops[0] > pops[1] > pops[2]
    iters = len(pops)
    sigma = ctrl._icem_sigma_vector()
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    rs = np.random.RandomState(3)
    zs = [rs.randn(pops[it], m, D).astype(np.float32) for _ in range(3) for it in range(iters)]
    _inject(ctrl, zs)
    log = []
    _spy(ctrl, log)
    worst = 0.0
    cur = 0
    for s in range(3):
        if s == 2 and m >= 2:
            ctrl.reset(dones=[i == 1 for i in range(m)])
        first = np.array([-1 if (s == 0 or (s == 2 and i == 1 and m >= 2)) else 1 for i in range(m)], dtype=np.int32)
        del log[:]
        action, info = ctrl.get_actions(obs)
        assert info == {} and action.shape == (m, ad) and action.dtype == np.float64 and len(log) == iters
        plan = ctrl.last_plan
        src = cur
        for it in range(iters):
            n_it = pops[it]
            dst = [b for b in range(3) if b != src and b != cur][0]
            snap = log[it]
            what = "%s step %d iteration %d" % (which, s, it)
            shift = first if it == 0 else np.zeros(m, dtype=np.int32)
            mu, sd, want_a, want_seq = ir.sample_f32(snap["icem_means"][src], snap["icem_stds"][src], snap["icem_kept"][src],
                                                     snap["icem_kc"][src], shift, zs[s * iters + it], sigma, ctrl.icem_rho, low, high,
                                                     n_it, m, h, ad, Kk, int(ctrl.icem_add_mean and it == iters - 1))
            if s == 2 and it == 0 and m >= 2:           # the reset env started afresh, its neighbours moved on
                assert np.all(mu[1] == 0) and np.any(mu[0] != 0), what
                assert ir.kept_count(snap["icem_kc"][src][0], Kk, shift[0]) >= 1, what
            assert np.array_equal(_bits(snap["a_clip"]), _bits(want_a)), "samples: " + what
            assert np.array_equal(_bits(snap["seq"]), _bits(want_seq)), "candidate tensor: " + what
            assert np.array_equal(_bits(snap["icem_means"][dst]), _bits(mu)) and np.array_equal(_bits(snap["icem_stds"][dst]), _bits(sd)), what
            ref = ir.refit(mu, sd, snap["a_clip"], snap["returns"], K, Kk, ctrl.alpha, low, high, ad)
            # the state the refit left: the next iteration's snapshot holds it; the last iteration's is what the step returned
            if it + 1 < iters:
                after = log[it + 1]
                got = dict(mean=after["icem_means"][dst], std=after["icem_stds"][dst], kept=after["icem_kept"][dst],
                           kc=after["icem_kc"][dst], work=after["icem_work"])
            else:
                got = dict(mean=plan["icem_mean"], std=plan["icem_std"], kept=plan["icem_elites"], kc=plan["icem_elite_count"],
                           work=ctrl._bufs["icem_work"].cpu().numpy())
                assert np.array_equal(_bits(got["mean"]), _bits(ctrl._bufs["icem_means"][dst].cpu().numpy())), what
            step = plan["icem_trace"][it]
            assert step["n"] == n_it and np.array_equal(_bits(step["returns"]), _bits(snap["returns"])), what
            assert np.array_equal(step["best_index"], ref["index"]) and np.array_equal(step["elites"], ref["Ke"]), what
            assert np.array_equal(step["valid"], ref["valid"]) and np.array_equal(_bits(step["best_return"]), _bits(ref["best_return"])), what
            assert np.array_equal(got["kc"], ref["kc"]), what
            B = max(float(np.max(np.abs(snap["a_clip"]))), float(np.max(np.abs(mu))), float(np.max(np.abs(sd))))
            for i in range(m):
                ke, kc = int(ref["Ke"][i]), int(ref["kc"][i])
                assert ke == K, what                    # (finite returns: every candidate is valid)
                assert np.array_equal(got["work"][i, :ke], ref["elites"][i]), "elites: " + what
                assert np.array_equal(_bits(got["kept"][i, :kc]), _bits(ref["kept"][i])), "kept rows: " + what
                mean_bound, std_bound = ir.refit_bounds(ke, B)
                r = max(float(np.max(np.abs(got["mean"][i].astype(np.float64) - ref["mean"][i]))) / mean_bound,
                        float(np.max(np.abs(got["std"][i].astype(np.float64) - ref["std"][i]))) / std_bound)
                worst = max(worst, r)
                assert r <= 1.0, "mean / std off by %.3f of the bound: %s" % (r, what)
            if it == iters - 1:
                assert np.array_equal(_bits(action.astype(np.float32)), _bits(ref["action"])), "action: " + what
                assert np.array_equal(action, ref["action"].astype(np.float64)), what
                assert np.array_equal(plan["best_index"], ref["index"]) and np.array_equal(plan["icem_valid"], ref["valid"]), what
                assert np.array_equal(_bits(plan["best_return"]), _bits(ref["best_return"])), what
                assert np.array_equal(_bits(plan["returns"]), _bits(snap["returns"])), what
                env, _, _ = cases.recipe(case)
                want = rollout_returns(cases.oracle_dynamics(case), make_reward(case["env"], env.dt), obs,
                                       snap["seq"].astype(np.float64), n_it, case.get("discount", 1.0)).reshape(m, n_it)
                assert rel_err(snap["returns"], want) < RTOL, what
            src = dst
        cur = src
        assert ctrl._bufs["icem_cur"] == cur and ctrl._bufs["icem_calls"] == (s + 1) * iters
        assert np.all(action >= low) and np.all(action <= high)
        obs = obs + 0.01 * rs.randn(*obs.shape)
    print("\n[icem] %s: worst mean / std error over its bound %.3f" % (which, worst))


# -------------------------------------------------------------------------------------------------------- monotone best return
def test_best_return_never_decreases_within_a_step():
    """``Kk >= 1`` and ``icem_decay = 1``: the best candidate of an iteration is kept row 0 of the next one and is rolled out again
    from the same observation, so a step's best returns never decrease."""
    torch.manual_seed(77)
    case, ctrl = _controller("mlp", icem_keep=0.5, icem_iters=4, icem_decay=1.0)
    ctrl.icem_trace_returns = True
    obs = _obs("mlp")
    rs = np.random.RandomState(8)
    for s in range(3):
        ctrl.get_actions(obs)
        trace = ctrl.last_plan["icem_trace"]
        best = np.stack([step["best_return"] for step in trace])
        again = np.stack([step["returns"][:, 0] for step in trace[1:]])
        print("\n[icem] step %d: best returns per iteration %s; the kept best rolled out again differs by at most %.3e"
              % (s, best.T.tolist(), float(np.max(np.abs(again.astype(np.float64) - best[:-1])))))
        assert np.all(np.isfinite(best))
        assert np.all(best[1:] >= best[:-1]), "the best return of a later iteration is lower: %s" % (best.T.tolist(),)
        obs = obs + 0.01 * rs.randn(*obs.shape)


# ---------------------------------------------------------------------------------------------------------------- status replay
def test_flagged_launch_replays_the_step_and_commits_once(_fresh_split_state):
    ctx = _fresh_split_state
    obs = _obs("mlp")

    def run(flag):
        torch.manual_seed(99)
        _, ctrl = _controller("mlp", icem_keep=0.5)
        ctrl.dynamics_model.planner_model()
        log = []
        _spy(ctrl, log)
        a0, _ = ctrl.get_actions(obs)
        if flag:
            ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
        del log[:]
        a1, _ = ctrl.get_actions(obs)
        state = {k: ctrl._bufs[k][ctrl._bufs["icem_cur"]].cpu().numpy().copy() for k in STATE[:4]}
        return a0, a1, dict(ctrl.last_plan), state, ctrl._bufs["icem_calls"], len(log)

    a0, a1, plan, state, calls, rollouts = run(False)
    assert not getattr(ctx, "split_degraded", False) and rollouts == 3 and calls == 6
    b0, b1, plan_b, state_b, calls_b, rollouts_b = run(True)
    assert ctx.split_degraded is True and rollouts_b == 6, "the flagged step was not replayed"
    assert calls_b == calls, "the counter was committed twice (or not at all)"
    assert np.array_equal(a0, b0) and np.array_equal(a1.view(np.int64), b1.view(np.int64))
    for k in state:
        assert np.array_equal(_bits(state[k]), _bits(state_b[k])), k
    for k in ("best_index", "best_return", "returns", "icem_mean", "icem_std", "icem_elites", "icem_elite_count", "icem_valid"):
        assert np.array_equal(_bits(np.asarray(plan[k], dtype=np.float32)), _bits(np.asarray(plan_b[k], dtype=np.float32))), k


# --------------------------------------------------------------------------------------------------------------- reward program
def test_reward_program_goes_through_the_same_loop():
    from test_reward_program_gpu import _controller as program_controller
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, ctrl = program_controller(cid, rng="device", use_icem=True, icem_keep=0.5)
    obs = cases.load_golden(cid)["obs0"]
    torch.manual_seed(seed)
    log = []
    _spy(ctrl, log)
    action, _ = ctrl.get_actions(obs)
    K, Kk, pops = ctrl._icem_sizes()
    assert model.planner_model().program_plans == len(pops) == len(log)
    last = log[-1]
    want = rollout_returns(cases.oracle_dynamics(case), env.reward, obs, last["seq"].astype(np.float64), pops[-1], case.get("discount", 1.0))
    assert rel_err(ctrl.last_plan["returns"], want.reshape(case["m"], pops[-1])) < RTOL
    low, high = ctrl.action_space.low.astype(np.float32), ctrl.action_space.high.astype(np.float32)
    ref = ir.refit(last["icem_means"][ctrl._bufs["icem_cur"]], last["icem_stds"][ctrl._bufs["icem_cur"]], last["a_clip"], last["returns"],
                   K, Kk, ctrl.alpha, low, high, 6)
    assert np.array_equal(ctrl.last_plan["best_index"], ref["index"]) and np.array_equal(action, ref["action"].astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------- bad arguments
def test_bad_arguments_raise():
    case = MODELS["mlp"]
    env, model = cases.product_model(case)
    with pytest.raises(ValueError, match="choose one"):
        cases.product_controller(dict(case, planner="cem"), model=model, env=env, rng="device", use_icem=True)
    with pytest.raises(ValueError, match="choose one"):
        cases.product_controller(case, model=model, env=env, rng="device", use_icem=True, use_mppi=True)
    with pytest.raises(ValueError, match="rng='device'"):
        cases.product_controller(case, model=model, env=env, rng="numpy", use_icem=True)
    for bad in (dict(icem_rho=1.0), dict(icem_iters=0), dict(icem_decay=0.5), dict(icem_keep=1.5), dict(alpha=1.0), dict(icem_sigma=-1.0)):
        with pytest.raises(ValueError):
            cases.product_controller(case, model=model, env=env, rng="device", use_icem=True, **bad)
    ctrl = cases.product_controller(case, model=model, env=env, rng="device", use_icem=True)
    ctrl._dist = lambda: (0, 2)
    with pytest.raises(_lib.L2AError, match="shard"):
        ctrl.get_actions(_obs("mlp"))
    ctrl = cases.product_controller(case, model=model, env=env, rng="device", use_icem=True)
    ctrl.rng = "numpy"
    with pytest.raises(_lib.L2AError, match="NumPy normals"):
        ctrl.get_actions(_obs("mlp"))
