"""What planning with a learned policy prior costs (``MPCController(policy_model=...)``), on BASELINE config 2 (n = 2000, h = 30,
5 x 26-512-512-20 mean), on the GrBAL default shape (ant, 5 adapted 3 x 512 sets, 5 x 500 candidates, h = 10) and on the config-1
shape (n = 500, h = 10, one 2 x 512 model), with a (256, 256) policy network.  Per shape the controllers share the recipe's weights
and take turns call by call in one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the
spread of the p50s is recorded):

    {rs, cem, mppi} x {plain, pi24, pi5pct}, and rs_python
        rs / cem / mppi  ``rng="device"`` random shooting / one-iteration device-mode CEM (``cem_mode="fixed"``) / one-iteration MPPI
        plain            without a policy (rs: ONE C call, ``l2a_controller_step``)
        pi24 / pi5pct    ``policy_candidates=24`` / ``n // 20``, ``policy_noise=0.1``
        rs_python        rs_plain with ``native_step=False``: the Python loop a plan with a policy takes too

and, per shape and n_pi, the proposal alone: HIP events around ``--steps`` calls of ``l2a_policy_propose`` (2 h - 1 launches) on
tensors that are already on the device (kind "parts").

    python tools/probe_policy_prior.py [--steps 1000] [--warmup 50] [--repeats 3] [--no-policy] [--out profiles/policy_prior.jsonl]

``--no-policy`` leaves the policy variants and the parts out: what a checkout without the feature can run (the parent commit).

The kernel's own time comes from a run under the profiler; ``--kernels SHAPE`` is the program to trace (the proposal at both n_pi)
and ``--stats CSV --shape SHAPE`` appends the kernels' rows:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_policy_prior.py --kernels SHAPE
    python tools/probe_policy_prior.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/policy_prior.jsonl]

``--closed-loop`` is a figure, not a test: on ``SyntheticEnv``'s toy system with fitted dynamics, 300 steps of an n = 2000 planner
are cloned into a policy, then an n = 200 planner runs 50 steps with and without it.  One seed is no distribution.
"""

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HIDDEN = (256, 256)
SHAPES = {"config2": dict(env="half_cheetah", mode="mean", hidden=(512, 512), E=5, n=2000, h=30, m=1, planner="rs"),
          "grbal": dict(env="ant", mode="per_block", hidden=(512, 512, 512), E=5, n=500, h=10, m=5, planner="rs"),
          "config1": dict(env="half_cheetah", mode="single", hidden=(512, 512), E=1, n=500, h=10, m=1, planner="rs")}
KERNELS = ("l2a_policy_mlp_k",)
PLANNERS = {"rs": dict(), "cem": dict(use_cem=True, cem_mode="fixed", num_cem_iters=1), "mppi": dict(use_mppi=True, mppi_iters=1)}


def _n_pis(case):
    return {"pi24": 24, "pi5pct": case["n"] // 20}


def _policy_model(case, env):
    import cases
    import policy_reference as pr
    from learning_to_adapt_amd.dynamics import MLPPolicyModel
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    pm = MLPPolicyModel(name="pol", env=env, hidden_sizes=HIDDEN, init_seed=0)
    pm.set_params(pr.policy_weights(od, ad, HIDDEN))
    pm.set_normalization(pr.policy_norm(od, ad, base=cases.recipe(case)[2][0]))
    return pm


def _controller(case, planner, **kw):
    import cases
    from learning_to_adapt_amd.policies import MPCController
    env, model = cases.product_model(case)
    return MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0), n_candidates=case["n"],
                         horizon=case["h"], rng="device", **dict(PLANNERS[planner], **kw))


def _controllers(case, with_policy):
    from learning_to_adapt_amd.envs import SyntheticEnv
    out = {}
    for planner in PLANNERS:
        out[planner + "_plain"] = _controller(case, planner)
        if with_policy:
            for tag, n_pi in _n_pis(case).items():
                out["%s_%s" % (planner, tag)] = _controller(case, planner, policy_model=_policy_model(case, SyntheticEnv(case["env"])),
                                                            policy_candidates=n_pi, policy_noise=0.1)
    out["rs_python"] = _controller(case, "rs", native_step=False)
    return out


def _proposal(case):
    """A callable per n_pi that runs one ``l2a_policy_propose`` on device tensors."""
    import torch
    import cases
    env, model = cases.product_model(case)
    native = model.planner_model()
    pm = _policy_model(case, env).planner_policy_model()
    m, n, h = case["m"], case["n"], case["h"]
    dev = native.device
    obs0 = torch.randn((m, native.obs_dim), dtype=torch.float32, device=dev)
    seq = torch.empty((h, m * n, native.act_dim), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
    mirror = torch.empty((n, m, h * native.act_dim), dtype=torch.float32, device=dev)
    sigma = torch.full((native.act_dim,), 0.1, dtype=torch.float32, device=dev)
    low, high = -torch.ones_like(sigma), torch.ones_like(sigma)
    return {tag: (lambda n_pi=n_pi, keep=(env, model): native.policy_propose(pm, obs0, m, n, n_pi, h, seq, sigma, low, high,
                                                                             mirror=mirror, seed=1))
            for tag, n_pi in _n_pis(case).items()}


def _parts(case, steps):
    import torch
    out = {}
    for name, fn in _proposal(case).items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        out["policy_propose_" + name] = round(start.elapsed_time(stop) / steps, 5)
    return out


def latency(args):
    import torch
    from learning_to_adapt_amd.utils import synthetic
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        torch.manual_seed(1)
        ctrls = _controllers(case, not args.no_policy)
        obs = synthetic.make_obs0(case["m"], ctrls["rs_plain"].env.observation_space.shape[0])
        for _ in range(args.warmup):
            for c in ctrls.values():
                c.get_actions(obs)
        torch.cuda.synchronize()
        p50 = {v: [] for v in ctrls}
        for _ in range(args.repeats):
            ts = {v: [] for v in ctrls}
            for _ in range(args.steps):
                for v, c in ctrls.items():          # the variants take turns call by call
                    t0 = time.perf_counter()
                    c.get_actions(obs)
                    ts[v].append((time.perf_counter() - t0) * 1e3)
            for v in ctrls:
                p50[v].append(float(np.percentile(ts[v], 50)))
        for v in ctrls:
            mid = float(np.median(p50[v]))
            twin = "rs_python" if v.startswith("rs_pi") else v.split("_")[0] + "_plain"
            n_pi = _n_pis(case).get(v.split("_", 1)[1])
            rec = dict(kind="latency", shape=shape, variant=v, env=case["env"], hidden=list(case["hidden"]), E=case["E"], n=case["n"],
                       m=case["m"], h=case["h"], n_pi=n_pi, policy_hidden=list(HIDDEN) if n_pi else None, steps=args.steps,
                       repeats=args.repeats, p50_ms=round(mid, 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), over_plain_ms=round(mid - float(np.median(p50[twin])), 4),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        for c in ctrls.values():
            for attr in ("_cstep", "_cemstep", "_mppistep"):
                if getattr(c, attr, None) is not None:
                    getattr(c, attr).close()
                    setattr(c, attr, None)
        del ctrls
        if not args.no_policy:
            rec = dict(kind="parts", shape=shape, n=case["n"], m=case["m"], h=case["h"], launches=2 * case["h"] - 1, n_pi=_n_pis(case),
                       policy_hidden=list(HIDDEN), steps=args.steps, launch_ms=_parts(case, args.steps), device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    return lines


def kernels(args):
    """The program to trace: the proposal at both n_pi, taking turns."""
    import torch
    torch.manual_seed(1)
    calls = _proposal(SHAPES[args.kernels])
    for _ in range(args.steps):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            if any(k in row["Name"] for k in KERNELS) or "l2a_" in row["Name"]:
                lines.append(dict(kind="kernel", shape=args.shape, name=row["Name"], calls=int(row["Calls"]),
                                  avg_us=round(float(row["AverageNs"]) / 1e3, 3), min_us=round(float(row["MinNs"]) / 1e3, 3),
                                  max_us=round(float(row["MaxNs"]) / 1e3, 3)))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    return lines


def closed_loop(args):
    """Clone an n = 2000 planner into a policy on the toy system, then plan with n = 200 with and without it."""
    import torch
    from learning_to_adapt_amd.dynamics import MLPDynamicsModel, MLPPolicyModel
    from learning_to_adapt_amd.envs import SyntheticEnv
    from learning_to_adapt_amd.policies import MPCController
    torch.manual_seed(0)
    np.random.seed(0)
    env = SyntheticEnv("half_cheetah")
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    obs = 0.3 * np.random.randn(4000, od)
    act = np.random.uniform(-1.0, 1.0, (4000, ad))
    model = MLPDynamicsModel(name="dyn", env=env, hidden_sizes=(512, 512), init_seed=0)
    model.fit(obs, act, env.toy_dynamics(obs, act), epochs=30, verbose=False)
    teacher = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=2000, horizon=10, rng="device")
    seen_o, seen_a = [], []
    o = env.reset()
    for t in range(300):
        a = np.asarray(teacher.get_action(o)[0], dtype=np.float64).reshape(-1)
        seen_o.append(np.asarray(o, dtype=np.float64).reshape(-1))
        seen_a.append(a)
        o, _, done, _ = env.step(a)
        if done or t % 50 == 49:
            o = env.reset()
    pm = MLPPolicyModel(name="pol", env=env, hidden_sizes=HIDDEN, init_seed=0)
    fit = pm.fit(np.stack(seen_o), np.stack(seen_a), epochs=60)
    lines = []
    for name, kw in (("teacher_n2000", dict(n_candidates=2000)), ("n200", dict(n_candidates=200)),
                     ("n200_policy", dict(n_candidates=200, policy_model=pm, policy_candidates=10, policy_noise=0.1))):
        ctrl = MPCController(name="policy", env=env, dynamics_model=model, horizon=10, rng="device", **kw)
        torch.manual_seed(1)
        np.random.seed(1)
        o = env.reset()
        total, won = 0.0, 0
        for _ in range(50):
            a = np.asarray(ctrl.get_action(o)[0], dtype=np.float64).reshape(-1)
            won += int(ctrl.last_plan.get("policy_candidates", 0) > int(ctrl.last_plan["best_index"][0]))
            o, r, done, _ = env.step(a)
            total += r
            if done:
                break
        rec = dict(kind="closed_loop", env="half_cheetah toy", variant=name, steps=50, reward=round(float(total), 4),
                   policy_rows_won=won, cloning_loss=round(fit["TrainLoss"], 5), seeds=1, device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-policy", action="store_true", help="the plain variants only (a checkout without the feature)")
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's proposals for a profiler")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--closed-loop", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the tree was measured)")
    args = ap.parse_args()
    lines = stats(args) if args.stats else kernels(args) if args.kernels else closed_loop(args) if args.closed_loop else latency(args)
    if args.tag:
        for rec in lines:
            rec["build"] = args.tag
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
