"""Plan-step latency of particle planning (``MPCController(ensemble_planning="particles")``) next to the mean-mode step it stands
beside, on BASELINE config 2 (n = 2000, h = 30, 5 x 26-512-512-20) and on the GrBAL default shape (ant, 3 x 512, n = 500, h = 10)
with an E = 5 mean ensemble, each for one env and for five (a particle plan rolls every env in a launch of its own).  Per shape
four planners share the recipe's weights and take turns call by call in one process after a warm-up; p50 of ``--steps`` calls
each, ``--repeats`` times (the spread of the p50s is recorded):

    mean        the ``rng="device"`` random-shooting step of the mean ensemble - equal FLOPs, the yardstick (one C call,
                ``l2a_controller_step``)
    mean_python the same step with ``native_step=False``: the Python loop a particle plan takes too (draw, launch, read back)
    per_block   a raw ``l2a_plan_rs`` of m E blocks on a per-block model holding the E sets once per env, on inputs expanded by
                hand once, keys read back: the E-fold rollout alone - no draw, no expansion, no scorer, one launch for all envs
    particles   the particle step: draw, expand, m per-block launches, score, keys read back

    python tools/probe_particles.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/particles.jsonl]

Kernel times come from a run of their own under the profiler; ``--kernels SHAPE`` is the program to trace (particle steps and
one-iteration device-CEM steps of the mean ensemble, nothing timed on the host) and ``--stats CSV --shape SHAPE`` appends the two
particle kernels' rows and CEM's three per-iteration launches' rows of the profiler's kernel statistics to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_particles.py --kernels SHAPE
    python tools/probe_particles.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/particles.jsonl]
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

CONFIG2 = dict(env="half_cheetah", mode="mean", hidden=(512, 512), E=5, n=2000, h=30, planner="rs")
GRBAL_E5 = dict(env="ant", mode="mean", hidden=(512, 512, 512), E=5, n=500, h=10, planner="rs")
SHAPES = {"config2": dict(CONFIG2, m=1), "config2_m5": dict(CONFIG2, m=5),
          "grbal_e5": dict(GRBAL_E5, m=1), "grbal_e5_m5": dict(GRBAL_E5, m=5)}
KERNELS = ("l2a_particle_expand_k", "l2a_particle_score_k", "l2a_cem_sample_k", "l2a_cem_rank_k", "l2a_cem_stats_k")
RISK = 1.0


def _controllers(case, variants):
    import cases
    env, model = cases.product_model(case)
    return env, {name: cases.product_controller(case, model=model, env=env, **kw) for name, kw in variants.items()}


def _per_block_step(case, obs):
    """The raw per-block plan as a callable: every env's E members as m E blocks of one launch, inputs expanded once."""
    import torch
    import cases
    from learning_to_adapt_amd.dynamics.native_model import NativeModel
    env, sets, norms = cases.recipe(case)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    m, E, n, h = case["m"], case["E"], case["n"], case["h"]
    pb = NativeModel(od, ad, case["hidden"], "relu", None, m * E, "per_block")
    for b in range(m * E):
        pb.set_weights(b, sets[b % E])
        pb.set_norm(b, norms[b % E])
    dev = pb.device
    obs_x = torch.as_tensor(np.repeat(obs, E, axis=0), dtype=torch.float32, device=dev).contiguous()
    low, high = float(env.action_space.low[0]), float(env.action_space.high[0])
    act = torch.empty((h, m, 1, n, ad), dtype=torch.float32, device=dev).uniform_(low, high)
    act_x = act.expand(h, m, E, n, ad).contiguous().view(h, m * E * n, ad)
    best = torch.empty((m * E,), dtype=torch.int64, device=dev)

    def step():
        pb.plan_rs(obs_x, act_x, m * E, n, h, case.get("discount", 1.0), env.reward_spec, best_key=best)
        return best.cpu()
    return step


def latency(args):
    import torch
    from learning_to_adapt_amd.utils import synthetic
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        torch.manual_seed(1)
        env, ctrls = _controllers(case, {"mean": dict(rng="device"), "mean_python": dict(rng="device", native_step=False),
                                         "particles": dict(rng="device", ensemble_planning="particles", risk_coef=RISK)})
        obs = synthetic.make_obs0(case["m"], env.observation_space.shape[0])
        steps = {"mean": lambda: ctrls["mean"].get_actions(obs), "mean_python": lambda: ctrls["mean_python"].get_actions(obs),
                 "per_block": _per_block_step(case, obs),
                 "particles": lambda: ctrls["particles"].get_actions(obs)}
        for _ in range(args.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        p50 = {v: [] for v in steps}
        for _ in range(args.repeats):
            ts = {v: [] for v in steps}
            for _ in range(args.steps):
                for v, fn in steps.items():         # the variants take turns call by call
                    t0 = time.perf_counter()
                    fn()
                    ts[v].append((time.perf_counter() - t0) * 1e3)
            for v in steps:
                p50[v].append(float(np.percentile(ts[v], 50)))
        base = float(np.median(p50["mean"]))
        for v in steps:
            mid = float(np.median(p50[v]))
            rec = dict(kind="latency", shape=shape, variant=v, env=case["env"], hidden=list(case["hidden"]), E=case["E"], n=case["n"],
                       m=case["m"], h=case["h"], risk_coef=RISK if v == "particles" else None, steps=args.steps,
                       repeats=args.repeats, p50_ms=round(mid, 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), ratio_to_mean=round(mid / base, 4),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctrls, steps
    return lines


def kernels(args):
    """The program to trace: particle steps and one-iteration CEM steps of the mean ensemble on one shape."""
    import torch
    from learning_to_adapt_amd.utils import synthetic
    torch.manual_seed(1)
    case = SHAPES[args.kernels]
    env, ctrls = _controllers(case, {"particles": dict(rng="device", ensemble_planning="particles", risk_coef=RISK)})
    cem = _controllers(dict(case, planner="cem", num_cem_iters=1), {"cem": dict(rng="device", cem_mode="fixed")})[1]
    obs = synthetic.make_obs0(case["m"], env.observation_space.shape[0])
    for _ in range(args.steps):
        ctrls["particles"].get_actions(obs)
        cem["cem"].get_actions(obs)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k + "(" in row["Name"]:
                    lines.append(dict(kind="kernel", shape=args.shape, kernel=k, calls=int(row["Calls"]),
                                      avg_us=round(float(row["AverageNs"]) / 1e3, 3), min_us=round(float(row["MinNs"]) / 1e3, 3),
                                      max_us=round(float(row["MaxNs"]) / 1e3, 3)))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's particle and CEM steps for a profiler")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the kernels was measured)")
    args = ap.parse_args()
    lines = stats(args) if args.stats else kernels(args) if args.kernels else latency(args)
    if args.tag:
        for rec in lines:
            rec["build"] = args.tag
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
