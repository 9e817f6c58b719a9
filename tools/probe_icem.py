"""The iCEM planner next to device CEM (``cem_mode="fixed"``, ``rng="device"``), on BASELINE config 2 (m = 1, n = 2000, h = 30,
5 x 26-512-512-20) and the GrBAL default (5 adapted 3 x 512 sets, n = 500, h = 10).

Step time: two controllers share one model - ``use_icem`` with ``icem_iters = 3`` and device CEM with ``num_cem_iters = 3`` - and take
turns call by call in one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the spread of
the p50s is recorded).

    python tools/probe_icem.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/icem.jsonl]

Kernel times come from a run of their own under the profiler; ``--kernels SHAPE`` is the program to trace (iCEM and CEM steps taking
turns, nothing timed on the host) and ``--stats CSV --shape SHAPE`` appends the planner kernels' rows of the profiler's kernel
statistics, and the launches per iteration they add up to, to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_icem.py --kernels SHAPE --steps 200
    python tools/probe_icem.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/icem.jsonl]

``--noise`` turns every mode to the planner's two noises instead: AR(1) (``icem_noise="ar1"``) next to power-law noise
(``icem_noise="powerlaw"``, ``icem_beta = 2``; ``--quality`` adds ``icem_beta = 1``), the step time through the Python loop and through
the C step (``native_icem_step=True``; a shape the C step declines is recorded as planned by the Python loop), the traced kernels
``l2a_icem_sample_k`` and ``l2a_icem_sample_noise_k``; the lines go to ``profiles/icem_noise.jsonl``.

Plan quality (``--quality``): the toy linear system and the fitted 5-member ensemble of ``tools/demo_closed_loop.py mb_mpc``, 50
closed-loop steps per episode, iCEM against device CEM at (as nearly as the integers allow) equal rollouts per step.
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

SHAPES = {"config2": "c2_hc_rs_n2000_h30_e5", "grbal_default": "c3b_ant_rs_n500_h10_pb5_3x512"}
VARIANTS = {"icem_3iter": dict(rng="device", use_icem=True, icem_iters=3),
            "cem_3iter_device": dict(rng="device", use_cem=True, num_cem_iters=3, cem_mode="fixed")}
NOISE_VARIANTS = {"ar1_python": dict(rng="device", use_icem=True, icem_iters=3),
                  "powerlaw_python": dict(rng="device", use_icem=True, icem_iters=3, icem_noise="powerlaw", icem_beta=2.0),
                  "ar1_c_step": dict(rng="device", use_icem=True, icem_iters=3, native_icem_step=True),
                  "powerlaw_c_step": dict(rng="device", use_icem=True, icem_iters=3, native_icem_step=True, icem_noise="powerlaw",
                                          icem_beta=2.0)}
NOISE_KERNELS = ("l2a_icem_sample_k", "l2a_icem_sample_noise_k")
ICEM_KERNELS = ("l2a_icem_sample_k", "l2a_icem_rank_k", "l2a_icem_stats_k")
CEM_KERNELS = ("l2a_cem_sample_k", "l2a_cem_rank_k", "l2a_cem_stats_k", "l2a_cem_refit_sample_k", "l2a_cem_pick_k")


def _build(shape, variants, table=None):
    """``(case, obs, {variant: controller})`` on one shared model."""
    table = VARIANTS if table is None else table
    import cases
    from learning_to_adapt_amd.policies import MPCController
    name = SHAPES[shape]
    case = dict(cases.CASES[name])
    gold = cases.load_golden("%s_s%d" % (name, case["seeds"][0]))
    env, model = cases.product_model(case)
    ctrls = {v: MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0), n_candidates=case["n"],
                              horizon=case["h"], **table[v]) for v in variants}
    return case, gold["obs0"], ctrls


def latency(args):
    import torch
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(1)
        table = NOISE_VARIANTS if args.noise else VARIANTS
        case, obs, ctrls = _build(shape, [v for v in table if not args.variants or v in args.variants.split(",")], table)
        for _ in range(args.warmup):
            for c in ctrls.values():
                c.get_actions(obs)
        torch.cuda.synchronize()
        p50 = {v: [] for v in ctrls}
        for _ in range(args.repeats):
            ts = {v: [] for v in ctrls}
            for _ in range(args.steps):
                for v, c in ctrls.items():          # the planners take turns call by call
                    t0 = time.perf_counter()
                    c.get_actions(obs)
                    ts[v].append((time.perf_counter() - t0) * 1e3)
            for v in ctrls:
                p50[v].append(float(np.percentile(ts[v], 50)))
        for v, c in ctrls.items():
            rollouts = sum(c._icem_sizes()[2]) if c.use_icem else c.num_cem_iters * case["n"]
            rec = dict(kind="latency", shape=shape, case=SHAPES[shape], variant=v, n=case["n"], m=case["m"], h=case["h"],
                       rollouts_per_step=int(rollouts), steps=args.steps, repeats=args.repeats,
                       p50_ms=round(float(np.median(p50[v])), 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), device=torch.cuda.get_device_name(0))
            if args.noise:
                rec.update(icem_noise=getattr(c, "icem_noise", "ar1"), icem_beta=getattr(c, "icem_beta", None), planned_by="c step" if c._icem_side == "c" else "python loop")
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctrls
    return lines


def kernels(args):
    """The program to trace: iCEM steps and three-iteration CEM steps on one shape."""
    import torch
    torch.manual_seed(1)
    if args.noise:
        _, obs, ctrls = _build(args.kernels, ["ar1_python", "powerlaw_python"], NOISE_VARIANTS)
    else:
        _, obs, ctrls = _build(args.kernels, list(VARIANTS))
    for _ in range(args.steps):
        for c in ctrls.values():
            c.get_actions(obs)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines, avg = [], {}
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in (NOISE_KERNELS if args.noise else ICEM_KERNELS + CEM_KERNELS):
                if k + "(" in row["Name"] or k + "<" in row["Name"]:
                    avg[k] = float(row["AverageNs"]) / 1e3
                    lines.append(dict(kind="kernel", shape=args.shape, case=SHAPES[args.shape], kernel=k, calls=int(row["Calls"]),
                                      avg_us=round(avg[k], 3), min_us=round(float(row["MinNs"]) / 1e3, 3),
                                      max_us=round(float(row["MaxNs"]) / 1e3, 3)))
    if all(k in avg for k in ICEM_KERNELS):
        lines.append(dict(kind="per_iteration", shape=args.shape, planner="icem", kernels=list(ICEM_KERNELS),
                          sum_avg_us=round(sum(avg[k] for k in ICEM_KERNELS), 3)))
    if all(k in avg for k in CEM_KERNELS[:3]):
        lines.append(dict(kind="per_iteration", shape=args.shape, planner="cem", kernels=list(CEM_KERNELS[:3]),
                          sum_avg_us=round(sum(avg[k] for k in CEM_KERNELS[:3]), 3)))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    return lines


def quality(args):
    """50 closed-loop steps on the toy system with the fitted ensemble of ``demo_closed_loop.py mb_mpc``; per planner the collected
    reward of ``--episodes`` episodes (the same start states for both)."""
    import torch
    from demo_closed_loop import random_paths
    from learning_to_adapt_amd.dynamics import MLPDynamicsModel
    from learning_to_adapt_amd.envs import SyntheticEnv
    from learning_to_adapt_amd.policies import MPCController
    np.random.seed(0)
    torch.manual_seed(0)
    env = SyntheticEnv("half_cheetah")
    od, ad = 20, 6
    obs, act = random_paths(env, 40, 50, 1)
    model = MLPDynamicsModel(name="dyn_model", env=env, hidden_sizes=(512, 512), learning_rate=1e-3, batch_size=256, ensemble_size=5,
                             init_seed=0)
    model.fit(obs[:, :-1].reshape(-1, od), act.reshape(-1, ad), obs[:, 1:].reshape(-1, od), epochs=args.epochs)
    n, h, iters = 2000, 10, 3
    icem = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=n, horizon=h, rng="device", use_icem=True,
                         icem_iters=iters)
    rollouts = sum(icem._icem_sizes()[2])
    cem = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=rollouts // iters, horizon=h, rng="device",
                        use_cem=True, num_cem_iters=iters, cem_mode="fixed")
    lines = []
    planners = (("icem_3iter", icem, rollouts), ("cem_3iter_device", cem, (rollouts // iters) * iters))
    if args.noise:          # the same rollouts per step: the noise does not change the populations
        planners = (("icem_3iter_ar1", icem, rollouts),) + tuple(
            ("icem_3iter_powerlaw_beta%g" % beta,
             MPCController(name="policy", env=env, dynamics_model=model, n_candidates=n, horizon=h, rng="device", use_icem=True,
                           icem_iters=iters, icem_noise="powerlaw", icem_beta=beta), rollouts) for beta in (1.0, 2.0))
    for name, policy, per_step in planners:
        totals = []
        for ep in range(args.episodes):
            np.random.seed(100 + ep)
            torch.manual_seed(100 + ep)
            o = env.reset()
            policy.reset(dones=[True])
            total = 0.0
            for _ in range(args.quality_steps):
                a = policy.get_action(o)[0][0]
                o, rew, _, _ = env.step(a)
                total += rew
            totals.append(float(total))
        rec = dict(kind="quality", system="demo_closed_loop mb_mpc (toy linear system, fitted 5 x 512-512 ensemble)", variant=name,
                   rollouts_per_step=int(per_step), horizon=h, closed_loop_steps=args.quality_steps, episodes=args.episodes,
                   returns=[round(t, 3) for t in totals], mean_return=round(float(np.mean(totals)), 3))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's iCEM and CEM steps for a profiler")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the planner kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--noise", action="store_true", help="AR(1) next to power-law noise, in every mode (profiles/icem_noise.jsonl)")
    ap.add_argument("--variants", default="", help="step time: only these variants (comma-separated; default: all of the mode's)")
    ap.add_argument("--quality", action="store_true", help="closed-loop plan quality on the toy system")
    ap.add_argument("--quality-steps", type=int, default=50)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the kernels was measured)")
    args = ap.parse_args()
    lines = stats(args) if args.stats else kernels(args) if args.kernels else quality(args) if args.quality else latency(args)
    if args.tag:
        for rec in lines:
            rec["build"] = args.tag
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
