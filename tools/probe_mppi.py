"""Plan-step latency of the reward-weighted (MPPI) planner next to the two planners it joins, on three shapes: BASELINE config 2
(m = 1, n = 2000, h = 30, 5 x 26-512-512-20), the GrBAL default (5 adapted 3 x 512 sets, n = 500, h = 10) and the ReBAL default
(LSTM 256, 5 envs, n = 500, h = 10).  Per shape three controllers share one model - ``use_mppi`` (one iteration), the
``rng="device"`` random-shooting step, device CEM with one iteration (``cem_mode="fixed"``) - and take turns call by call in one
process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the spread of the p50s is recorded).

    python tools/probe_mppi.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/mppi.jsonl]

Kernel times come from a run of their own under the profiler; ``--kernels SHAPE`` is the program to trace (MPPI and one-iteration
CEM steps, nothing timed on the host) and ``--stats CSV --shape SHAPE`` appends the five planner kernels' rows of the profiler's
kernel statistics to the same file:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_mppi.py --kernels SHAPE
    python tools/probe_mppi.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/mppi.jsonl]
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

SHAPES = {"config2": "c2_hc_rs_n2000_h30_e5", "grbal_default": "c3b_ant_rs_n500_h10_pb5_3x512", "rebal_default": "c6_hc_rnn_rs_n500_h10_m5"}
VARIANTS = {"mppi": dict(rng="device", use_mppi=True, mppi_iters=1),
            "rs_device": dict(rng="device"),
            "cem_1iter_device": dict(rng="device", use_cem=True, num_cem_iters=1, cem_mode="fixed")}
KERNELS = ("l2a_mppi_sample_k", "l2a_mppi_update_k", "l2a_cem_sample_k", "l2a_cem_rank_k", "l2a_cem_stats_k")


def _build(shape, variants):
    """``(case, obs, {variant: controller})`` on one shared model."""
    import cases
    name = SHAPES[shape]
    case = dict(cases.CASES[name])
    gold = cases.load_golden("%s_s%d" % (name, case["seeds"][0]))
    recurrent = case["planner"].startswith("rnn")
    obs = gold["obs"][0] if recurrent else gold["obs0"]
    if recurrent:
        from learning_to_adapt_amd.policies import RNNMPCController as Controller
        env, model = cases.product_rnn_model(case)
    else:
        from learning_to_adapt_amd.policies import MPCController as Controller
        env, model = cases.product_model(case)
    ctrls = {v: Controller(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0), n_candidates=case["n"],
                           horizon=case["h"], **VARIANTS[v]) for v in variants}
    return case, obs, ctrls


def latency(args):
    import torch
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(1)
        case, obs, ctrls = _build(shape, list(VARIANTS))
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
            rec = dict(kind="latency", shape=shape, case=SHAPES[shape], variant=v, n=case["n"], m=case["m"], h=case["h"],
                       steps=args.steps, repeats=args.repeats, p50_ms=round(float(np.median(p50[v])), 4),
                       p50_ms_repeats=[round(x, 4) for x in p50[v]], spread_ms=round(max(p50[v]) - min(p50[v]), 4),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctrls
    return lines


def kernels(args):
    """The program to trace: MPPI steps and one-iteration CEM steps on one shape."""
    import torch
    torch.manual_seed(1)
    _, obs, ctrls = _build(args.kernels, ["mppi", "cem_1iter_device"])
    for _ in range(args.steps):
        for c in ctrls.values():
            c.get_actions(obs)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k + "(" in row["Name"]:
                    lines.append(dict(kind="kernel", shape=args.shape, case=SHAPES[args.shape], kernel=k, calls=int(row["Calls"]),
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
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's MPPI and CEM steps for a profiler")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the planner kernels' rows from")
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
