"""Plan-step latency of CEM on BASELINE config 5 (m = 1, n = 4000, h = 30, E = 5, 5 iterations) through three paths: the Python
parity path (NumPy normals, ``get_cem_action``), the Python device path (``get_cem_action_device``) and the C device step
(``native_cem_step=True``: ``l2a_cem_controller_create_device`` + ``l2a_controller_step``).  Also a whole 500-candidate plan
(50 elites, device paths) - the rollout size of one rank of an 8-way config-5 plan, NOT that rank's step (the sharded step ranks
all 4000 returns for 400 elites and all-gathers them; it has no C form yet).  p50 / p99 of host wall time per step, one JSON line per path.

    python tools/probe_cem_step.py [--steps 60] [--warmup 10] [--out profiles/cem_step.jsonl]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402


def _measure(ctrl, obs, steps, warmup):
    for _ in range(warmup):
        ctrl.get_actions(obs)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        ctrl.get_actions(obs)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    name = "c5_hc_cem_n4000_h30_e5"
    obs = cases.load_golden(name + "_s0")["obs0"]
    runs = [("python_parity", 4000, dict()), ("python_device", 4000, dict(rng="device")),
            ("c_device", 4000, dict(rng="device", native_cem_step=True)),
            ("python_device_n500_plan", 500, dict(rng="device")), ("c_device_n500_plan", 500, dict(rng="device", native_cem_step=True))]
    lines = []
    for label, n, kw in runs:
        case = dict(cases.CASES[name])
        case["n"] = n
        torch.manual_seed(1)
        np.random.seed(1)
        ctrl = cases.product_controller(case, **kw)
        ts = _measure(ctrl, obs, args.steps, args.warmup)
        if kw.get("native_cem_step"):
            assert ctrl._cemstep is not None, "the C controller did not serve the steps"
        rec = dict(path=label, n=n, m=1, h=case["h"], E=case["E"], iters=case["num_cem_iters"], steps=args.steps,
                   p50_ms=round(float(np.percentile(ts, 50)), 3), p99_ms=round(float(np.percentile(ts, 99)), 3),
                   mean_ms=round(float(np.mean(ts)), 3), device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del ctrl
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
