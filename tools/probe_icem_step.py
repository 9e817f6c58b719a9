"""Plan-step latency of the iCEM step as one C call (``MPCController(native_icem_step=True)``) next to the Python loop
``get_icem_action``, on two shapes: BASELINE config 2 (m = 1, n = 2000, h = 30, 5 x 26-512-512-20) and the GrBAL default (5 adapted
3 x 512 sets, n = 500, h = 10), ``icem_iters=3`` and the planner's other defaults.  Per shape the controllers share one model and
take turns call by call in one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the
spread of the p50s is recorded).  The yardstick is ``icem_python``, the unchanged loop, measured in the same run.  ``icem_c`` copies
the state and the last returns table back after every step, as the Python loop does; ``icem_c_lean``
(``icem_fetch_returns = False``) leaves the tables on the device.  The C controllers' own stage times (``l2a_controller_stats``:
sample / launch / wait / decode / call, of the last timed step) go into the same file, and a ``verdict`` line per shape says
whether ``icem_c`` is slower than the loop by more than the spread of the loop's own repeats.

    python tools/probe_icem_step.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/icem_step.jsonl]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"config2": ("c2_hc_rs_n2000_h30_e5", {}), "grbal_default": ("c3b_ant_rs_n500_h10_pb5_3x512", {})}
ICEM = dict(rng="device", use_icem=True, icem_iters=3)
VARIANTS = {"icem_c": dict(ICEM, native_icem_step=True), "icem_c_lean": dict(ICEM, native_icem_step=True), "icem_python": dict(ICEM)}


def _build(shape):
    """``(case, obs, {variant: controller})`` on one shared model."""
    import cases
    from learning_to_adapt_amd.policies import MPCController
    name, over = SHAPES[shape]
    case = dict(cases.CASES[name], **over)
    env, model = cases.product_model(case)
    obs = cases.load_golden("%s_s%d" % (name, case["seeds"][0]))["obs0"]
    if len(obs) != case["m"]:
        obs = obs[0] + 0.01 * np.random.RandomState(3).randn(case["m"], obs.shape[1])
    ctrls = {v: MPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0), n_candidates=case["n"],
                              horizon=case["h"], **kw) for v, kw in VARIANTS.items()}
    ctrls["icem_c_lean"].icem_fetch_returns = False
    return case, obs, ctrls


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the code was measured)")
    args = ap.parse_args()
    lines = []
    for shape in args.shapes.split(","):
        torch.manual_seed(1)
        case, obs, ctrls = _build(shape)
        for _ in range(args.warmup):
            for c in ctrls.values():
                c.get_actions(obs)
        torch.cuda.synchronize()
        for v, c in ctrls.items():
            if (c._icemstep is None) != (v == "icem_python"):
                raise SystemExit("%s on %s did not plan on its side" % (v, shape))
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
        recs = {}
        for v, c in ctrls.items():
            K, Kk, pops = c._icem_sizes()
            rec = dict(kind="latency", shape=shape, case=SHAPES[shape][0], variant=v, n=case["n"], m=case["m"], h=case["h"],
                       icem_iters=c.icem_iters, pops=pops, K=K, Kk=Kk, steps=args.steps, repeats=args.repeats,
                       p50_ms=round(float(np.median(p50[v])), 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), device=torch.cuda.get_device_name(0))
            st = c._icemstep
            if st is not None:
                s = st.stats()
                rec["stage_us"] = {k: round(x, 2) for k, x in s["stage_us"].items()}
                rec["relaunches"] = s["relaunches"]
            recs[v] = rec
        loop = recs["icem_python"]
        diff = round(recs["icem_c"]["p50_ms"] - loop["p50_ms"], 4)
        recs["verdict"] = dict(kind="verdict", shape=shape, yardstick="icem_python", c_minus_python_ms=diff,
                               python_spread_ms=loop["spread_ms"], c_slower_by_more_than_the_spread=bool(diff > loop["spread_ms"]),
                               sharded="unmeasured")
        for rec in recs.values():
            if args.tag:
                rec["build"] = args.tag
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        for c in ctrls.values():
            if c._icemstep is not None:
                c._icemstep.close()
                c._icemstep = None
        del ctrls
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
