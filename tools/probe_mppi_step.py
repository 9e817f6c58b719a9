"""Plan-step latency of the MPPI step as one C call (``MPCController(native_mppi_step=True)``) next to the Python loop
``get_mppi_action`` and to one-iteration device CEM through ITS C step (``native_cem_step=True``), on three shapes: BASELINE config 2
(m = 1, n = 2000, h = 30, 5 x 26-512-512-20), the GrBAL default (5 adapted 3 x 512 sets, n = 500, h = 10) and ``run_mb_mpc.py``'s
default (one 2 x 512 model, n = 2000, h = 20, the 10 envs of the sampler at once).  Per shape the controllers share one model and
take turns call by call in one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the
spread of the p50s is recorded).  ``mppi_c`` copies the mean and the last returns table back after every step, as the Python loop
does; ``mppi_c_lean`` (``mppi_fetch_returns = False``) leaves the table on the device.  The C controllers' own stage times
(``l2a_controller_stats``: sample / launch / wait / decode / call, of the last timed step) go into the same file.

    python tools/probe_mppi_step.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/mppi_step.jsonl]
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

SHAPES = {"config2": ("c2_hc_rs_n2000_h30_e5", {}), "grbal_default": ("c3b_ant_rs_n500_h10_pb5_3x512", {}),
          "mb_mpc_default": ("c1_hc_rs_n500_h10_e1", dict(n=2000, h=20, m=10))}
VARIANTS = {"mppi_c": dict(rng="device", use_mppi=True, mppi_iters=1, native_mppi_step=True),
            "mppi_c_lean": dict(rng="device", use_mppi=True, mppi_iters=1, native_mppi_step=True),
            "mppi_python": dict(rng="device", use_mppi=True, mppi_iters=1),
            "cem_1iter_c": dict(rng="device", use_cem=True, num_cem_iters=1, cem_mode="fixed", native_cem_step=True)}


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
    ctrls["mppi_c_lean"].mppi_fetch_returns = False
    return case, obs, ctrls


def _handle(v, c):
    return c._mppistep if v.startswith("mppi_c") else c._cemstep if v == "cem_1iter_c" else None


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
            if v != "mppi_python" and _handle(v, c) is None:
                raise SystemExit("%s on %s did not take its C step" % (v, shape))
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
        for v, c in ctrls.items():
            rec = dict(kind="latency", shape=shape, case=SHAPES[shape][0], variant=v, n=case["n"], m=case["m"], h=case["h"],
                       steps=args.steps, repeats=args.repeats, p50_ms=round(float(np.median(p50[v])), 4),
                       p50_ms_repeats=[round(x, 4) for x in p50[v]], spread_ms=round(max(p50[v]) - min(p50[v]), 4),
                       device=torch.cuda.get_device_name(0))
            st = _handle(v, c)
            if st is not None:
                s = st.stats()
                rec["stage_us"] = {k: round(x, 2) for k, x in s["stage_us"].items()}
                rec["relaunches"] = s["relaunches"]
            if args.tag:
                rec["build"] = args.tag
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        for v, c in ctrls.items():
            st = _handle(v, c)
            if st is not None:
                st.close()
        del ctrls
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
