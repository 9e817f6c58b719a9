#!/usr/bin/env python
"""What planning with a reward program costs, end to end through ``MPCController.get_actions`` (parity mode, one GPU):

* custom env - a reward none of the reference's envs has, declared as a ``RewardProgram`` (``l2a_plan_rs_program``: h carry
  launches + one scoring launch) against the same env WITHOUT a declared program, i.e. the loop such an env ran before
  reward programs existed (``_get_rs_action_unfused``: h host round trips through ``dynamics_model.predict`` with the
  float64 NumPy reward between them);
* cost of generality - the HalfCheetah reward as a program against the fused ``RewardSpec`` path on the same plan.

At the config-1 shape (n=500, h=10, one 2x512 model, HalfCheetah dims) and at config 2 (n=2000, h=30, E=5 mean).  The
variants of a shape take turns call by call; p50 of ``--calls`` (200) calls after warm-up; every call ends in the read-back
of the keys, so the host clock covers the GPU work.  Appends one JSON line per shape to ``--out``.

    python tools/probe_reward_program.py [--calls=200] [--out=profiles/reward_program.jsonl]
"""
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
import reward_program_cases as rpc  # noqa: E402
from learning_to_adapt_amd.envs import RewardProgram, SyntheticEnv  # noqa: E402


def controllers(case):
    """The four controllers of a shape, one model each (same recipe weights)."""
    out = {}
    od, ad = 20, 6
    custom = rpc.new_reward_program(od, ad, 0.01)
    for name in ("program", "unfused", "hc_program", "hc_spec"):
        env, model = cases.product_model(case)
        if name == "program":
            env.reward_spec = custom                            # SyntheticEnv.reward evaluates reward_spec
        elif name == "unfused":
            env.reward_spec = None                              # nothing declared: the controller keeps the reference's loop
            env.reward = custom.evaluate
        elif name == "hc_program":
            env.reward_spec = RewardProgram.from_spec(SyntheticEnv("half_cheetah").reward_spec, od, ad)
        out[name] = cases.product_controller(case, model=model, env=env)
    assert out["program"]._program() and not out["unfused"]._fusable() and out["hc_program"]._program()
    assert not out["hc_spec"]._program() and out["hc_spec"]._fusable()
    return out


def run(tag, case, calls, warmup=20):
    ctrls = controllers(case)
    obs = np.random.RandomState(1).randn(case["m"], 20)
    picks = {}
    for name, c in ctrls.items():
        np.random.seed(0)
        picks[name] = c.get_actions(obs)[0]
        for _ in range(warmup):
            c.get_actions(obs)
    torch.cuda.synchronize()
    times = {name: [] for name in ctrls}
    for _ in range(calls):
        for name, c in ctrls.items():                           # the variants take turns: drift hits all of them alike
            t0 = time.perf_counter()
            c.get_actions(obs)
            times[name].append(1e3 * (time.perf_counter() - t0))
    p50 = {k: float(np.percentile(v, 50)) for k, v in times.items()}
    row = dict(shape=tag, n=case["n"], h=case["h"], m=case["m"], E=case["E"], hidden=case["hidden"], calls=calls,
               p50_ms={k: round(v, 4) for k, v in p50.items()},
               p95_ms={k: round(float(np.percentile(v, 95)), 4) for k, v in times.items()},
               unfused_over_program=round(p50["unfused"] / p50["program"], 3),
               hc_program_over_hc_spec=round(p50["hc_program"] / p50["hc_spec"], 3),
               same_action_program_unfused=bool(np.array_equal(picks["program"], picks["unfused"])),
               same_action_hc_program_hc_spec=bool(np.array_equal(picks["hc_program"], picks["hc_spec"])),
               program_plans=int(ctrls["program"].dynamics_model.planner_model().program_plans),
               device=ctrls["program"].dynamics_model.planner_model().ctx.info().get("name"))
    for c in ctrls.values():
        if getattr(c, "_cstep", None) is not None:
            c._cstep.close()
            c._cstep = None
        if getattr(c, "_ahead", None) is not None:
            c._ahead.stop()
    return row


if __name__ == "__main__":
    calls, out = 200, os.path.join(ROOT, "profiles", "reward_program.jsonl")
    for a in sys.argv[1:]:
        if a.startswith("--calls="):
            calls = int(a.split("=")[1])
        if a.startswith("--out="):
            out = a.split("=", 1)[1]
    if not torch.cuda.is_available():
        raise SystemExit("probe_reward_program.py times GPU plans: no GPU visible")
    C = cases.CASES
    for tag, case in (("config 1 (n=500, h=10, one 2x512 model)", C["c1_hc_rs_n500_h10_e1"]),
                      ("config 2 (n=2000, h=30, E=5 mean)", C["c2_hc_rs_n2000_h30_e5"])):
        row = run(tag, case, calls)
        print(json.dumps(row), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")
