#!/usr/bin/env python
"""What planning with a learned reward model costs, end to end through ``MPCController.get_actions`` (parity mode, one GPU):

* native  - ``MLPRewardModel`` handed to the controller as it is: the carry chain and the matrix-core scorer
  (``l2a_plan_rs_reward_model``);
* predict - the same controller and model behind a wrapper that exposes only ``predict``: the loop such a model ran before
  (``_get_rs_action_unfused``: h host round trips, one ``dynamics_model.predict`` and one ``reward_model.predict`` each);
* program - a ``RewardProgram`` env on the same plan: the same carry chain with the closed-form scorer behind it.

plus the scoring launch alone (``l2a_score_trajectory_model`` on a trajectory in HBM, HIP events around ``--calls``
launches).  At the config-1 shape (n=500, h=10, one 2x512 model, HalfCheetah dims) and at config 2 (n=2000, h=30, E=5 mean),
with a (256, 256) reward net.  The variants of a shape take turns call by call; p50 of ``--calls`` (200) calls after warm-up;
every call ends in the read-back of the keys, so the host clock covers the GPU work.  Appends one JSON line per shape to
``--out``.

    python tools/probe_reward_model.py [--calls=200] [--out=profiles/reward_model.jsonl]
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
import reward_model_cases as rmc  # noqa: E402
import reward_program_cases as rpc  # noqa: E402
from learning_to_adapt_amd.dynamics import MLPRewardModel  # noqa: E402
from learning_to_adapt_amd.policies import MPCController  # noqa: E402

HIDDEN = (256, 256)


class PredictOnly(object):
    def __init__(self, model):
        self.model = model

    def predict(self, obs, act, nxt):
        return self.model.predict(obs, act, nxt)


def reward_model(case, env):
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=HIDDEN, init_seed=0)
    rm.set_params(rmc.reward_weights(od, ad, HIDDEN))
    rm.set_normalization(rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0]))
    return rm


def controllers(case):
    """The three controllers of a shape, one dynamics model each (same recipe weights)."""
    out, rms = {}, {}
    for name in ("native", "predict", "program"):
        env, model = cases.product_model(case)
        if name == "program":
            env.reward_spec = rpc.new_reward_program(20, 6, 0.01)
            out[name] = cases.product_controller(case, model=model, env=env)
            continue
        rms[name] = reward_model(case, env)
        given = rms[name] if name == "native" else PredictOnly(rms[name])
        out[name] = MPCController(name="policy", env=env, dynamics_model=model, reward_model=given, use_reward_model=True,
                                  discount=case.get("discount", 1.0), n_candidates=case["n"], horizon=case["h"])
    assert out["native"]._native_reward_model() is rms["native"] and not out["predict"]._fusable() and out["program"]._program()
    return out, rms


def score_alone_ms(rm, case, calls):
    """The scoring launch alone, HIP events around `calls` launches of it on a trajectory of the plan's shape."""
    m, n, h = case["m"], case["n"], case["h"]
    native = rm.planner_reward_model()
    obs0, traj, actions = rmc.inputs(1, m, n, 20, 6, h, rm.normalization)
    dev = native.device
    o, t, a = (torch.from_numpy(x).to(dev) for x in (obs0, traj, actions))
    best = torch.zeros((m,), dtype=torch.int64, device=dev)
    for _ in range(10):
        native.score_trajectory(o, t, a, m, n, h, 1.0, best_key=best)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        native.score_trajectory(o, t, a, m, n, h, 1.0, best_key=best)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls


def run(tag, case, calls, warmup=20):
    ctrls, rms = controllers(case)
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
    score = score_alone_ms(rms["native"], case, calls)
    native = ctrls["native"].dynamics_model.planner_model()
    row = dict(shape=tag, n=case["n"], h=case["h"], m=case["m"], E=case["E"], hidden=case["hidden"], reward_hidden=list(HIDDEN),
               calls=calls, p50_ms={k: round(v, 4) for k, v in p50.items()},
               p95_ms={k: round(float(np.percentile(v, 95)), 4) for k, v in times.items()},
               score_launch_ms=round(score, 4), score_share_of_native=round(score / p50["native"], 3),
               predict_over_native=round(p50["predict"] / p50["native"], 3),
               native_over_program=round(p50["native"] / p50["program"], 3),
               same_action_native_predict=bool(np.array_equal(picks["native"], picks["predict"])),
               reward_model_plans=int(native.reward_model_plans), device=native.ctx.info().get("name"))
    for c in ctrls.values():
        if getattr(c, "_cstep", None) is not None:
            c._cstep.close()
            c._cstep = None
        if getattr(c, "_ahead", None) is not None:
            c._ahead.stop()
    return row


if __name__ == "__main__":
    calls, out = 200, os.path.join(ROOT, "profiles", "reward_model.jsonl")
    for a in sys.argv[1:]:
        if a.startswith("--calls="):
            calls = int(a.split("=")[1])
        if a.startswith("--out="):
            out = a.split("=", 1)[1]
    if not torch.cuda.is_available():
        raise SystemExit("probe_reward_model.py times GPU plans: no GPU visible")
    C = cases.CASES
    for tag, case in (("config 1 (n=500, h=10, one 2x512 model)", C["c1_hc_rs_n500_h10_e1"]),
                      ("config 2 (n=2000, h=30, E=5 mean)", C["c2_hc_rs_n2000_h30_e5"])):
        row = run(tag, case, calls)
        print(json.dumps(row), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")
