"""Plan-step latency of CEM on BASELINE config 5 (m = 1, n = 4000, h = 30, E = 5, 5 iterations) through three paths: the Python
parity path (NumPy normals, ``get_cem_action``), the Python device path (``get_cem_action_device``) and the C device step
(``native_cem_step=True``: ``l2a_cem_controller_create_device`` + ``l2a_controller_step``).  Also a whole 500-candidate plan
(50 elites, device paths) - the rollout size of one rank of an 8-way config-5 plan, NOT that rank's step (the sharded step ranks
all 4000 returns for 400 elites and gathers them: ``--sharded``).  p50 / p99 of host wall time per step, one JSON line per path.

    python tools/probe_cem_step.py [--steps 60] [--warmup 10] [--out profiles/cem_step.jsonl]

``--sharded``: the sharded C step (``l2a_cem_controller_create_sharded_device``) on ONE GPU, four configurations in one run:
 (a) config 5 through the unsharded C step (``c_device``: the controller; ``c_step_unsharded``: ``NativeCemStep.step`` alone);
 (b) the sharded controller at world = 1 with a callback that returns at once: (b) - (a) = 5 x (pack + unpack);
 (c) rank 0 of 8 through the sharded step, with a stand-in callback that copies this rank's words into the other ranks' slots
     (no second GPU here: the elite statistics are then meaningless, their cost is not - as tools/probe_c5_shard.py's stand-in);
 (d) the Python path of the same shard (``get_cem_action_device`` told it is rank 0 of 8, the all-gather a local copy).
Nothing here measures a collective between GPUs.

    python tools/probe_cem_step.py --sharded [--out profiles/cem_step_sharded.jsonl]
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


WORLD = 8


def _record(label, case, n, ts, steps, **extra):
    rec = dict(path=label, n=n, m=1, h=case["h"], E=case["E"], iters=case["num_cem_iters"], steps=steps,
               p50_ms=round(float(np.percentile(ts, 50)), 3), p99_ms=round(float(np.percentile(ts, 99)), 3),
               mean_ms=round(float(np.mean(ts)), 3), min_ms=round(float(np.min(ts)), 3), device=torch.cuda.get_device_name(0))
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


def _measure_step(st, obs, stream, steps, warmup):
    for _ in range(warmup):
        st.step(obs, stream)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        st.step(obs, stream)
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def sharded(args):
    from learning_to_adapt_amd.policies import MPCController
    from learning_to_adapt_amd.policies.native_cem_step import NativeCemStep
    name = "c5_hc_cem_n4000_h30_e5"
    case = dict(cases.CASES[name])
    obs = cases.load_golden(name + "_s0")["obs0"]
    env, model = cases.product_model(case)
    native = model.planner_model()
    n, m, h, iters = case["n"], case["m"], case["h"], case["num_cem_iters"]
    stream = torch.cuda.current_stream(native.device).cuda_stream
    lines = []

    # (a) the unsharded C step, through the controller (the figure of profiles/cem_step.jsonl) and alone
    torch.manual_seed(1)
    ctrl = cases.product_controller(case, model=model, env=env, rng="device", native_cem_step=True)
    ts = _measure(ctrl, obs, args.steps, args.warmup)
    assert ctrl._cemstep is not None, "the C controller did not serve the steps"
    lines.append(_record("c_device", case, n, ts, args.steps, config="a"))
    num_elites, alpha, reward = max(int(n * ctrl.percent_elites), 1), ctrl.alpha, ctrl._reward_spec
    del ctrl

    def build(shard):
        return NativeCemStep(native, m, n, h, env.action_space.low, env.action_space.high, 1.0, reward, iters, num_elites, alpha, True, 1,
                             shard=shard)

    st = build(None)
    lines.append(_record("c_step_unsharded", case, n, _measure_step(st, obs, stream, args.steps, args.warmup), args.steps, config="a"))
    st.close()

    # (b) world = 1, a callback that returns at once: the cost of 5 x (pack + unpack) and of the callback's two copies
    st = build((0, 1, lambda payload: None))
    lines.append(_record("c_step_sharded_world1_noop_reduce", case, n, _measure_step(st, obs, stream, args.steps, args.warmup),
                         args.steps, config="b"))
    st.close()

    # (c) rank 0 of 8, the other ranks' words a copy of this rank's
    lo, hi = MPCController._shard_range(n, 0, WORLD)
    assert n % WORLD == 0

    def standin(payload):
        t = payload[:m * n].view(m, WORLD, n // WORLD)
        t.copy_(t[:, 0:1, :].clone().expand_as(t))

    st = build((0, WORLD, standin))
    lines.append(_record("c_step_rank0_of_8_standin_reduce", case, n, _measure_step(st, obs, stream, args.steps, args.warmup), args.steps,
                         config="c", n_local=hi - lo, note="no collective between GPUs: a local stand-in fills the other ranks' words"))
    assert st.stats()["relaunches"] == 0
    st.close()

    # (d) the Python path of the same shard
    class OneRankOfEight(MPCController):
        def _dist(self):
            return 0, WORLD

        @staticmethod
        def _all_gather(mine, world):
            return [mine for _ in range(world)]

        def _agree(self, flag, world):
            return bool(flag)

    torch.manual_seed(1)
    ctrl = OneRankOfEight(name="policy", env=env, dynamics_model=model, discount=1.0, n_candidates=n, horizon=h, use_cem=True,
                          num_cem_iters=iters, rng="device")
    lines.append(_record("python_device_rank0_of_8_standin_gather", case, n, _measure(ctrl, obs, args.steps, args.warmup), args.steps,
                         config="d", n_local=hi - lo, note="no collective between GPUs: the all-gather is a local copy"))
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--sharded", action="store_true", help="the sharded C step's four configurations (see above)")
    args = ap.parse_args()
    if args.sharded:
        return sharded(args)
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
