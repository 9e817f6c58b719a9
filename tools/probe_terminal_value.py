"""What planning with a learned terminal value costs (``MPCController(value_model=...)``), on BASELINE config 2 (n = 2000,
h = 30, 5 x 26-512-512-20 mean), on the GrBAL default shape (ant, 5 adapted 3 x 512 sets, 5 x 500 candidates, h = 10) and on the config-1 shape (n = 500,
h = 10, one 2 x 512 model), with a (256, 256) value network.  Per shape eight controllers share the recipe's weights and take
turns call by call in one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the spread
of the p50s is recorded):

    {rs, cem} x {fused, program} x {plain, value}, and rs_fused_python
        rs / cem        ``rng="device"`` random shooting / one-iteration device-mode CEM
        fused / program the env's closed-form formula in the rollout kernel / a ``RewardProgram`` env (trajectory rollout + scorer)
        plain / value   without / with the value model (``l2a_plan_rs_value``, ``l2a_plan_rs_program_value``)
        rs_fused_python rs_fused_plain with ``native_step=False``: the Python loop a plan with a value model takes too (the plain
                        fused RS step is one C call, ``l2a_controller_step``)

and, per shape, the three launches the fused difference is made of, HIP events around ``--steps`` calls of each on candidates that
are already on the device (kind "parts"): ``l2a_plan_rs`` (keys), ``l2a_plan_rs_chunk`` with ``state_out`` (what a state-writing
request costs over the plain one: micro tiles decline it) and ``l2a_plan_rs_value`` (the chunk plus the new launch).

    python tools/probe_terminal_value.py [--steps 1000] [--warmup 50] [--repeats 3] [--no-value] [--out profiles/terminal_value.jsonl]

``--no-value`` leaves the four value variants and the parts out: what a checkout without the feature can run (the parent commit).

The new launch's own time comes from a run under the profiler, next to ``l2a_reward_model_predict`` of a reward model of the same
widths on the same rows; ``--kernels SHAPE`` is the program to trace and ``--stats CSV --shape SHAPE`` appends both kernels' rows:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_terminal_value.py --kernels SHAPE
    python tools/probe_terminal_value.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/terminal_value.jsonl]
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
KERNELS = ("l2a_value_mlp_k", "l2a_score_mlp_k")


def _value_model(case, env):
    import cases
    import value_model_cases as vmc
    from learning_to_adapt_amd.dynamics import MLPValueModel
    od = env.observation_space.shape[0]
    vm = MLPValueModel(name="val", env=env, hidden_sizes=HIDDEN, init_seed=0)
    vm.set_params(vmc.value_weights(od, HIDDEN))
    vm.set_normalization(vmc.value_norm(od, base=cases.recipe(case)[2][0]))
    return vm


def _controllers(case, with_value):
    import cases
    import reward_program_cases as rpc
    out = {}
    for planner in ("rs", "cem"):
        for reward in ("fused", "program"):
            for value in (("plain", "value") if with_value else ("plain",)):
                env, model = cases.product_model(case)
                if reward == "program":
                    env = rpc.program_env(case["env"])
                kw = dict(rng="device")
                if planner == "cem":
                    kw.update(cem_mode="fixed")
                if value == "value":
                    kw.update(value_model=_value_model(case, env), terminal_value_coef=1.0)
                out["%s_%s_%s" % (planner, reward, value)] = cases.product_controller(
                    dict(case, planner=planner, num_cem_iters=1), model=model, env=env, **kw)
    # the plain fused RS step is ONE C call (l2a_controller_step); a plan with a value model takes the Python loop: its plain twin
    env, model = cases.product_model(case)
    out["rs_fused_python"] = cases.product_controller(case, model=model, env=env, rng="device", native_step=False)
    return out


def _parts(case, steps):
    """The launches of the fused difference, HIP events around `steps` calls of each."""
    import ctypes
    import torch
    import cases
    from learning_to_adapt_amd.envs.reward_spec import reward_spec_for_env
    env, model = cases.product_model(case)
    native = model.planner_model()
    vm = _value_model(case, env).planner_value_model()
    m, n, h, disc = case["m"], case["n"], case["h"], case.get("discount", 1.0)
    dev = native.device
    spec = reward_spec_for_env(env)
    obs0 = torch.randn((m, native.obs_dim), dtype=torch.float32, device=dev)
    a = torch.empty((h, m * n, native.act_dim), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
    rets = torch.empty((m, n), dtype=torch.float32, device=dev)
    state = torch.empty((m * n, native.obs_dim), dtype=torch.float32, device=dev)
    best = torch.empty((m,), dtype=torch.int64, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())            # noqa: E731
    null = ctypes.c_void_p()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def chunk():
        native.ctx.check(native.lib.l2a_plan_rs_chunk(native.handle, ptr(obs0), 0, ptr(a), m, n, h, 0, float(disc), ctypes.byref(spec), 0,
                                                      null, ptr(rets), ptr(state), null, stream), "l2a_plan_rs_chunk")

    calls = {"plan_rs": lambda: native.plan_rs(obs0, a, m, n, h, disc, spec, best_key=best),
             "plan_rs_chunk_state_out": chunk,
             "plan_rs_value": lambda: native.plan_rs_value(obs0, a, m, n, h, disc, spec, vm, best_key=best),
             "value_terminal": lambda: vm.terminal(state, rets, m, n, h, disc, best_key=best)}
    out = {}
    for name, fn in calls.items():
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        out[name] = round(start.elapsed_time(stop) / steps, 5)
    return out


def latency(args):
    import torch
    from learning_to_adapt_amd.utils import synthetic
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        torch.manual_seed(1)
        ctrls = _controllers(case, not args.no_value)
        obs = synthetic.make_obs0(case["m"], ctrls["rs_fused_plain"].env.observation_space.shape[0])
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
            plain = float(np.median(p50["rs_fused_python" if v == "rs_fused_value" else v.rsplit("_", 1)[0] + "_plain"]))
            rec = dict(kind="latency", shape=shape, variant=v, env=case["env"], hidden=list(case["hidden"]), E=case["E"], n=case["n"],
                       m=case["m"], h=case["h"], value_hidden=list(HIDDEN) if v.endswith("_value") else None, steps=args.steps,
                       repeats=args.repeats, p50_ms=round(mid, 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), over_plain_ms=round(mid - plain, 4),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        for c in ctrls.values():
            for attr in ("_cstep", "_cemstep"):
                if getattr(c, attr, None) is not None:
                    getattr(c, attr).close()
                    setattr(c, attr, None)
        del ctrls
        if not args.no_value:
            rec = dict(kind="parts", shape=shape, n=case["n"], m=case["m"], h=case["h"], value_hidden=list(HIDDEN), steps=args.steps,
                       launch_ms=_parts(case, args.steps), device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    return lines


def kernels(args):
    """The program to trace: the fold, and ``l2a_reward_model_predict`` of a reward model of the same widths, on the same rows."""
    import torch
    import cases
    import reward_model_cases as rmc
    from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
    torch.manual_seed(1)
    case = SHAPES[args.kernels]
    env, _ = cases.product_model(case)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    vm = _value_model(case, env).planner_value_model()
    rm = NativeRewardModel(od, ad, HIDDEN, "relu")
    rm.set_weights(rmc.reward_weights(od, ad, HIDDEN))
    rm.set_norm(rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0]))
    m, n, h = case["m"], case["n"], case["h"]
    dev = vm.device
    state = torch.randn((m * n, od), dtype=torch.float32, device=dev)
    nxt = state + 0.1 * torch.randn((m * n, od), dtype=torch.float32, device=dev)
    act = torch.empty((m * n, ad), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
    rets = torch.randn((m, n), dtype=torch.float32, device=dev)
    out = torch.empty((m * n,), dtype=torch.float32, device=dev)
    best = torch.empty((m,), dtype=torch.int64, device=dev)
    for _ in range(args.steps):                 # the two launches take turns
        vm.terminal(state, rets, m, n, h, 1.0, returns_out=out, best_key=best)
        rm.predict(state, act, nxt, out=out)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Name"]:
                    lines.append(dict(kind="kernel", shape=args.shape, kernel=k, name=row["Name"], calls=int(row["Calls"]),
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
    ap.add_argument("--no-value", action="store_true", help="the four plain variants only (a checkout without the feature)")
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's fold and reward-model predict for a profiler")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the tree was measured)")
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
