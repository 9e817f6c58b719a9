"""Plan-step latency of TS1 particle planning (``MPCController(ensemble_planning="particles", particle_sampling="ts1")``) next to
the TS-infinity step, on the four shapes of ``tools/probe_particles.py``: BASELINE config 2 (n = 2000, h = 30, 5 x 26-512-512-20)
and the GrBAL default shape (ant, 3 x 512, n = 500, h = 10) with an E = 5 mean ensemble, each for one env and for five.  Per shape
the two planners share the recipe's weights and take turns call by call in one process after a warm-up; p50 of ``--steps`` calls
each, ``--repeats`` times (the spread of the p50s is recorded):

    tsinf   the particle step as it was: draw, expand, m fused per-block launches, score, keys read back
    ts1     draw, expand, m h one-step launches with h - 1 shuffle launches between the steps, score, keys read back

    python tools/probe_particles_ts1.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/particles_ts1.jsonl]

``--rewards`` times the same two planners on an env whose reward is a program (``tests/reward_program_cases.py``:
``new_reward_program``) and with a learned reward model (``MLPRewardModel``, 256 x 256) in place of the fused formula, next to the
fused pair in the same process - six variants taking turns (``profiles/particles_ts1_rewards.jsonl``):

    tsinf_program / tsinf_rm   m trajectory rollouts and m scoring launches behind the expansion, then the particle score
    ts1_program / ts1_rm       m h one-step rollouts (and m h one-step reward-model launches), h step launches that take the
                               step's reward, accumulate and deal (``l2a_particle_step``), then the particle score

    python tools/probe_particles_ts1.py --rewards [--steps 1000] [--out profiles/particles_ts1_rewards.jsonl]

``ratio_to_tsinf`` is the price of TS1 (for a rewards variant: against its own TS-infinity counterpart); the ``tsinf`` rows stand next to the ``particles`` rows of ``profiles/particles.jsonl``
(the same step before TS1 existed).  Kernel times come from a run of their own under the profiler; ``--kernels SHAPE`` is the
program to trace (TS1 steps, nothing timed on the host) and ``--stats CSV --shape SHAPE`` appends the shuffle kernel's row next to
the expansion's and the scorer's rows of the same trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_particles_ts1.py --kernels SHAPE
    python tools/probe_particles_ts1.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE [--out profiles/particles_ts1.jsonl]
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

from probe_particles import RISK, SHAPES, _controllers      # noqa: E402  (the shapes and the recipe are that probe's)

KERNELS = ("l2a_particle_shuffle_k", "l2a_particle_step_k", "l2a_particle_expand_k", "l2a_particle_score_k")
VARIANTS = {"tsinf": dict(rng="device", ensemble_planning="particles", risk_coef=RISK),
            "ts1": dict(rng="device", ensemble_planning="particles", risk_coef=RISK, particle_sampling="ts1")}
RM_HIDDEN = (256, 256)
REWARD_VARIANTS = ("tsinf", "ts1", "tsinf_program", "ts1_program", "tsinf_rm", "ts1_rm")


def _reward_controllers(case, names=REWARD_VARIANTS):
    """The fused pair, the pair on an env with a reward program and the pair with a reward model: one dynamics model for all six."""
    import cases
    import reward_model_cases as rmc
    import reward_program_cases as rpc
    from learning_to_adapt_amd.dynamics import MLPRewardModel
    env, model = cases.product_model(case)
    penv, _ = cases.product_model(case)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    penv.reward_spec = rpc.new_reward_program(od, ad, penv.dt)
    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=RM_HIDDEN, init_seed=0)
    rm.set_params(rmc.reward_weights(od, ad, RM_HIDDEN))
    rm.set_normalization(rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0]))
    ctrls = {}
    for name in names:
        sampling, _, kind = name.partition("_")
        kw = dict(VARIANTS[sampling], ts1_step_rewards=True)
        if kind == "rm":
            kw.update(reward_model=rm, use_reward_model=True)
        ctrls[name] = cases.product_controller(case, model=model, env=penv if kind == "program" else env, **kw)
    return env, ctrls


def _launches(case, v):
    m, h = case["m"], case["h"]
    return {"tsinf": m + 2, "ts1": m * h + h + 1, "tsinf_program": 2 * m + 2, "ts1_program": m * h + h + 2,
            "tsinf_rm": 2 * m + 2, "ts1_rm": 2 * m * h + h + 2}[v]


def latency(args):
    import torch
    from learning_to_adapt_amd.utils import synthetic
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        torch.manual_seed(1)
        env, ctrls = _reward_controllers(case) if args.rewards else _controllers(case, VARIANTS)
        obs = synthetic.make_obs0(case["m"], env.observation_space.shape[0])
        steps = {v: (lambda c=ctrls[v]: c.get_actions(obs)) for v in ctrls}
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
        for v in steps:
            mid = float(np.median(p50[v]))
            base = float(np.median(p50["tsinf" + v[len(v.partition("_")[0]):]]))       # the variant's own TS-infinity counterpart
            launches = _launches(case, v)
            rec = dict(kind="latency", shape=shape, variant=v, env=case["env"], hidden=list(case["hidden"]), E=case["E"], n=case["n"],
                       m=case["m"], h=case["h"], risk_coef=RISK, launches=launches, steps=args.steps, repeats=args.repeats,
                       p50_ms=round(mid, 4), p50_ms_repeats=[round(x, 4) for x in p50[v]],
                       spread_ms=round(max(p50[v]) - min(p50[v]), 4), ratio_to_tsinf=round(mid / base, 4),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctrls, steps
    return lines


def kernels(args):
    """The program to trace: TS1 particle steps on one shape (``--variant``: the fused formula, a program or a reward model)."""
    import torch
    from learning_to_adapt_amd.utils import synthetic
    torch.manual_seed(1)
    case = SHAPES[args.kernels]
    env, ctrls = _reward_controllers(case, (args.variant,)) if args.variant != "ts1" else _controllers(case, {"ts1": VARIANTS["ts1"]})
    obs = synthetic.make_obs0(case["m"], env.observation_space.shape[0])
    for _ in range(args.steps):
        ctrls[args.variant].get_actions(obs)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k + "(" in row["Name"]:
                    lines.append(dict(kind="kernel", shape=args.shape, variant=args.variant, kernel=k, calls=int(row["Calls"]),
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
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's TS1 steps for a profiler")
    ap.add_argument("--rewards", action="store_true", help="time the program and reward-model variants next to the fused pair")
    ap.add_argument("--variant", default="ts1", choices=["ts1", "ts1_program", "ts1_rm"], help="what --kernels runs")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = stats(args) if args.stats else kernels(args) if args.kernels else latency(args)
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
