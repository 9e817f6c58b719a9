"""What planning under a termination program costs (``MPCController(termination=...)``), on the config-1 shape (n = 500, h = 10,
one 2 x 512 model), the GrBAL default shape (ant, 5 adapted 3 x 512 sets, 5 x 500 candidates, h = 10) and BASELINE config 2
(n = 2000, h = 30, 5 x 26-512-512-20 mean).  Per shape the controllers share the recipe's weights and take turns call by call in
one process after a warm-up; p50 of ``--steps`` ``get_actions`` calls each, ``--repeats`` times (the spread of the p50s is recorded):

    {rs, cem} x {program, model, value} x {plain, never, half}
        rs / cem         ``rng="device"`` random shooting / one-iteration device-mode CEM
        program          a ``RewardProgram`` env (trajectory rollout + scorer)
        model            a (256, 256) ``MLPRewardModel`` (``use_reward_model``)
        value            the program env with a (256, 256) ``MLPValueModel``
        plain            the same controller without a termination program
        never / half     one guard on one coordinate that never fires (``[-inf, inf]``) / whose lower bound is bisected on the
                         random-shooting controller's own plan until about half of its candidates terminate (the share of the
                         last warm-up plan is recorded per variant from ``termination_diagnostics``; CEM's candidates are drawn
                         around its mean, so its share differs)

    python tools/probe_termination.py [--steps 1000] [--warmup 50] [--repeats 3] [--shapes ...] [--out profiles/termination.jsonl]

The new kernel's own time next to ``l2a_score_traj_k``'s comes from a run under the profiler with no counters in it; ``--kernels
SHAPE`` is the program to trace and ``--stats CSV --shape SHAPE`` appends both kernels' rows:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o SHAPE -- python tools/probe_termination.py --kernels SHAPE --guards never|half
    python tools/probe_termination.py --stats DIR/.../SHAPE_kernel_stats.csv --shape SHAPE --guards never|half [--out profiles/termination.jsonl]

``--closed-loop`` runs 50 steps on ``SyntheticEnv``'s toy system with a guard on one coordinate, the toy dynamics fitted as usual,
with and without ``termination=`` (a figure, not a test): steps survived and reward collected.
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
SHAPES = {"config1": dict(env="half_cheetah", mode="single", hidden=(512, 512), E=1, n=500, h=10, m=1, planner="rs"),
          "grbal": dict(env="ant", mode="per_block", hidden=(512, 512, 512), E=5, n=500, h=10, m=5, planner="rs"),
          "config2": dict(env="half_cheetah", mode="mean", hidden=(512, 512), E=5, n=2000, h=30, m=1, planner="rs")}
KERNELS = ("l2a_score_term_k", "l2a_score_traj_k")
INF = float("inf")


def _half_guard(case, coord=0):
    """A lower bound on one coordinate under which about half of a random-shooting plan's candidates terminate: bisected on the
    terminated share that ``termination_diagnostics`` reports for the controller's own plan (same seed at every trial), between
    the lowest and the highest value the coordinate takes along the model's predicted trajectories of random candidates."""
    import torch
    import cases
    import reward_program_cases as rpc
    from learning_to_adapt_amd.envs import TerminationProgram
    from learning_to_adapt_amd.utils import synthetic
    env, model = cases.product_model(case)
    native = model.planner_model()
    m, n, h = case["m"], case["n"], case["h"]
    obs = synthetic.make_obs0(m, native.obs_dim)
    obs0 = torch.from_numpy(obs.astype(np.float32)).to(native.device)
    low, high = env.action_space.low, env.action_space.high
    a = torch.from_numpy(np.random.RandomState(0).uniform(low, high, (h, m * n, native.act_dim)).astype(np.float32)).to(native.device)
    x = native.rollout_traj(obs0, a, m, n, h)[:, :, coord].cpu().numpy()
    lo, hi = float(x.min()), float(x.max())
    term = TerminationProgram().alive_in_range(coord, lo, INF)
    ctrl = cases.product_controller(dict(case, planner="rs"), model=model, env=rpc.program_env(case["env"]), rng="device",
                                    termination=term)
    for _ in range(16):
        mid = 0.5 * (lo + hi)
        term.guards[0].lo = mid                     # the controller hands this very struct to the library at every plan
        torch.manual_seed(1)
        ctrl.get_actions(obs)
        share = float(np.mean(ctrl.termination_diagnostics()["terminated"]))
        if share > 0.5:
            hi = mid
        else:
            lo = mid
    return coord, float(np.float32(0.5 * (lo + hi)))


def _termination(kind, od, guard):
    """Both variants carry ONE one-element guard on the same coordinate, so that they differ in the dead rows alone."""
    from learning_to_adapt_amd.envs import TerminationProgram
    if kind == "never":
        return TerminationProgram().alive_in_range(guard[0], -INF, INF)
    return TerminationProgram().alive_in_range(guard[0], guard[1], INF)


def _controllers(case, guard):
    import cases
    import reward_model_cases as rmc
    import reward_program_cases as rpc
    import value_model_cases as vmc
    from learning_to_adapt_amd.dynamics import MLPRewardModel, MLPValueModel
    out = {}
    for planner in ("rs", "cem"):
        for reward in ("program", "model", "value"):
            for term in ("plain", "never", "half"):
                env, model = cases.product_model(case)
                od, ad = env.observation_space.shape[0], env.action_space.shape[0]
                base = cases.recipe(case)[2][0]
                kw = dict(rng="device")
                if planner == "cem":
                    kw.update(cem_mode="fixed")
                if reward == "model":
                    rm = MLPRewardModel(name="rew", env=env, hidden_sizes=HIDDEN, init_seed=0)
                    rm.set_params(rmc.reward_weights(od, ad, HIDDEN))
                    rm.set_normalization(rmc.reward_norm(od, ad, base=base))
                    kw.update(reward_model=rm, use_reward_model=True)
                else:
                    env = rpc.program_env(case["env"])
                if reward == "value":
                    vm = MLPValueModel(name="val", env=env, hidden_sizes=HIDDEN, init_seed=0)
                    vm.set_params(vmc.value_weights(od, HIDDEN))
                    vm.set_normalization(vmc.value_norm(od, base=base))
                    kw.update(value_model=vm, terminal_value_coef=1.0)
                if term != "plain":
                    kw.update(termination=_termination(term, od, guard))
                out["%s_%s_%s" % (planner, reward, term)] = cases.product_controller(
                    dict(case, planner=planner, num_cem_iters=1), model=model, env=env, **kw)
    return out


def latency(args):
    import torch
    from learning_to_adapt_amd.utils import synthetic
    lines = []
    for shape in args.shapes.split(","):
        case = SHAPES[shape]
        torch.manual_seed(1)
        guard = _half_guard(case)
        ctrls = _controllers(case, guard)
        obs = synthetic.make_obs0(case["m"], ctrls["rs_program_plain"].env.observation_space.shape[0])
        for _ in range(args.warmup):
            for c in ctrls.values():
                c.get_actions(obs)
        torch.cuda.synchronize()
        dead = {v: (float(np.mean(c.termination_diagnostics()["terminated"])) if c.termination_diagnostics() else None)
                for v, c in ctrls.items()}
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
            plain = float(np.median(p50[v.rsplit("_", 1)[0] + "_plain"]))
            rec = dict(kind="latency", shape=shape, variant=v, env=case["env"], hidden=list(case["hidden"]), E=case["E"], n=case["n"],
                       m=case["m"], h=case["h"], steps=args.steps, repeats=args.repeats, p50_ms=round(mid, 4),
                       p50_ms_repeats=[round(x, 4) for x in p50[v]], spread_ms=round(max(p50[v]) - min(p50[v]), 4),
                       over_plain_ms=round(mid - plain, 4), terminated_share=dead[v], guard=list(guard) if v.endswith("half") else None,
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del ctrls
    return lines


def kernels(args):
    """The program to trace: the new kernel and ``l2a_score_traj_k`` on the same trajectory, taking turns.  ``--guards never``: one
    guard that never fires; ``--guards half``: its lower bound at the median over the candidates of the coordinate's lowest value
    along this very trajectory, so that half of the rows die before the horizon's end."""
    import torch
    import cases
    import reward_program_cases as rpc
    from learning_to_adapt_amd import _lib
    torch.manual_seed(1)
    case = SHAPES[args.kernels]
    env, model = cases.product_model(case)
    native = model.planner_model()
    od, ad = native.obs_dim, native.act_dim
    m, n, h = case["m"], case["n"], case["h"]
    prog = rpc.new_reward_program(od, ad, env.dt)
    dev = native.device
    obs0 = torch.randn((m, od), dtype=torch.float32, device=dev)
    a = torch.empty((h, m * n, ad), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0)
    traj = native.rollout_traj(obs0, a, m, n, h)
    guard = (0, float(traj[:, :, 0].min(dim=0).values.median()))
    rets = torch.empty((m, n), dtype=torch.float32, device=dev)
    best = torch.empty((m,), dtype=torch.int64, device=dev)
    ctx = _lib.Context.get(0)
    term = _termination(args.guards, od, guard)
    for _ in range(args.steps):
        ctx.score_trajectory(obs0, traj, a, m, n, h, 1.0, prog, returns_out=rets, best_key=best)
        ctx.score_trajectory_term(obs0, traj, a, m, n, h, 1.0, term, program=prog, returns_out=rets, best_key=best)
    torch.cuda.synchronize()
    return []


def stats(args):
    lines = []
    with open(args.stats) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Name"]:
                    lines.append(dict(kind="kernel", shape=args.shape, guards=args.guards, kernel=k, name=row["Name"], calls=int(row["Calls"]),
                                      avg_us=round(float(row["AverageNs"]) / 1e3, 3), min_us=round(float(row["MinNs"]) / 1e3, 3),
                                      max_us=round(float(row["MaxNs"]) / 1e3, 3)))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    return lines


def closed_loop(args):
    """50 steps on the toy system, the dynamics model fitted on random transitions of it, with and without ``termination=``."""
    import torch
    from learning_to_adapt_amd.dynamics import MLPDynamicsModel
    from learning_to_adapt_amd.envs import SyntheticEnv, TerminationProgram
    from learning_to_adapt_amd.policies import MPCController
    torch.manual_seed(0)
    np.random.seed(0)
    env = SyntheticEnv("half_cheetah")
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    obs = 0.3 * np.random.randn(4000, od)
    act = np.random.uniform(-1.0, 1.0, (4000, ad))
    model = MLPDynamicsModel(name="dyn", env=env, hidden_sizes=(512, 512), init_seed=0)
    model.fit(obs, act, env.toy_dynamics(obs, act), epochs=30, verbose=False)
    coord = od - 4          # a coordinate the reward does not read
    term = TerminationProgram(terminal_reward=-10.0).alive_in_range(coord, -0.15, 0.15)
    lines = []
    for with_term in (False, True):
        env.termination_spec = None
        ctrl = MPCController(name="policy", env=env, dynamics_model=model, n_candidates=500, horizon=10, rng="device",
                             termination=term if with_term else None)
        env.termination_spec = term         # the env ends the episode either way
        torch.manual_seed(1)
        o = env.reset()
        total, survived = 0.0, 0
        for _ in range(50):
            action = np.asarray(ctrl.get_action(o)[0], dtype=np.float64).reshape(-1)
            o, r, done, _ = env.step(action)
            total += r
            survived += 1
            if done:
                break
        rec = dict(kind="closed_loop", env="half_cheetah toy", guard=[coord, -0.15, 0.15], terminal_reward=-10.0,
                   termination=with_term, steps_survived=survived, of=50, reward=round(total, 4),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--kernels", default="", choices=[""] + list(SHAPES), help="run this shape's scoring launches for a profiler")
    ap.add_argument("--guards", default="never", choices=["never", "half"], help="with --kernels / --stats: which guard was traced")
    ap.add_argument("--stats", default="", help="a rocprofv3 kernel-statistics CSV to take the kernels' rows from")
    ap.add_argument("--shape", default="config2", choices=list(SHAPES), help="the shape the --stats file was traced on")
    ap.add_argument("--closed-loop", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="recorded as `build` in every line (which state of the tree was measured)")
    args = ap.parse_args()
    lines = stats(args) if args.stats else kernels(args) if args.kernels else closed_loop(args) if args.closed_loop else latency(args)
    if args.tag:
        for rec in lines:
            rec["build"] = args.tag
    if args.out and lines:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
