#!/usr/bin/env python
"""What the MLP planner's trajectory rollout costs as ONE launch of the trajectory-writing micro-tile kernel against the carry
chain of ``h`` one-step launches - per class of plan, against the chain of the PARENT build.

One process loads one library (``L2A_LIB_PATH`` selects a parent build, which has no ``l2a_rollout_traj``), so the comparison
takes two steps:

    python tools/probe_mlp_traj.py --tag=parent --raw=OUT.raw.jsonl      # with L2A_LIB_PATH=<the parent's libl2a_hip.so>
    python tools/probe_mlp_traj.py --tag=new    --raw=OUT.raw.jsonl      # the tree's own build
    ... the two in alternation, at least twice each ...
    python tools/probe_mlp_traj.py --combine=OUT.raw.jsonl --out=profiles/mlp_traj.jsonl

A measuring process times, for every plan of PLANS (h = 10):

* ``plan_rs_program`` (rollout + scoring launch, the library's own trajectory buffer) under the micro policies the library has:
  the parent's is the chain; the new build's 0 = its own chain, 2 = the single launch where eligible, 1 = the automatic rule;
* new build only: ``rollout_traj`` alone under policies 2 and 0; and, in front of all turns, ``plan_rs_program`` under the
  automatic policy alone (``auto_alone``: batch after batch of the same call, exactly what the parent's process runs);

HIP events around batches of BATCH calls, the variants taking turns batch by batch, ``--calls`` (200) calls each after warm-up;
the figure of a variant is the p50 of its batches.  And, for the config-1 shape and the GrBAL default, parity-mode
``MPCController.get_actions`` with a program env and with a native reward model (host clock around calls that end in the
read-back of the keys).

``--combine`` writes one line per plan: p50 over the processes of each side, ``single_over_parent_chain`` (policy 2 of the new
build over the parent), ``chain_over_parent_chain`` (policy 0 over the parent), ``auto_over_parent_chain`` (policy 1), ``auto_alone_over_parent_chain`` and
``spread``: the larger of the two sides' run-to-run spreads, (max - min) / median over the processes of a side.  A class of plan
belongs to the automatic rule when ``single_over_parent_chain < 1 - spread`` for every measured plan of the class.
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

BATCH = 20
H = 10
HC, ANT = (20, 6, 0.01), (41, 8, 0.02)
#        tag,                              dims, hidden,          mode,        E, m, n
PLANS = [("config-1 (2x512, n=500)", HC, (512, 512), "single", 1, 1, 500),
         ("GrBAL default (5 adapted 3x512, n=500)", ANT, (512, 512, 512), "per_block", 5, 5, 500),
         ("2x256, n=500", HC, (256, 256), "single", 1, 1, 500),
         ("5 adapted 3x256, n=500", ANT, (256, 256, 256), "per_block", 5, 5, 500),
         ("mean E=5 2x512, n=100", HC, (512, 512), "mean", 5, 1, 100),
         ("mean E=5 2x512, n=500", HC, (512, 512), "mean", 5, 1, 500),
         ("2x512, n=3000 (three micro tiles per CU)", HC, (512, 512), "single", 1, 1, 3000),
         ("mean E=5 2x512, n=3000 (three micro tiles per CU)", HC, (512, 512), "mean", 5, 1, 3000),
         ("mean E=5 2x512, n=2100 (just above CUs/2 tiles)", HC, (512, 512), "mean", 5, 1, 2100),
         ("mean E=5 2x256, n=2100 (just above CUs/2 tiles)", HC, (256, 256), "mean", 5, 1, 2100),
         ("2x512, n=100", HC, (512, 512), "single", 1, 1, 100),
         ("mean E=5 2x256, n=500", HC, (256, 256), "mean", 5, 1, 500),
         ("mean E=5 2x256, n=3000 (three micro tiles per CU)", HC, (256, 256), "mean", 5, 1, 3000)]


def plan_class(hidden, mode, E, m, n, cus):
    tiles16 = m * ((n + 15) // 16)
    return "%d / %s / %s" % (hidden[0], "ensemble" if mode == "mean" and E > 1 else "one set",
                             "at most CUs/2 tiles" if 2 * tiles16 <= cus else "more than CUs/2 tiles")


def timed_batches(variants, calls):
    """variants: name -> (prepare, call).  Alternating batches of BATCH calls between HIP events -> name -> [ms per call]."""
    per = {k: [] for k in variants}
    for prepare, call in variants.values():
        prepare()
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    for _ in range(max(calls // BATCH, 1)):
        for name, (prepare, call) in variants.items():
            prepare()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(BATCH):
                call()
            stop.record()
            torch.cuda.synchronize()
            per[name].append(start.elapsed_time(stop) / BATCH)
    return per


def measure_plan(tag, row, calls):
    import reward_program_cases as rpc
    from learning_to_adapt_amd import _lib
    from learning_to_adapt_amd.dynamics.native_model import NativeModel
    from learning_to_adapt_amd.utils import synthetic
    name, (od, ad, dt), hidden, mode, E, m, n = row
    native = NativeModel(od, ad, list(hidden), "relu", None, E, mode)
    low, high = -np.ones(ad), np.ones(ad)
    for e in range(E):
        native.set_weights(e, synthetic.make_weight_set(od, ad, list(hidden), 100 + e))
        native.set_norm(e, synthetic.make_norm(od, ad, low, high, 200 + e))
    dev, ctx = native.device, native.ctx
    cus = ctx.info()["compute_units"]
    rs = np.random.RandomState(2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    obs0, acts = up(rs.randn(m, od)), up(rs.uniform(low, high, (H, m * n, ad)))
    best = torch.zeros((m,), dtype=torch.int64, device=dev)
    prog = rpc.new_reward_program(od, ad, dt)
    has_traj = hasattr(_lib.load(), "l2a_rollout_traj")
    variants = {}

    def program():
        native.plan_rs_program(obs0, acts, m, n, H, 1.0, prog, best_key=best)

    if has_traj:
        traj = torch.empty((H, m * n, od), dtype=torch.float32, device=dev)
        for policy in (0, 1, 2):
            variants["program_micro%d" % policy] = ((lambda p=policy: ctx.set_micro(p)), program)
        for policy in (0, 2):
            variants["rollout_micro%d" % policy] = ((lambda p=policy: ctx.set_micro(p)),
                                                    (lambda: native.rollout_traj(obs0, acts, m, n, H, traj_out=traj)))
        geo = {p: _lib.mlp_traj_geometry(od, ad, len(hidden), hidden[0], mode, E, m, n, H, micro=p, cus=cus) for p in (1, 2)}
    else:
        variants["program_micro1"] = ((lambda: None), program)
        geo = None
    try:
        # the automatic policy alone first - what the parent's process measures, batch after batch of the same call - then the turns
        per = timed_batches({"program_auto_alone": ((lambda: ctx.set_micro(1)), program)}, calls) if has_traj else {}
        per.update(timed_batches(variants, calls))
    finally:
        ctx.set_micro(1)
    keys = best.cpu().numpy().view(np.uint64).tolist()
    return dict(kind="plan", tag=tag, plan=name, plan_class=plan_class(hidden, mode, E, m, n, cus), m=m, n=n, h=H, hidden=list(hidden),
                mode=mode, n_sets=E, obs_dim=od, act_dim=ad, calls=calls, compute_units=cus,
                p50_ms={k: round(float(np.median(v)), 5) for k, v in per.items()},
                batches_ms={k: [round(x, 5) for x in v] for k, v in per.items()},
                geometry=geo, keys=[str(k) for k in keys], device=ctx.info().get("name"))


def measure_controllers(tag, calls):
    import cases
    import reward_model_cases as rmc
    import reward_program_cases as rpc
    from learning_to_adapt_amd.dynamics import MLPRewardModel
    from learning_to_adapt_amd.policies import MPCController
    rows = []
    shapes = (("config-1 (2x512, n=500)", dict(cases.CASES["c1_hc_rs_n500_h10_e1"])),
              ("GrBAL default (5 adapted 3x512, n=500)", dict(cases.CASES["c3b_ant_rs_n500_h10_pb5_3x512"])))
    for name, case in shapes:
        ctrls = {}
        for kind in ("program", "model"):
            env, model = cases.product_model(case)
            od, ad = env.observation_space.shape[0], env.action_space.shape[0]
            kw = {}
            if kind == "program":
                env = rpc.program_env(case["env"])
            else:
                rm = MLPRewardModel(name="rew", env=env, hidden_sizes=(256, 256), init_seed=0)
                rm.set_params(rmc.reward_weights(od, ad, (256, 256)))
                rm.set_normalization(rmc.reward_norm(od, ad, base=cases.recipe(case)[2][0]))
                kw = dict(reward_model=rm, use_reward_model=True)
            ctrls[kind] = MPCController(name="policy", env=env, dynamics_model=model, discount=1.0, n_candidates=case["n"],
                                        horizon=case["h"], use_cem=False, **kw)
            assert ctrls[kind]._program()
        obs = np.random.RandomState(1).randn(case["m"], od)
        for c in ctrls.values():
            np.random.seed(0)
            for _ in range(20):
                c.get_actions(obs)
        torch.cuda.synchronize()
        times = {k: [] for k in ctrls}
        for _ in range(calls):
            for k, c in ctrls.items():
                t0 = time.perf_counter()
                c.get_actions(obs)
                times[k].append(1e3 * (time.perf_counter() - t0))
        rows.append(dict(kind="controller", tag=tag, plan=name, calls=calls,
                         p50_ms={k: round(float(np.percentile(v, 50)), 4) for k, v in times.items()},
                         p95_ms={k: round(float(np.percentile(v, 95)), 4) for k, v in times.items()}))
        for c in ctrls.values():
            if getattr(c, "_cstep", None) is not None:
                c._cstep.close()
                c._cstep = None
            if getattr(c, "_ahead", None) is not None:
                c._ahead.stop()
    return rows


def combine(raw, out):
    rows = [json.loads(line) for line in open(raw) if line.strip()]
    lines = []

    def side(plan, kind, tag, key):
        v = [r["p50_ms"][key] for r in rows if r["kind"] == kind and r["plan"] == plan and r["tag"] == tag and key in r["p50_ms"]]
        if not v:
            return None, None, []
        return float(np.median(v)), (max(v) - min(v)) / float(np.median(v)), v

    for plan in dict.fromkeys(r["plan"] for r in rows if r["kind"] == "plan"):
        first = next(r for r in rows if r["kind"] == "plan" and r["plan"] == plan and r["tag"] == "new")
        parent, sp_parent, v_parent = side(plan, "plan", "parent", "program_micro1")
        line = dict(kind="plan", plan=plan, plan_class=first["plan_class"], m=first["m"], n=first["n"], h=first["h"], hidden=first["hidden"],
                    mode=first["mode"], n_sets=first["n_sets"], compute_units=first["compute_units"], device=first["device"],
                    single_geometry=first["geometry"]["2"] if "2" in first["geometry"] else first["geometry"][2],
                    parent_chain_ms=round(parent, 5), parent_runs_ms=v_parent)
        spread = sp_parent
        for key, label in (("program_micro2", "single"), ("program_micro0", "chain"), ("program_micro1", "auto"),
                           ("program_auto_alone", "auto_alone")):
            new, sp_new, v_new = side(plan, "plan", "new", key)
            line[label + "_ms"] = round(new, 5)
            line[label + "_runs_ms"] = v_new
            line[label + "_over_parent_chain"] = round(new / parent, 4)
            if label == "single":
                spread = max(spread, sp_new)
        line["spread"] = round(spread, 4)
        line["single_wins"] = bool(line["single_over_parent_chain"] < 1.0 - spread)
        r2, _, _ = side(plan, "plan", "new", "rollout_micro2")
        r0, _, _ = side(plan, "plan", "new", "rollout_micro0")
        line["rollout_alone_single_ms"], line["rollout_alone_chain_ms"] = round(r2, 5), round(r0, 5)
        line["rollout_alone_single_over_chain"] = round(r2 / r0, 4)
        keys = set(tuple(r["keys"]) for r in rows if r["kind"] == "plan" and r["plan"] == plan)
        line["same_keys_on_every_run"] = len(keys) == 1
        lines.append(line)
    for plan in dict.fromkeys(r["plan"] for r in rows if r["kind"] == "controller"):
        line = dict(kind="controller get_actions (parity mode)", plan=plan)
        for key in ("program", "model"):
            parent, sp_parent, v_parent = side(plan, "controller", "parent", key)
            new, sp_new, v_new = side(plan, "controller", "new", key)
            line[key] = dict(parent_ms=round(parent, 4), new_ms=round(new, 4), new_over_parent=round(new / parent, 4),
                             spread=round(max(sp_parent, sp_new), 4), parent_runs_ms=v_parent, new_runs_ms=v_new)
        lines.append(line)
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


if __name__ == "__main__":
    calls, out, raw, tag, comb, only = 200, os.path.join(ROOT, "profiles", "mlp_traj.jsonl"), None, "new", None, None
    for a in sys.argv[1:]:
        if a.startswith("--calls="):
            calls = int(a.split("=")[1])
        if a.startswith("--out="):
            out = a.split("=", 1)[1]
        if a.startswith("--raw="):
            raw = a.split("=", 1)[1]
        if a.startswith("--tag="):
            tag = a.split("=", 1)[1]
        if a.startswith("--combine="):
            comb = a.split("=", 1)[1]
        if a.startswith("--only="):
            only = a.split("=", 1)[1]
    if comb:
        combine(comb, out)
        sys.exit(0)
    if not torch.cuda.is_available():
        raise SystemExit("probe_mlp_traj.py times GPU plans: no GPU visible")
    if raw is None:
        raise SystemExit("--raw=FILE: where this process appends its rows (see the module docstring)")
    done = []
    if only != "controllers":
        done += [measure_plan(tag, row, calls) for row in PLANS]
    if only != "plans":
        done += measure_controllers(tag, calls)
    with open(raw, "a") as f:
        for row in done:
            f.write(json.dumps(row) + "\n")
            print(json.dumps({k: v for k, v in row.items() if k != "batches_ms"}), flush=True)
