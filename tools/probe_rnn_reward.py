#!/usr/bin/env python
"""What the recurrent planner costs with a reward program or a learned reward model, end to end through
``RNNMPCController.get_actions`` (parity mode, one GPU, LSTM 256, HalfCheetah shapes):

* program / model            - the new paths: ``l2a_lstm_plan_rs_program`` on a ``RewardProgram`` env, and
  ``l2a_lstm_plan_rs_reward_model`` with ``native_reward_model=True`` and a (256, 256) reward net;
* program_loop / model_loop  - the same env / model behind the unfused loop only (``_get_rs_action_unfused``: h host round
  trips of ``dynamics_model.predict``): the env's ``reward_spec`` hidden from the controller, the model behind a wrapper that
  exposes only ``predict``;
* formula_program / formula  - HalfCheetah's own reward as a program against the fused ``RewardSpec`` launch;

plus the rollout part alone (``l2a_lstm_rollout_traj``): the single launch of the trajectory-writing micro-tile kernel
(``l2a_set_micro(2)``) against the carry chain (``l2a_set_micro(0)``) on the same plan, HIP events around ``--calls`` launches
of each, taken in alternating batches.  At the ReBAL default (m=5, n=500, h=10) and at n=2000, h=30, m=1.  The variants of a
shape take turns call by call; p50 of ``--calls`` (200) calls after warm-up; every call ends in the read-back of the keys, so
the host clock covers the GPU work.  Appends one JSON line per shape to ``--out``.

    python tools/probe_rnn_reward.py [--calls=200] [--out=profiles/rnn_reward_paths.jsonl]
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
from learning_to_adapt_amd import _lib  # noqa: E402
from learning_to_adapt_amd.dynamics import MLPRewardModel  # noqa: E402
from learning_to_adapt_amd.envs import RewardProgram  # noqa: E402
from learning_to_adapt_amd.policies import RNNMPCController  # noqa: E402

HIDDEN = (256, 256)
BATCH = 20


class PredictOnly(object):
    def __init__(self, model):
        self.model = model

    def predict(self, obs, act, nxt):
        return self.model.predict(obs, act, nxt)


def controllers(case):
    """The six controllers of a shape, one dynamics model each (same recipe weights)."""
    out = {}
    for name in ("program", "model", "program_loop", "model_loop", "formula_program", "formula"):
        env, model = cases.product_rnn_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        kw = {}
        if name.startswith("program"):
            env.reward_spec = rpc.new_reward_program(od, ad, env.dt)
        elif name == "formula_program":
            env.reward_spec = RewardProgram.from_spec(env.reward_spec, od, ad)
        elif name.startswith("model"):
            rm = MLPRewardModel(name="rew", env=env, hidden_sizes=HIDDEN, init_seed=0)
            rm.set_params(rmc.reward_weights(od, ad, HIDDEN))
            rm.set_normalization(rmc.reward_norm(od, ad, base=cases.rnn_recipe(case)[2]))
            kw = dict(reward_model=rm if name == "model" else PredictOnly(rm), use_reward_model=True, native_reward_model=True)
        c = RNNMPCController(name="policy", env=env, dynamics_model=model, discount=case.get("discount", 1.0),
                             n_candidates=case["n"], horizon=case["h"], **kw)
        if name == "program_loop":
            c._reward_spec = None           # the controller does not see the program: the env's `reward` on the host, step by step
        out[name] = c
    assert out["program"]._program() and out["model"]._program() and out["formula_program"]._program()
    assert not out["program_loop"]._fusable() and not out["model_loop"]._fusable()
    assert out["formula"]._fusable() and not out["formula"]._program()
    return out


def rollout_alone_ms(ctrl, case, calls):
    """``l2a_lstm_rollout_traj`` alone: single launch (micro policy 2) and chain (0) in alternating batches of BATCH launches."""
    m, n, h = case["m"], case["n"], case["h"]
    native = ctrl.dynamics_model.planner_model()
    dev, ctx = native.device, native.ctx
    rs = np.random.RandomState(2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    obs0, acts = up(rs.randn(m, native.obs_dim)), up(rs.uniform(-1.0, 1.0, (h, m * n, native.act_dim)))
    c0, h0 = up(rs.randn(m, native.units)), up(np.tanh(rs.randn(m, native.units)))
    traj = torch.empty((h, m * n, native.obs_dim), dtype=torch.float32, device=dev)
    geo = {p: _lib.lstm_traj_geometry(native.obs_dim, native.act_dim, native.units, m, n, h, micro=p,
                                      cus=ctx.info()["compute_units"]) for p in (0, 1, 2)}
    per = {2: [], 0: []}
    try:
        for policy in (2, 0):
            ctx.set_micro(policy)
            for _ in range(10):
                native.rollout_traj(obs0, c0, h0, acts, m, n, h, traj_out=traj)
        torch.cuda.synchronize()
        for _ in range(max(calls // BATCH, 1)):
            for policy in (2, 0):                               # the variants take turns
                ctx.set_micro(policy)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(BATCH):
                    native.rollout_traj(obs0, c0, h0, acts, m, n, h, traj_out=traj)
                stop.record()
                torch.cuda.synchronize()
                per[policy].append(start.elapsed_time(stop) / BATCH)
    finally:
        ctx.set_micro(1)
    single, chain = float(np.mean(per[2])), float(np.mean(per[0]))
    return dict(single_ms=round(single, 4), chain_ms=round(chain, 4), single_over_chain=round(single / chain, 4),
                single_batches_ms=[round(v, 4) for v in per[2]], chain_batches_ms=[round(v, 4) for v in per[0]],
                spread_of_batch_ratios=round(float(np.std(np.array(per[2]) / np.array(per[0]))), 4),
                automatic_path="single" if geo[1]["single"] else "chain", single_geometry=geo[2])


def run(tag, case, calls, warmup=20):
    ctrls = controllers(case)
    obs = np.random.RandomState(1).randn(case["m"], 20)
    for c in ctrls.values():
        np.random.seed(0)
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
    native = ctrls["program"].dynamics_model.planner_model()
    row = dict(shape=tag, n=case["n"], h=case["h"], m=case["m"], units=case["units"], reward_hidden=list(HIDDEN), calls=calls,
               p50_ms={k: round(v, 4) for k, v in p50.items()},
               p95_ms={k: round(float(np.percentile(v, 95)), 4) for k, v in times.items()},
               program_over_loop=round(p50["program"] / p50["program_loop"], 4),
               model_over_loop=round(p50["model"] / p50["model_loop"], 4),
               formula_program_over_fused=round(p50["formula_program"] / p50["formula"], 4),
               rollout=rollout_alone_ms(ctrls["program"], case, calls),
               program_plans=int(native.program_plans), device=native.ctx.info().get("name"))
    for c in ctrls.values():
        if getattr(c, "_cstep", None) is not None:
            c._cstep.close()
            c._cstep = None
        if getattr(c, "_ahead", None) is not None:
            c._ahead.stop()
    return row


if __name__ == "__main__":
    calls, out = 200, os.path.join(ROOT, "profiles", "rnn_reward_paths.jsonl")
    for a in sys.argv[1:]:
        if a.startswith("--calls="):
            calls = int(a.split("=")[1])
        if a.startswith("--out="):
            out = a.split("=", 1)[1]
    if not torch.cuda.is_available():
        raise SystemExit("probe_rnn_reward.py times GPU plans: no GPU visible")
    base = cases.CASES["c6_hc_rnn_rs_n500_h10_m5"]
    for tag, case in (("ReBAL default (m=5, n=500, h=10, LSTM 256)", base),
                      ("n=2000, h=30, m=1, LSTM 256", dict(base, n=2000, h=30, m=1))):
        row = run(tag, case, calls)
        print(json.dumps(row), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(row) + "\n")
