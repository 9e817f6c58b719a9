"""Step latency of the SHARDED recurrent planner on the run_rebal.py default shape (m = 5, n = 500, h = 10, LSTM 256) as rank 0 of
two gloo ranks that share ONE GPU (tile split off, as tests/test_distributed_gpu.py), through two routes:

  python_glue   ``L2A_NATIVE_STEP=0``: slice, launch, payload, torch.distributed collective, read-back and the second host round trip
                of ``_advance_hidden`` in Python - the route every sharded recurrent plan took before
                ``l2a_lstm_controller_create_sharded`` existed
  c_step        the whole step in one C call, the state advanced on the device behind the collective

p50 / p99 of the host wall time of ``RNNMPCController.get_actions`` over ``--steps`` steps, ``--repeats`` runs per route (fresh
processes each), one JSON line per run.  ``host_ms`` = the step minus the GPU time of this rank's rollout launch (250 candidates per
env, timed alone with events in the same process before the steps); the C route also reports the stage table of
``l2a_controller_stats`` of its last step.  Two processes on one GPU and a gloo collective through the host: NOT a multi-GPU figure.

    python tools/probe_sharded_rnn_step.py [--steps 1000] [--warmup 50] [--repeats 3] [--out profiles/sharded_rnn_step.jsonl]
"""

import argparse
import json
import os
import socket
import sys
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = "c6_hc_rnn_rs_n500_h10_m5_s0"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, route, steps, warmup, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["L2A_SPLIT"] = "0"           # ranks sharing one GPU: a tile's two workgroups may not be co-resident
    os.environ["L2A_NATIVE_STEP"] = "1" if route == "c_step" else "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    try:
        import cases
        case, seed = cases.split_id(CID)
        obs = cases.load_golden(CID)["obs"][0]
        ctrl = cases.product_rnn_controller(case)
        ctrl.reset(dones=[True] * case["m"])
        np.random.seed(seed)
        # this rank's rollout launch alone (the other rank waits at the barrier)
        native = ctrl.dynamics_model.planner_model()
        m, h, U = case["m"], case["h"], native.units
        lo, hi = ctrl._shard_range(case["n"], rank, world)
        kernel_ms = None
        if rank == 0:
            dev = native.device
            a = torch.rand((h, m * (hi - lo), native.act_dim), device=dev) * 2 - 1
            z = torch.zeros((m, U), device=dev)
            o = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(dev)
            best = torch.zeros((m,), dtype=torch.int64, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ks = []
            for i in range(60):
                ev[0].record()
                native.plan_rs(o, z, z, a, m, hi - lo, h, 1.0, ctrl._reward_spec, cand_offset=lo, best_key=best)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= 10:
                    ks.append(ev[0].elapsed_time(ev[1]))
            kernel_ms = float(np.percentile(ks, 50))
        dist.barrier()
        for _ in range(warmup):
            ctrl.get_actions(obs)
        torch.cuda.synchronize()
        dist.barrier()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            ctrl.get_actions(obs)
            ts.append((time.perf_counter() - t0) * 1e3)
        served = ctrl._cstep is not None and ctrl._cstep.stats()["steps"] == steps + warmup
        assert served == (route == "c_step"), "the steps did not take the route under test"
        if rank == 0:
            p50 = float(np.percentile(ts, 50))
            rec = dict(route=route, shape="m5_n500_h10_lstm256", world=world, rank=rank, n_local=hi - lo, backend="gloo", gpus=1,
                       steps=steps, p50_ms=round(p50, 4), p99_ms=round(float(np.percentile(ts, 99)), 4),
                       mean_ms=round(float(np.mean(ts)), 4), min_ms=round(float(np.min(ts)), 4), kernel_ms=round(kernel_ms, 4),
                       host_ms=round(p50 - kernel_ms, 4), device=torch.cuda.get_device_name(0))
            if served:
                s = ctrl._cstep.stats()
                rec["stage_us_last_step"] = {k: round(v, 1) for k, v in s["stage_us"].items()}
                rec["chain"] = dict(hits=s["hits"], misses=s["misses"], sync_draws=s["sync_draws"], relaunches=s["relaunches"])
            with open(out_path, "w") as f:
                f.write(json.dumps(rec))
        if ctrl._cstep is not None:
            ctrl._cstep.close()
        if getattr(ctrl, "_ahead", None) is not None:
            ctrl._ahead.stop()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--tmp", default="/tmp")
    args = ap.parse_args()
    for run in range(args.repeats):
        for route in ("python_glue", "c_step"):
            path = os.path.join(args.tmp, "sharded_rnn_step_%d_%s_%d.json" % (os.getpid(), route, run))
            mp.spawn(_worker, args=(2, _free_port(), route, args.steps, args.warmup, path), nprocs=2, join=True)
            rec = json.load(open(path))
            os.remove(path)
            rec["run"] = run
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
