"""Device time of one CEM iteration boundary on config 5's shape (m = 1, n = 4000, h = 30, act_dim = 6, 400 elites): the fused
``l2a_cem_refit_sample`` against ``l2a_cem_refit`` + ``l2a_cem_sample``, both readings, the whole plan and the 500-candidate shard of
an 8-way plan, and every return tied (the ranking's worst case: one value bin).  Prints one JSON line per case (HIP-event time per
iteration boundary, median of `--reps` batches); run under
``rocprofv3 --kernel-trace --stats`` for the per-kernel table.

    python tools/probe_cem_refit_sample.py [--iters 200] [--reps 5] [--out profiles/cem_refit_sample.jsonl]
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from learning_to_adapt_amd import _lib  # noqa: E402
from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = _lib.Context.get(0)
    lib = ctx.lib
    dev = torch.device("cuda:0")
    n, m, h, ad, k, alpha = 4000, 1, 30, 6, 400, 0.1
    D = h * ad
    rs = np.random.RandomState(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    rets_random = up(rs.randn(m, n))
    rets_equal = torch.full((m, n), 1.5, device=dev)       # every return tied (a constant reward, or every rollout diverged)
    a_in = [up(rs.randn(n, m, D)), torch.empty((n, m, D), device=dev)]
    mean = [up(0.3 * rs.randn(m, D)), torch.empty((m, D), device=dev)]
    std = torch.empty((m, D), device=dev)
    a_raw = torch.empty((n, m, D), device=dev)
    low, high = up(-np.ones(ad)), up(np.ones(ad))
    rows = torch.empty((m * k,), dtype=torch.int32, device=dev)
    stream = _stream_ptr(dev)
    lines = []
    cases = [(ref, shard, "random") for ref in (1, 0) for shard in ((0, n), (0, 500))] + [(1, (0, n), "all_equal"), (0, (0, n), "all_equal")]
    for reference, (lo, hi), kind in cases:
        rets = rets_random if kind == "random" else rets_equal
        seq = torch.empty((h, m * (hi - lo), ad), device=dev)

        def two(i):
            ctx.check(lib.l2a_cem_refit(ctx.handle, _ptr(rets), _ptr(a_in[0]), n, m, D, k, reference, alpha, _ptr(rows),
                                        _ptr(mean[1]), _ptr(std), stream), "l2a_cem_refit")
            ctx.check(lib.l2a_cem_sample(ctx.handle, None, ctypes.c_ulonglong(7), ctypes.c_ulonglong(i * n * m * D), _ptr(mean[1]),
                                         _ptr(std), _ptr(low), _ptr(high), n, m, h, ad, reference, lo, hi, _ptr(a_in[1]),
                                         _ptr(a_raw), _ptr(seq), stream), "l2a_cem_sample")

        def fused(i):
            ctx.check(lib.l2a_cem_refit_sample(ctx.handle, _ptr(rets), _ptr(a_in[0]), n, m, h, ad, k, reference, alpha, None,
                                               ctypes.c_ulonglong(7), ctypes.c_ulonglong(i * n * m * D), _ptr(low), _ptr(high), lo,
                                               hi, _ptr(rows), _ptr(mean[0]), _ptr(mean[1]), _ptr(std), _ptr(a_in[1]),
                                               _ptr(a_raw), _ptr(seq), stream), "l2a_cem_refit_sample")

        for name, fn in (("refit+sample", two), ("refit_sample", fused)):
            for i in range(10):
                fn(i)
            per = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.iters):
                    fn(i)
                e1.record()
                e1.synchronize()
                per.append(e0.elapsed_time(e1) * 1000.0 / args.iters)
            rec = dict(path=name, reference=reference, returns=kind, n=n, m=m, h=h, act_dim=ad, elites=k, shard=[lo, hi],
                       us_per_iteration=round(float(np.median(per)), 2), reps=[round(x, 2) for x in per],
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
