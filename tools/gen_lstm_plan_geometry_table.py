#!/usr/bin/env python
"""The launch the recurrent launcher picks over a grid of models, requests and policies (``l2a_lstm_plan_geometry``: no GPU
needed), digested into tests/lstm_plan_geometry_table.json - which tests/test_lstm_plan_geometry_table.py recomputes and
compares.  A geometry change shows there as a changed group; regenerate the file with this tool only when the change is meant:

    python tools/gen_lstm_plan_geometry_table.py            # rewrites both files

Per row: the return code and the 12 ints of the call (zeros when it fails).  The file holds, per model group, the CRC-32 of the
group's int32 rows in iteration order, and a histogram over the rows' classes.  The rows themselves go, column by column and
xz-compressed, to tests/golden/lstm_plan_geometry_rows.xz, so that a mismatch can be named row by row."""
import ctypes
import itertools
import json
import lzma
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import instance_matrix as im  # noqa: E402
from learning_to_adapt_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "lstm_plan_geometry_table.json")
ROWS = os.path.join(ROOT, "tests", "golden", "lstm_plan_geometry_rows.xz")

# the (obs_dim, act_dim) pairs on the edges of every (OT, KG0) of tests/instance_matrix.py
EDGE_DIMS = sorted({d for dims in im._DIMS.values() for d in dims} | set(im._DIMS_O4) | set(im._DIMS_K0L1))
MAIN_DIMS = [(20, 6), (64, 16)]
SMALL_LDS = 64 * 1024       # the tuned 512-unit kernel, the stacks' matrix-core rows and the stacks' micro tiles no longer fit


def groups():
    """[(key, obs_dim, act_dim, units, cell, full)]: `units` an int = the model of l2a_lstm_create, a list = l2a_rnn_create's;
    `full`: the whole request grid, else the three plan sizes of EDGE_N."""
    out = []

    def add(od, ad, units, cell, full):
        tag = "create%d" % units if isinstance(units, int) else "x".join(str(u) for u in units)
        out.append(("%dx%d|%s|%s" % (od, ad, cell, tag), od, ad, units, cell, full))

    for od, ad in MAIN_DIMS:
        for u in (128, 256, 512):                                   # the tuned LSTM kernel
            add(od, ad, [u], "lstm", True)
        for cell in ("lstm", "gru", "rnn"):                         # stacks of 256-unit layers (three of LSTM: the `publish` exception)
            for depth in (1, 2, 3):
                if not (cell == "lstm" and depth == 1):
                    add(od, ad, [256] * depth, cell, True)
        for cell in ("gru", "rnn"):                                 # ... of 512-unit layers
            add(od, ad, [512], cell, True)
        for cell, units in (("lstm", [256] * 4), ("lstm", [512] * 2), ("gru", [512] * 2), ("rnn", [512] * 3)):   # (too wide for any kernel)
            add(od, ad, units, cell, False)
    for od, ad in [d for d in EDGE_DIMS if d not in MAIN_DIMS]:
        for u in (128, 256, 512):
            add(od, ad, [u], "lstm", False)
    for r in im.GENERIC_ROWS:
        add(r.obs_dim, r.act_dim, list(r.units), r.cell, False)
    # the model of l2a_lstm_create at widths without a tuned instance (the VALU LSTM kernel; 1024 units: its rows do not fit),
    # one with; a stack too wide for the generic VALU kernel; input shapes outside the tuned kernel's at a micro-tile width
    for u in (100, 256, 1024):
        add(20, 6, u, "lstm", False)
    add(20, 6, [400, 400, 400], "gru", False)
    add(65, 3, [256, 256], "gru", False)
    add(20, 40, [256], "lstm", False)
    assert len({g[0] for g in out}) == len(out)
    return out


M = [1, 5]
N = [1, 4, 5, 16, 17, 37, 100, 500, 512, 1000, 2000, 2500, 3500, 4096, 8000, 16000]
EDGE_M = [1, 300]           # (300 envs: more than CUs - no micro-tile deal)
EDGE_N = [37, 500, 2500]
H = [3, 4096]
# request bits (_lib.LSTM_REQUEST_BITS): a plan | per-row states | a state written out | both (a chunk continuation) | no results |
# no split allowed | a state advance (per-row, state out, no split) | the trajectory rollout | ... with other bits set (ignored)
REQUEST = [0, 1, 2, 3, 4, 8, 11, 16, 23]
# the arguments of l2a_lstm_plan_geometry's policy that differ from the defaults (auto, 1, 1, 256, 160 KiB)
POLICY = [{}, {"kernel": 1}, {"kernel": 2}, {"split": 0}, {"micro": 0}, {"micro": 2}, {"micro": 2, "kernel": 1},
          {"micro": 0, "split": 0}, {"cus": 304}, {"cus": 128}, {"cus": 304, "micro": 2}, {"cus": 128, "micro": 0},
          {"lds": SMALL_LDS}, {"lds": SMALL_LDS, "kernel": 1}, {"lds": SMALL_LDS, "kernel": 2}, {"lds": SMALL_LDS, "micro": 2}, {"lds": 96 * 1024}]
COLUMNS = ("rc", "family", "mtm", "split", "workgroups", "lds_bytes", "tiles_per_env", "mc_w", "mc_hi", "mc_r", "exchange_bytes",
           "publish", "zero")


def group_key(group):
    return group[0]


def requests(full):
    """The rows of one group, in iteration order: (m, n, h, request, policy)."""
    return list(itertools.product(M if full else EDGE_M, N if full else EDGE_N, H, REQUEST, POLICY))


def policy_ints(policy):
    return [policy.get("kernel", 0), policy.get("split", -1), policy.get("micro", -1), policy.get("cus", 0), policy.get("lds", 0)]


def group_rows(lib, group, reqs):
    """int32 [len(reqs), 13]: rc and the 12 ints of every request of the group."""
    _, obs_dim, act_dim, units, cell, _ = group
    layers = [units] if isinstance(units, int) else units
    arr = (ctypes.c_int * len(layers))(*layers)
    n_layers = 0 if isinstance(units, int) else len(layers)
    pol = (ctypes.c_int * 5)()
    out = (ctypes.c_int * 12)()
    rows = np.zeros((len(reqs), 13), dtype=np.int32)
    cell_code = _lib.CELL_CODES[cell]
    for i, (m, n, h, request, policy) in enumerate(reqs):
        pol[:] = policy_ints(policy)
        rc = lib.l2a_lstm_plan_geometry(obs_dim, act_dim, n_layers, arr, cell_code, m, n, h, request, pol, out)
        rows[i, 0] = rc
        if rc == _lib.L2A_OK:
            rows[i, 1:] = out[:]
    return rows


def class_key(row):
    rc, family, mtm, split, _, _, _, _, mc_hi, _, xbytes, publish, _ = (int(x) for x in row)
    return (rc, family, mtm, split, mc_hi, int(xbytes > 0), publish)


def compute(lib=None):
    """{group key: rows} in iteration order, for the committed grid."""
    lib = lib or _lib.load()
    reqs = {True: requests(True), False: requests(False)}
    return {group_key(g): group_rows(lib, g, reqs[g[5]]) for g in groups()}


def histogram(tables):
    hist = {}
    for rows in tables.values():
        uniq, cnt = np.unique(rows, axis=0, return_counts=True)
        for r, c in zip(uniq, cnt):
            k = " ".join(str(x) for x in class_key(r))
            hist[k] = hist.get(k, 0) + int(c)
    return dict(sorted(hist.items()))


def digest(tables):
    whole = 0
    for rows in tables.values():
        whole = zlib.crc32(rows.tobytes(), whole)
    return {"columns": list(COLUMNS), "calls": int(sum(len(r) for r in tables.values())), "crc32": whole,
            "class_key": "rc family mtm split mc_hi exchange_bytes>0 publish",
            "histogram": histogram(tables),
            "groups": {k: zlib.crc32(rows.tobytes()) for k, rows in tables.items()}}


def pack_rows(tables):
    """Every group's rows in iteration order, one column after the other (the columns repeat themselves)."""
    return lzma.compress(np.ascontiguousarray(np.concatenate(list(tables.values())).T).tobytes(), preset=9)


def stored_rows():
    """{group key: rows} as committed in ROWS."""
    with open(ROWS, "rb") as f:
        a = np.frombuffer(lzma.decompress(f.read()), dtype=np.int32).reshape(len(COLUMNS), -1).T
    out, at = {}, 0
    for g in groups():
        per = len(requests(g[5]))
        out[group_key(g)] = np.ascontiguousarray(a[at:at + per])
        at += per
    assert at == len(a)
    return out


if __name__ == "__main__":
    tables = compute()
    d = digest(tables)
    with open(TABLE, "w") as f:
        json.dump(d, f, indent=0, sort_keys=False)
        f.write("\n")
    with open(ROWS, "wb") as f:
        f.write(pack_rows(tables))
    print("%s + %s: %d calls, %d failing, %d classes, crc32 %d, %d + %d bytes" % (
        TABLE, ROWS, d["calls"], sum(c for k, c in d["histogram"].items() if not k.startswith("0 ")), len(d["histogram"]), d["crc32"],
        os.path.getsize(TABLE), os.path.getsize(ROWS)))
