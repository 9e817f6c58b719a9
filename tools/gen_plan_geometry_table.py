#!/usr/bin/env python
"""The launch geometry of the MLP rollout over a grid of shapes, plans and policies (``l2a_plan_geometry``: no GPU needed),
digested into tests/plan_geometry_table.json - which tests/test_plan_geometry_table.py recomputes and compares.  A geometry
change shows there as a changed group; regenerate the file with this tool only when the change is meant:

    python tools/gen_plan_geometry_table.py            # rewrites both files

Per row: the return code and the 12 ints of the call (zeros when it fails).  The file holds, per (shape, hidden, sets) group,
the CRC-32 of the group's int32 rows in iteration order, and a histogram over the rows' classes.  The rows themselves go,
column by column and xz-compressed (24 KB), to tests/golden/plan_geometry_rows.xz, so that a mismatch can be named row by row."""
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
from learning_to_adapt_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "plan_geometry_table.json")
ROWS = os.path.join(ROOT, "tests", "golden", "plan_geometry_rows.xz")

SHAPES = [(20, 6), (41, 8), (64, 16)]                       # (obs_dim, act_dim)
HIDDEN = [[128, 128], [256, 256], [512], [512, 512], [512, 512, 512], [200, 72]]
SETS = [(1, "single"), (2, "mean"), (3, "mean"), (5, "mean"), (8, "mean"), (9, "mean"), (5, "per_block")]
M = [1, 5]
N = list(range(1, 34)) + [96, 127, 128, 129, 255, 256, 257, 300, 368, 500, 512, 816, 817, 1000, 1024, 1632, 1633,
                          2000, 2500, 4000, 4080, 4096, 4097, 8000, 8176, 8192, 16000, 20000]
H = [30, 4096]
# the arguments of _lib.plan_geometry that differ from the defaults (-1 for split, fan, micro, double; 0 for cus)
POLICY = [{}, {"split": 0}, {"split": 2}, {"fan": 0}, {"micro": 0}, {"micro": 2}, {"double": 0}, {"cus": 128}, {"cus": 304},
          {"micro": 0, "double": 0}, {"split": 0, "double": 0, "micro": 0}]
COLUMNS = ("rc", "kind", "nt", "split", "split_from", "fan", "workgroups", "lds_bytes", "sets_per_batch", "micro_tiles",
           "placement_units", "front_workgroups", "whole_instance")


def groups(shapes=SHAPES, hidden=HIDDEN, sets=SETS):
    return list(itertools.product(shapes, hidden, sets))


def group_key(group):
    (obs_dim, act_dim), hidden, (n_sets, mode) = group
    return "%dx%d|%s|%d %s" % (obs_dim, act_dim, "-".join(str(x) for x in hidden), n_sets, mode)


def requests(ms=M, ns=N, hs=H, policies=POLICY):
    """The rows of one group, in iteration order: (m, n, h, policy)."""
    return list(itertools.product(ms, ns, hs, policies))


def group_rows(lib, group, reqs):
    """int32 [len(reqs), 13]: rc and the 12 ints of every request of the group."""
    (obs_dim, act_dim), hidden, (n_sets, mode) = group
    hid = (ctypes.c_int * len(hidden))(*hidden)
    pol = (ctypes.c_int * 5)()
    out = (ctypes.c_int * 12)()
    rows = np.zeros((len(reqs), 13), dtype=np.int32)
    mode_code = _lib.MODE_CODES[mode]
    for i, (m, n, h, policy) in enumerate(reqs):
        pol[:] = [policy.get("split", -1), policy.get("fan", -1), policy.get("micro", -1), policy.get("cus", 0), policy.get("double", -1)]
        rc = lib.l2a_plan_geometry(obs_dim, act_dim, len(hidden), hid, n_sets, mode_code, m, n, h, pol, out)
        rows[i, 0] = rc
        if rc == _lib.L2A_OK:
            rows[i, 1:] = out[:]
    return rows


def class_key(row):
    rc, kind, nt, split, split_from, fan, _, _, lb, micro_tiles, pl_units, front, whole = (int(x) for x in row)
    return (rc, kind, nt, split, fan, int(split_from >= 0), int(front > 0), whole, int(micro_tiles > 0), lb, pl_units)


def compute():
    """{group key: rows} in iteration order, for the committed grid."""
    lib = _lib.load()
    reqs = requests()
    return {group_key(g): group_rows(lib, g, reqs) for g in groups()}


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
            "class_key": "rc kind nt split fan split_from>=0 front_workgroups>0 whole_instance micro_tiles>0 sets_per_batch placement_units",
            "histogram": histogram(tables),
            "groups": {k: zlib.crc32(rows.tobytes()) for k, rows in tables.items()}}


def pack_rows(tables):
    """Every group's rows in iteration order, one column after the other (the columns repeat themselves: 17 MB -> 24 KB)."""
    return lzma.compress(np.ascontiguousarray(np.concatenate(list(tables.values())).T).tobytes(), preset=9)


def stored_rows():
    """{group key: rows} as committed in ROWS."""
    with open(ROWS, "rb") as f:
        a = np.frombuffer(lzma.decompress(f.read()), dtype=np.int32).reshape(len(COLUMNS), -1).T
    per = len(requests())
    return {group_key(g): np.ascontiguousarray(a[i * per:(i + 1) * per]) for i, g in enumerate(groups())}


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
