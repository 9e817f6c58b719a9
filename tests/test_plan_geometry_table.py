"""The launch geometry of the MLP rollout over a grid of shapes, plans and policies, against the committed table
(tests/plan_geometry_table.json and the rows in tests/golden/plan_geometry_rows.xz, written by
tools/gen_plan_geometry_table.py: grid, row layout and class key are defined there).  `l2a_plan_geometry` projects the plan
`plan_rollout` decides and `launch_rollout` executes, so a row that changes here is a launch that changes.  No GPU needed; the
whole grid (338 184 calls) takes a few seconds."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_plan_geometry_table as gen  # noqa: E402

from learning_to_adapt_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def committed():
    with open(gen.TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return gen.compute()


def _describe(key, i, old, new):
    m, n, h, policy = gen.requests()[i]
    cols = [c for c, a, b in zip(gen.COLUMNS, old, new) if a != b]
    return ("group %s, row %d (m = %d, n = %d, h = %d, policy %s) differs in %s:\n  committed %s\n  computed  %s"
            % (key, i, m, n, h, policy, cols, dict(zip(gen.COLUMNS, old.tolist())), dict(zip(gen.COLUMNS, new.tolist()))))


def test_every_group_matches_the_committed_table(committed, computed):
    assert list(computed) == list(committed["groups"]) and len(computed) == 126
    stored = gen.stored_rows()
    for key, rows in computed.items():
        old = stored[key]
        assert gen.zlib.crc32(old.tobytes()) == committed["groups"][key], key      # the stored rows are the digested ones
        if gen.zlib.crc32(rows.tobytes()) != committed["groups"][key]:
            assert old.shape == rows.shape, (key, old.shape, rows.shape)
            i = int(np.flatnonzero((old != rows).any(axis=1))[0])
            pytest.fail(_describe(key, i, old[i], rows[i]))
    d = gen.digest(computed)
    assert d["calls"] == committed["calls"] == 338184
    assert d["crc32"] == committed["crc32"]


def test_histogram_matches_and_no_call_fails(committed, computed):
    hist = gen.histogram(computed)
    print(json.dumps(hist, indent=0))
    assert hist == committed["histogram"]
    assert all(k.split()[0] == str(_lib.L2A_OK) for k in hist), [k for k in hist if k.split()[0] != str(_lib.L2A_OK)]
    assert len(hist) >= 60
    for rows in computed.values():
        assert not rows[:, 0].any()


def test_per_block_needs_a_set_per_env():
    hid = (gen.ctypes.c_int * 2)(512, 512)
    out = (gen.ctypes.c_int * 12)()
    rc = _lib.load().l2a_plan_geometry(20, 6, 2, hid, 5, _lib.MODE_CODES["per_block"], 10, 100, 30, None, out)
    assert rc == _lib.L2A_EINVAL
