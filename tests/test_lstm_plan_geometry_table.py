"""The launch of the recurrent launcher over a grid of models, requests and policies, against the committed table
(tests/lstm_plan_geometry_table.json and the rows in tests/golden/lstm_plan_geometry_rows.xz, written by
tools/gen_lstm_plan_geometry_table.py: grid, row layout and class key are defined there).  `l2a_lstm_plan_geometry` projects the
plan `plan_rnn_launch` decides and `launch()` / `rollout_traj()` execute, so a row that changes here is a launch that changes.
The committed rows were recorded from the launcher as it was before the plan function existed (a record-and-return in front of
each of its seven launch sites).  No GPU needed; the whole grid takes a few seconds.

Further down: the geometries the docstrings of tests/test_rnn.py name, each derived here from the plan's arithmetic."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lstm_plan_geometry_table as gen  # noqa: E402

from learning_to_adapt_amd import _lib  # noqa: E402

CALLS = 394128
COL = {c: i for i, c in enumerate(gen.COLUMNS)}


@pytest.fixture(scope="module")
def committed():
    with open(gen.TABLE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return gen.compute()


def _describe(key, full, i, old, new):
    m, n, h, request, policy = gen.requests(full)[i]
    cols = [c for c, a, b in zip(gen.COLUMNS, old, new) if a != b]
    return ("group %s, row %d (m = %d, n = %d, h = %d, request %d, policy %s) differs in %s:\n  committed %s\n  computed  %s"
            % (key, i, m, n, h, request, policy, cols, dict(zip(gen.COLUMNS, old.tolist())), dict(zip(gen.COLUMNS, new.tolist()))))


def test_every_group_matches_the_committed_table(committed, computed):
    full = {g[0]: g[5] for g in gen.groups()}
    assert list(computed) == list(committed["groups"]) == list(full)
    stored = gen.stored_rows()
    for key, rows in computed.items():
        old = stored[key]
        assert gen.zlib.crc32(old.tobytes()) == committed["groups"][key], key      # the stored rows are the digested ones
        if gen.zlib.crc32(rows.tobytes()) != committed["groups"][key]:
            assert old.shape == rows.shape, (key, old.shape, rows.shape)
            i = int(np.flatnonzero((old != rows).any(axis=1))[0])
            pytest.fail(_describe(key, full[key], i, old[i], rows[i]))
    d = gen.digest(computed)
    assert d["calls"] == committed["calls"] == CALLS >= 100000
    assert d["crc32"] == committed["crc32"]


def test_histogram_matches(committed, computed):
    hist = gen.histogram(computed)
    print(json.dumps(hist, indent=0))
    assert hist == committed["histogram"]


def _select(computed, key, **where):
    """The rows of group `key` whose request matches `where` (m, n, h, request, or a policy dict)."""
    full = {g[0]: g[5] for g in gen.groups()}[key]
    names = ("m", "n", "h", "request", "policy")
    idx = [i for i, rq in enumerate(gen.requests(full)) if all(rq[names.index(k)] == v for k, v in where.items())]
    assert idx, (key, where)
    return computed[key][idx]


def test_the_grid_reaches_what_it_must(computed):
    a = np.concatenate(list(computed.values()))
    ok = a[a[:, 0] == _lib.L2A_OK]
    fam, mtm, wg = ok[:, COL["family"]], ok[:, COL["mtm"]], ok[:, COL["workgroups"]]
    assert sorted(set(fam.tolist())) == list(range(7))                                  # every family
    micro = fam == _lib.LSTM_FAMILIES.index("generic_micro")
    assert (micro & (mtm == 3)).any()
    # workgroups of four micro tiles: in one round (at most 304 workgroups: the largest CU count of the grid), and in several
    assert (micro & (mtm == 4) & (wg <= 128)).any() and (micro & (mtm == 4) & (wg > 304)).any()
    mfma16 = fam == _lib.LSTM_FAMILIES.index("lstm_mfma16")
    assert (mfma16 & (ok[:, COL["split"]] == 1) & (ok[:, COL["exchange_bytes"]] > 0)).any() and (mfma16 & (ok[:, COL["split"]] == 0)).any()
    assert {p.get("kernel", 0) for p in gen.POLICY} == {0, 1, 2} and {p.get("split", 1) for p in gen.POLICY} == {0, 1}
    assert {p.get("micro", 1) for p in gen.POLICY} == {0, 1, 2} and {p.get("cus", 256) for p in gen.POLICY} >= {128, 256, 304}
    bits = 0
    for r in gen.REQUEST:
        bits |= r
    assert bits == 31 and 0 in gen.REQUEST
    # every error return of plan_rnn_launch, each on a request nothing else can fail
    fails = lambda rows: bool((rows[:, 0] == _lib.L2A_EINVAL).all())  # noqa: E731
    small = gen.SMALL_LDS
    assert fails(_select(computed, "20x6|gru|256x256", policy={"lds": small, "kernel": 1}))       # the matrix-core recurrent kernel's LDS
    assert fails(_select(computed, "20x6|gru|400x400x400", policy={"kernel": 2}))                 # the generic recurrent kernel's LDS
    assert fails(_select(computed, "20x6|lstm|create100", policy={"kernel": 1}))                  # not eligible for the MFMA kernel
    assert fails(_select(computed, "20x6|lstm|512", policy={"lds": small, "kernel": 1}, request=2))     # the tuned kernel's LDS (a state written out: no micro tiles)
    assert fails(_select(computed, "20x6|lstm|create1024", policy={}))                            # the VALU LSTM kernel's LDS
    # the fallbacks under the small LDS: the stack's matrix-core rows no longer fit, the VALU kernel's dense rows do
    rows = _select(computed, "64x16|gru|256", policy={"lds": small}, request=0)
    assert (rows[:, COL["family"]] == _lib.LSTM_FAMILIES.index("generic_valu")).all() and not rows[:, COL["publish"]].any()
    # the `publish` exception: three 256-unit LSTM layers take micro tiles and do not publish
    rows = _select(computed, "20x6|lstm|256x256x256", policy={}, request=0, m=5, n=500)
    assert (rows[:, COL["family"]] == _lib.LSTM_FAMILIES.index("generic_micro")).all() and not rows[:, COL["publish"]].any()


# ---- the geometries tests/test_rnn.py names in its docstrings ------------------------------------------------------------------

def _deal(cus, m, n, max_hi):
    """Workgroups per env, micro tiles of the largest, for ceil(n / 4) micro tiles dealt to at most cus // m workgroups."""
    quads = -(-n // 4)
    w = min(cus // m, quads)
    hi = -(-quads // w)
    if hi > max_hi:
        return w, hi
    w = -(-quads // hi)
    return w, -(-quads // w)


def test_gru_stack_of_3500_candidates_runs_four_micro_tiles_per_workgroup_in_one_round():
    """875 micro tiles on 256 CUs are four per workgroup: 219 workgroups, one round."""
    assert _deal(256, 1, 3500, 3)[1] == 4
    g = _lib.lstm_plan_geometry(20, 6, [256, 256], "gru", 1, 3500, 10, cus=256)
    assert -(-875 // 4) == 219
    assert (g["family"], g["mtm"], g["workgroups"], g["mc_hi"], g["mc_r"]) == ("generic_micro", 4, 219, 4, 875 - 219 * 3)
    assert g["workgroups"] <= 256 and not g["split"] and g["publish"]


def test_gru_of_16000_candidates_runs_four_micro_tiles_per_workgroup_in_several_rounds():
    g = _lib.lstm_plan_geometry(20, 6, [256], "gru", 1, 16000, 10, cus=256)
    assert (g["family"], g["mtm"], g["workgroups"], g["mc_hi"], g["mc_r"]) == ("generic_micro", 4, 1000, 4, 1000)
    assert g["workgroups"] > 3 * 256


def test_lstm_of_64_envs_by_12_candidates_under_policy_2():
    """64 envs leave 256 // 64 = 4 workgroups per env; 12 candidates are three micro tiles, one per workgroup on three of them:
    at most three per workgroup, so under policy 2 the plan TAKES micro tiles, 192 workgroups (tests/test_rnn.py used to call
    this case a fall-back; nothing in the launcher ever made it one).  With one more env than CUs there is no workgroup per env
    left and the plan does fall back."""
    assert _deal(256, 64, 12, 3) == (3, 1)
    g = _lib.lstm_plan_geometry(20, 6, [256], "lstm", 64, 12, 2, micro=2, cus=256)
    assert (g["family"], g["workgroups"], g["mc_w"], g["mc_hi"], g["mc_r"]) == ("lstm_micro", 64 * 3, 3, 1, 3)
    assert 256 // 257 == 0
    g = _lib.lstm_plan_geometry(20, 6, [256], "lstm", 257, 12, 2, micro=2, cus=256)
    assert (g["family"], g["mc_w"], g["workgroups"]) == ("lstm_mfma16", 0, 257)


def test_rebal_default_takes_micro_tiles_on_5_by_42_workgroups():
    """256 units, m = 5, n = 500 under policy 1: 5 x 32 = 160 16-candidate tiles leave 96 of 256 CUs idle and are too many for the
    unit-tile split; 125 micro tiles per env on 51 workgroups are three each, which 42 workgroups hold as well."""
    tiles = 5 * -(-500 // 16)
    assert 2 * tiles > 256 > tiles
    assert _deal(256, 5, 500, 3) == (42, 3) and 256 // 5 == 51
    g = _lib.lstm_plan_geometry(20, 6, [256], "lstm", 5, 500, 10, micro=1, cus=256)
    assert (g["family"], g["workgroups"], g["mc_w"], g["mc_hi"], g["mc_r"]) == ("lstm_micro", 5 * 42, 42, 3, 125 - 42 * 2)
    assert g["publish"] and g["lds_bytes"] >= 84 * 1024
