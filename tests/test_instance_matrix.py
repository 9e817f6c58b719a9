"""The instance matrix (tests/instance_matrix.py) against the launcher's own routing code, without a GPU.

(a) every MLP row, under its policy, is routed (`l2a_plan_geometry`: the plan `plan_rollout` decides and launch_rollout executes) to the
    unit its instance lives in, and the unit's switch (restated in `instance_matrix.dispatched_instance`) picks that instance;
(b) the rows cover the literal enumeration of instances minus the explicit UNREACHABLE list - removing a row, or changing a
    policy so that it routes elsewhere, fails here;
(c) the GPU file runs every row: no row is skipped, deselected by a mark or expected to fail;
(d) the carry launches of a row (tests/test_gpu_instance_matrix.py: a chunk of one horizon step, a chunk of two, a predict)
    take the geometry of the row's plan: the launcher's decision does not look at h below 4096, and with m = 1 a predict of
    the row's n rows is a plan of h = 1;
(e) GENERIC_ROWS reaches every run-time branch of the generic recurrent kernel it claims, and its oracle stays finite.
"""

import ctypes
import re

import pytest

import instance_matrix as im
from learning_to_adapt_amd import _lib

GEOMETRY_FIELDS = ("kernel", "nt", "split", "fan", "whole_instance", "front_workgroups")


def _geometry(row, h=None, micro=None):
    p = row.policy
    return _lib.plan_geometry(row.obs_dim, row.act_dim, row.hidden, row.E, row.mode, row.m, row.n, row.h if h is None else h,
                              split=p["split"], fan=p["fan"], micro=p["micro"] if micro is None else micro, cus=256,
                              double=p["double"])


def _unit_of(row, g):
    """The translation unit whose launcher `l2a_launch_mfma` (l2a_mfma_launch.h) / `l2a_launch_mlp_micro` calls for a geometry."""
    width = row.hidden[0]
    if g["kernel"] == "micro":
        return "mlp_micro", "uw%d" % (width // 256)
    assert g["kernel"] == "mfma16"
    if g["front_workgroups"]:           # the described launch is the rest behind the double tiles of whole_2_8
        assert width == 512 and g["whole_instance"] and g["nt"] == 1
        return "mlp", "whole_2_8"
    geo = 1 if g["fan"] else 2 if g["whole_instance"] else 0
    units = [u for u, v in im.MFMA_UNITS.items() if v == (g["nt"], width, geo)]
    assert len(units) == 1, (row.id, g)
    return "mlp", units[0]


@pytest.mark.parametrize("row", im.MLP_ROWS, ids=[r.id for r in im.MLP_ROWS])
def test_row_routes_to_its_instance(row):
    hid = (ctypes.c_int * len(row.hidden))(*row.hidden)
    assert _lib.load().l2a_mfma_eligible(row.obs_dim, row.act_dim, len(row.hidden), hid) == 1
    g = _geometry(row)
    assert {k: g[k] for k in GEOMETRY_FIELDS} == row.expect, row.id
    family, unit = _unit_of(row, g)
    if family == "mlp_micro":           # l2a_api.hip: gact_m
        gact = row.activation not in ("relu", "identity") or len(row.hidden) == 1
        assert im.Instance(family, unit, 0, 0, "", gact, False) == row.instance
    else:
        assert im.dispatched_instance(family, unit, row.obs_dim, row.act_dim, len(row.hidden), row.activation) == row.instance
    assert row.h == 3 and row.m == 1


CARRY_MLP_ROWS = [r for r in im.MLP_ROWS if r.instance.family == "mlp"]


@pytest.mark.parametrize("row", CARRY_MLP_ROWS, ids=[r.id for r in CARRY_MLP_ROWS])
def test_carry_launches_route_to_the_rows_instance(row):
    """Chunk A is a launch of h = 1, chunk B one of h = 2, and the predict (every row has m = 1: n rows in one block) is
    h = 1 again (l2a_api.hip: l2a_predict), all with micro = 0: the launcher must pick the geometry of the row's own plan - and
    with it, by (a), the row's instance.  (A launch with per-row states or a state output never takes the micro tiles whatever the
    policy says: l2a_api.hip:297.)"""
    assert row.m == 1
    for h in (1, 2):
        g = _geometry(row, h=h, micro=0)
        assert {k: g[k] for k in GEOMETRY_FIELDS} == row.expect, (row.id, h)
        assert _unit_of(row, g) == ("mlp", row.instance.unit)


def test_rows_cover_every_compiled_instance():
    assert len(set(im.ENUMERATED)) == len(im.ENUMERATED)
    assert set(im.UNREACHABLE) <= set(im.ENUMERATED)
    covered = {r.instance for r in im.ROWS}
    missing = set(im.ENUMERATED) - set(im.UNREACHABLE) - covered
    extra = covered - (set(im.ENUMERATED) - set(im.UNREACHABLE))
    assert not missing and not extra, (sorted(missing), sorted(extra))
    assert len({r.id for r in im.ROWS}) == len(im.ROWS)
    # the counts DESIGN.md quotes
    fam = lambda f: sum(1 for i in im.COMPILED if i.family == f)  # noqa: E731
    assert (fam("mlp"), fam("mlp_micro"), fam("lstm"), fam("lstm_micro")) == (267, 4, 48, 2)


def test_unreachable_list_matches_the_launcher_and_the_sources():
    """Each entry quotes the condition that excludes it; the launcher agrees (OT = 4 never reports the whole-tiles instance;
    the LSTM / micro families have none), and l2a_mfma_inst.hip carries the two guards that keep the entries out of the build."""
    assert len(im.UNREACHABLE) == 6 + len(im.MFMA_UNITS)
    assert all(re.match(r"l2a_(api|mfma_inst)\.hip:\d+", why) for why in im.UNREACHABLE.values())
    for od, ad in ((49, 15), (64, 1), (64, 16)):
        for depth in (1, 2):
            g = _lib.plan_geometry(od, ad, [512] * depth, 1, "single", 1, im.N_SMALL, im.H, split=0, fan=0, micro=0, cus=256, double=1)
            assert g["kernel"] == "mfma16" and g["nt"] == 1 and not g["whole_instance"]
    # K0L = 1 with a generic activation: the switch itself, restated
    assert im.dispatched_instance("mlp", "1_4", 41, 8, 2, "tanh").variant == ""


def test_lstm_rows_meet_the_launcher_conditions():
    """Every LSTM row reaches its instance - the family, and split on or off, at 256 CUs - by the launcher's own plan
    (`plan_rnn_launch`, asked through `lstm_plan_geometry`); the conditions that plan relies on, restated as arithmetic on the row."""
    for row in im.LSTM_ROWS:
        g = _lib.lstm_plan_geometry(row.obs_dim, row.act_dim, [row.hidden], "lstm", row.m, row.n, row.h, split=row.policy["split"],
                                    micro=row.policy["micro"], cus=256)
        if row.instance.family == "lstm_micro":
            assert (g["family"], g["split"], g["mtm"]) == ("lstm_micro", 0, 3), row.id
        else:
            assert (g["family"], g["split"]) == ("lstm_mfma16", 1 if row.instance.variant == "split" else 0), row.id
            assert g["workgroups"] == 3 * (1 + g["split"]) and (g["exchange_bytes"] > 0) == bool(g["split"]), row.id
            # the carry launches (chunks of h = 1 and 2 with a state output, the second with per-row states; a predict of n rows)
            for h, request in ((1, ("state_out",)), (2, ("per_row", "state_out")), (1, ("per_row", "state_out"))):
                c = _lib.lstm_plan_geometry(row.obs_dim, row.act_dim, [row.hidden], "lstm", row.m, row.n, h, request=request,
                                            split=row.policy["split"], micro=0, cus=256)
                assert (c["family"], c["split"], c["workgroups"]) == (g["family"], g["split"], g["workgroups"]), (row.id, h)
        tiles = row.m * ((row.n + 15) // 16)
        quads = (row.n + 3) // 4
        assert row.hidden in (128, 256, 512) and row.obs_dim <= 64 and row.act_dim <= 16
        assert (row.instance.ot, row.instance.kg0) == ((row.obs_dim + 15) // 16, (row.obs_dim + row.act_dim + 15) // 16) \
            or row.instance.family == "lstm_micro"
        if row.instance.family == "lstm_micro":
            assert row.policy["micro"] == 2 and row.hidden in (256, 512) and -(-quads // min(256 // row.m, quads)) <= 3
        else:
            assert row.policy["micro"] == 0
            assert row.policy["split"] == (1 if row.instance.variant == "split" else 0)
            assert 2 * tiles <= 256 and row.h < 4096
            # The carry launches take the same branch: the unit-tile split reads only the tile count, the split policy
            # and h < 4096 (chunks of h = 1 and 2 over the same m, n; l2a_lstm_predict is m = 1, n = rows, h = 1 with the default
            # `allow_split`), and `plan_only` keeps every launch with per-row states or a state output off the micro tiles.
            assert row.m == 1           # so a predict of m * n rows is the plan's own tile count


def test_gpu_file_runs_every_row():
    import test_gpu_instance_matrix as gpu
    for fn, rows in ((gpu.test_mlp_instance_matches_oracle, im.MLP_ROWS), (gpu.test_lstm_instance_matches_oracle, im.LSTM_ROWS)):
        marks = [m for m in fn.pytestmark]
        assert [m.name for m in marks] == ["parametrize"], marks             # no skip / xfail mark on the test
        args = marks[0].args[1]
        assert list(args) == list(rows) and all(isinstance(a, im.Row) for a in args)    # plain rows: no marked parameter
        assert list(marks[0].kwargs["ids"]) == [r.id for r in rows]
    assert [m.name for m in gpu.pytestmark] == ["gpu"] if isinstance(gpu.pytestmark, list) else gpu.pytestmark.name == "gpu"


def test_gpu_file_runs_the_carry_of_every_row_that_has_one():
    """The carry checks live inside the two row tests (the row's case is warm there), behind `has_carry`: true for every row
    but the micro-tile ones, whose kernels the launcher never gives a carry launch."""
    import inspect
    import test_gpu_instance_matrix as gpu
    for row in im.ROWS:
        assert gpu.has_carry(row) == (row.instance.family not in ("mlp_micro", "lstm_micro")), row.id
    assert sum(gpu.has_carry(r) for r in im.MLP_ROWS) == len(CARRY_MLP_ROWS) > 0
    for fn, carry in ((gpu.test_mlp_instance_matches_oracle, "_mlp_carry"), (gpu.test_lstm_instance_matches_oracle, "_lstm_carry")):
        src = inspect.getsource(fn)
        assert "if has_carry(row):" in src and src.count(carry + "(ctx, case, row, ") == 2 and "_check_chain(" in src


def test_gpu_file_runs_every_generic_row_on_both_kernels():
    import test_gpu_instance_matrix as gpu
    marks = {m.args[0]: m for m in gpu.test_generic_recurrent_branches_match_oracle.pytestmark}
    assert sorted(marks) == ["kernel", "row"] and all(m.name == "parametrize" for m in marks.values())
    assert list(marks["row"].args[1]) == list(im.GENERIC_ROWS) and list(marks["kernel"].args[1]) == ["mfma", "valu"]
    assert len({r.id for r in im.GENERIC_ROWS}) == len(im.GENERIC_ROWS)


def test_generic_rows_reach_the_branches_they_name():
    """The run-time switches of l2a_rnn_mfma.h, restated: unit tiles per product call (:306-308, :339-340), the operand ring's
    tail (:130-133) and clamp (:97), the action prefetch (:208), the observation tiles per wave (:380)."""
    rows = im.GENERIC_ROWS
    ut = lambda u: (u + 15) // 16  # noqa: E731
    for cell in ("gru", "rnn"):
        classes = {(1 if ut(u) < 8 else 2 if ut(u) < 16 else 4, ut(u) % 2) for r in rows if r.cell == cell for u in r.units}
        assert {(2, 0), (2, 1), (4, 1)} <= classes, (cell, classes)
    assert any(r.cell == "lstm" and len(r.units) > 1 and any(u % 4 for u in r.units) for r in rows)
    rings = [k for r in rows for k in im.generic_rings(r)[0]]
    assert {k % 4 for k in rings} == {0, 1, 2, 3} and 2 in rings
    assert any(im.generic_rings(r)[1] == 1 for r in rows)                        # an output layer of one k-group
    assert any(len(r.units) == 3 and len(set(r.units)) == 3 for r in rows)
    assert any(r.act_dim > 32 for r in rows) and any(r.obs_dim > 64 for r in rows)
    assert {"tanh", "relu", "sigmoid", "swish"} <= {r.activation for r in rows}
    assert all(re.match(r":\d+", r.why) for r in rows)


@pytest.mark.parametrize("row", im.GENERIC_ROWS, ids=[r.id for r in im.GENERIC_ROWS])
def test_generic_rows_keep_the_oracle_finite(row):
    import numpy as np
    import test_gpu_instance_matrix as gpu
    case = gpu._generic_oracle(row)
    for a in (case.want, case.states) + tuple(x for pair in case.cells for x in pair) + case.pred_want:
        assert np.all(np.isfinite(a)) and np.max(np.abs(a)) < 1e3, row.id
