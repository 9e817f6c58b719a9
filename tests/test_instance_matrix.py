"""The instance matrix (tests/instance_matrix.py) against the launcher's own routing code, without a GPU.

(a) every MLP row, under its policy, is routed (`l2a_plan_geometry`: launch_rollout stopped before its first HIP call) to the
    unit its instance lives in, and the unit's switch (restated in `instance_matrix.dispatched_instance`) picks that instance;
(b) the rows cover the literal enumeration of instances minus the explicit UNREACHABLE list - removing a row, or changing a
    policy so that it routes elsewhere, fails here;
(c) the GPU file runs every row: no row is skipped, deselected by a mark or expected to fail.
"""

import ctypes
import re

import pytest

import instance_matrix as im
from learning_to_adapt_amd import _lib

GEOMETRY_FIELDS = ("kernel", "nt", "split", "fan", "whole_instance", "front_workgroups")


def _geometry(row):
    p = row.policy
    return _lib.plan_geometry(row.obs_dim, row.act_dim, row.hidden, row.E, row.mode, row.m, row.n, row.h,
                              split=p["split"], fan=p["fan"], micro=p["micro"], cus=256, double=p["double"])


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
    """The LSTM launcher has no dry run; the conditions its routing relies on (l2a_lstm_api.hip) are arithmetic on the row."""
    for row in im.LSTM_ROWS:
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


def test_gpu_file_runs_every_row():
    import test_gpu_instance_matrix as gpu
    for fn, rows in ((gpu.test_mlp_instance_matches_oracle, im.MLP_ROWS), (gpu.test_lstm_instance_matches_oracle, im.LSTM_ROWS)):
        marks = [m for m in fn.pytestmark]
        assert [m.name for m in marks] == ["parametrize"], marks             # no skip / xfail mark on the test
        args = marks[0].args[1]
        assert list(args) == list(rows) and all(isinstance(a, im.Row) for a in args)    # plain rows: no marked parameter
        assert list(marks[0].kwargs["ids"]) == [r.id for r in rows]
    assert [m.name for m in gpu.pytestmark] == ["gpu"] if isinstance(gpu.pytestmark, list) else gpu.pytestmark.name == "gpu"
