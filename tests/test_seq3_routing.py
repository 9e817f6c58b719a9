"""Which plans the launcher sends to the static three-set-step instances of the MFMA rollout kernel (csrc/l2a_mfma.h SEQ3;
`l2a_set_seq3`), read from the launcher's own decision code without a GPU (`_lib.plan_geometry`): a mean ensemble of five
2 x 512 sets of up to 32 inputs under the shared-set tile split - every workgroup then runs full, full, shared in one batch -
and nothing else.  The switch selects instances only: the six geometry fields the other routing tests compare are the same
with it on and off."""

import pytest

from learning_to_adapt_amd import _lib

FIELDS = ("kernel", "nt", "split", "fan", "whole_instance", "front_workgroups")
HC = dict(obs_dim=20, act_dim=6, hidden=[512, 512], n_sets=5, mode="mean", m=1, h=30)


def _geo(**over):
    kw = dict(HC, **over)
    return _lib.plan_geometry(kw.pop("obs_dim"), kw.pop("act_dim"), kw.pop("hidden"), kw.pop("n_sets"), kw.pop("mode"),
                              kw.pop("m"), kw.pop("n"), kw.pop("h"), **kw)


def _same_fields(over):
    on, off = _geo(seq3=1, **over), _geo(seq3=0, **over)
    assert not off["seq3"]
    assert [on[f] for f in FIELDS] == [off[f] for f in FIELDS], (over, on, off)
    assert _geo(**over) == on                       # the default is on
    return on


# n = 16 and 40 are one and three candidate tiles: with the member fan on such a plan is the fan's (5 x tiles <= CUs), so the
# tile split - and with it the static step - is reached with the fan off; 2000 and 2048 (128 tiles = 256 workgroups, the last
# that fits 256 CUs) under every default
@pytest.mark.parametrize("over", [dict(n=16, fan=0), dict(n=40, fan=0), dict(n=2000), dict(n=2048), dict(n=2000, split=1)],
                         ids=lambda o: "-".join("%s=%s" % kv for kv in sorted(o.items())))
def test_static_step_is_reported_for_the_five_set_tile_split(over):
    g = _same_fields(over)
    assert g["seq3"], g
    assert (g["kernel"], g["nt"], g["split"], g["split_from"], g["fan"], g["sets_per_batch"]) == ("mfma16", 1, 2, -1, False, 3), g


def test_small_plans_with_the_fan_on_are_the_fans():
    for n in (16, 40, 500):
        g = _same_fields(dict(n=n))
        assert g["fan"] and g["split"] == 3 and not g["seq3"], (n, g)


NOT_STATIC = [
    dict(n=2000, n_sets=1, mode="single"), dict(n=2000, n_sets=3), dict(n=2000, n_sets=4), dict(n=2000, n_sets=7),
    dict(n=40, fan=0, n_sets=3), dict(n=40, fan=0, n_sets=4), dict(n=40, fan=0, n_sets=7), dict(n=40, fan=0, n_sets=1, mode="single"),
    dict(n=2000, hidden=[512, 512, 512]), dict(n=2000, hidden=[512]),
    dict(n=2000, hidden=[128, 128]), dict(n=2000, hidden=[256, 256]),
    dict(n=2000, obs_dim=41, act_dim=8),            # Ant: 49 inputs, four input k-groups
    dict(n=2000, split=0), dict(n=2000, split=2),
    dict(n=2000, batch=1), dict(n=2000, batch=2),
    dict(n=400, m=5, mode="per_block"),             # per-block sets: one set per candidate
    dict(n=4800),                                   # 300 tiles: whole tiles + a tail split
    dict(n=500),                                    # the fan wins
    dict(n=2000, seq3=0),
]


@pytest.mark.parametrize("over", NOT_STATIC, ids=lambda o: "-".join("%s=%s" % (k, "x".join(map(str, v)) if isinstance(v, list) else v)
                                                                    for k, v in sorted(o.items())))
def test_static_step_is_not_reported(over):
    if "seq3" in over:
        g = _geo(**over)
    else:
        g = _same_fields(over)
    assert not g["seq3"], g


def test_what_the_neighbours_run_instead():
    assert _geo(n=4800)["split_from"] >= 0                                    # the tail split
    assert _geo(n=2000, batch=2)["sets_per_batch"] == 2 and _geo(n=2000, batch=1)["sets_per_batch"] == 1
    assert _geo(n=2000, split=2)["split"] == 1 and _geo(n=2000, split=0)["split"] == 0
    assert _geo(n=2000, n_sets=7)["sets_per_batch"] == 3                      # batches of 3 + 1: not one batch
    assert _geo(n=2000, n_sets=3, fan=0)["split"] == 2                        # full, shared: two sets (fan on: double-tile fan)
    assert not _geo(n=2000, n_sets=3, fan=0)["seq3"]


def test_counted_entry_point_and_the_twelve_int_one_agree():
    import ctypes
    lib = _lib.load()
    hid = (ctypes.c_int * 2)(512, 512)
    pol5 = (ctypes.c_int * 5)(-1, -1, -1, 0, -1)
    out12 = (ctypes.c_int * 13)(*([-7] * 13))
    out13 = (ctypes.c_int * 13)()
    assert lib.l2a_plan_geometry(20, 6, 2, hid, 5, _lib.MODE_CODES["mean"], 1, 2000, 30, pol5, out12) == _lib.L2A_OK
    assert lib.l2a_plan_geometry_ex(20, 6, 2, hid, 5, _lib.MODE_CODES["mean"], 1, 2000, 30, pol5, 5, out13, 13) == _lib.L2A_OK
    assert list(out12)[:12] == list(out13)[:12] and out12[12] == -7 and out13[12] == 1      # (twelve ints written, no more)
    assert lib.l2a_plan_geometry_ex(20, 6, 2, hid, 5, _lib.MODE_CODES["mean"], 1, 2000, 30, pol5, 8, out13, 13) != _lib.L2A_OK
    assert lib.l2a_plan_geometry_ex(20, 6, 2, hid, 5, _lib.MODE_CODES["mean"], 1, 2000, 30, pol5, 5, out13, 14) != _lib.L2A_OK
