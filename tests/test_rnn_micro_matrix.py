"""The table of the generic recurrent micro-tile kernel (tests/rnn_micro_matrix.py) against the sources and the launcher, without a GPU.

(a) `RNN_MICRO_ENUMERATED` is what csrc/l2a_rnn_micro_inst.hip instantiates and what the dispatch of csrc/l2a_rnn_micro.h
    branches to: a new instance fails here until it has rows;
(b) every row is routed (`l2a_lstm_plan_geometry`: the plan `plan_rnn_launch` decides and the launch executes) to its instance
    and deals workgroups of exactly the micro-tile counts the row names; the rows cover every pair but the UNREACHABLE ones
    (none: a grid of (m, n) is exhausted through the launcher - MT = 1 of the four-tile instances needs more envs than CUs);
(c) every input edge appears under every instance, every depth the launcher gives micro tiles appears, every n is ragged;
(d) the float64 oracle of every row is finite and separates each env's two best returns by MARGIN;
(e) the GPU file runs every row: none skipped, deselected by a mark or expected to fail.
"""

import os
import re

import numpy as np
import pytest

import rnn_micro_matrix as rm
from learning_to_adapt_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learning_to_adapt_amd", "csrc")
CELLS = {"L2A_CELL_LSTM": "lstm", "L2A_CELL_GRU": "gru", "L2A_CELL_RNN": "rnn"}


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _geometry(row, micro=2, cus=256, units=None, m=None, n=None):
    return _lib.lstm_plan_geometry(row.obs_dim, row.act_dim, list(row.units if units is None else units), row.cell,
                                   row.m if m is None else m, row.n if n is None else n, row.h, micro=micro, cus=cus)


def test_enumeration_matches_the_sources():
    inst = _source("l2a_rnn_micro_inst.hip")
    launched = re.findall(r"return launch_rnn<(\d+), (L2A_CELL_\w+), (\d+)>\(", inst)
    assert len(launched) == len(set(launched)) == 8
    assert [rm.Instance(int(uw), CELLS[cell], int(mtm)) for uw, cell, mtm in launched] == rm.INSTANCES
    # no other instantiation of the kernel: launch_rnn is its only user
    assert len(re.findall(r"l2a_rnn_micro_k<", inst)) == 1 and "l2a_rnn_micro_k<UW, CELL, MTM>" in inst
    # the width and mtm conditions in front of the instantiations
    assert re.findall(r"if \(units == (\d+) && mtm == (\d+)\)", inst) == [("256", "3"), ("256", "4"), ("512", "3")]

    kernel = _source("l2a_rnn_micro.h")
    kernel = kernel[kernel.index("__global__ void __launch_bounds__(256) l2a_rnn_micro_k("):]
    bodies = re.findall(r"l2a_rnn_micro_body<(\d), UW, CELL, MTM>\(p, env, 4 \* q0, l2a_smem\)", kernel)
    assert bodies == ["4", "3", "2", "1"]
    # body<4> exists in the MTM == 4 instances only
    guard = re.search(r"if constexpr \(MTM == 4\) \{\s*if \(mt == 4\) \{ l2a_rnn_micro_body<4,", kernel)
    assert guard is not None and kernel.count("l2a_rnn_micro_body<4,") == 1
    want = [(i.uw, i.cell, i.mtm, mt) for i in rm.INSTANCES for mt in sorted(int(b) for b in bodies) if mt <= i.mtm]
    assert want == rm.RNN_MICRO_ENUMERATED and len(want) == 27 == len(set(want))
    assert set(rm.UNREACHABLE) <= set(want) and len(rm.REACHABLE) == 27 - len(rm.UNREACHABLE)


@pytest.mark.parametrize("row", rm.ROWS + rm.REFRESH_ROWS, ids=[r.id for r in rm.ROWS + rm.REFRESH_ROWS])
def test_row_routes_to_its_bodies(row):
    g = _geometry(row)
    mtm, mts = (row.instance.mtm, row.mts) if isinstance(row, rm.Row) else (3, (1,))
    assert (g["family"], g["mtm"]) == ("generic_micro", mtm), (row.id, g)
    assert rm.workgroup_sizes(g) == set(mts), (row.id, g)
    assert g["workgroups"] == row.m * g["mc_w"]
    # the instance l2a_launch_rnn_micro picks: width and cell of the model, mtm of the plan
    assert len(set(row.units)) == 1 and row.units[0] in (256, 512)
    if isinstance(row, rm.Row):
        assert row.instance == rm.Instance(row.units[0] // 256, row.cell, g["mtm"])
    # policy 1 takes micro tiles for these models wherever policy 2 does; policy 0 runs the 16-candidate matrix-core kernel
    assert _geometry(row, micro=1) == g
    assert _geometry(row, micro=0)["family"] in ("generic_mfma16", "generic_valu")
    assert row.h == 3 and row.n % 4 != 0 and row.m * row.n * row.h <= 128 * 37 * 3


def test_rows_cover_every_reachable_pair_and_every_edge():
    assert len({r.id for r in rm.ROWS}) == len(rm.ROWS)
    covered = {(r.instance.uw, r.cell, r.instance.mtm, mt) for r in rm.ROWS for mt in r.mts}
    assert covered == set(rm.REACHABLE), (sorted(set(rm.REACHABLE) - covered), sorted(covered - set(rm.REACHABLE)))
    for inst in rm.INSTANCES:
        mine = [r for r in rm.ROWS if r.instance == inst]
        assert {(r.obs_dim, r.act_dim) for r in mine} == set(rm.EDGES), inst
        assert {"tanh", "relu"} <= {r.activation for r in mine} and {r.activation for r in mine} & {"sigmoid", "swish"}, inst
        assert any(r.n % 4 != 0 for r in mine) and {"vel", "dist"} <= {r.reward for r in mine}
        assert {len(r.units) for r in mine} == set(rm.DEPTHS[inst]), inst
    # what each edge is there for, restated: KG0 = ceil(inputs / 16) odd is the zero-padded case, OT = ceil(obs / 16)
    kg0 = lambda od, ad: (od + ad + 15) // 16  # noqa: E731
    assert {kg0(*e) for e in rm.EDGES} == {1, 2, 3, 4, 5} and {(e[0] + 15) // 16 for e in rm.EDGES} == {1, 2, 3, 4}
    assert [e for e in rm.EDGES if e[0] % 16 == 0] == [(16, 1), (48, 16), (64, 1), (64, 16)]
    assert any(e[0] % 16 + e[1] > 16 for e in rm.EDGES) and (3, 1) in rm.EDGES and (64, 16) in rm.EDGES


def _micro(cell, units, m=2, n=37, shape=(64, 16)):
    """The launch of a plan, or None where the launcher takes no such model at all."""
    try:
        return _lib.lstm_plan_geometry(shape[0], shape[1], list(units), cell, m, n, rm.H, micro=2, cus=256)
    except _lib.L2AError:
        return None


def test_depths_are_what_the_launcher_gives_micro_tiles():
    """The deepest stack `l2a_lstm_plan_geometry` still reports as `generic_micro`, per cell, width and mtm - asked, not assumed:
    a launcher that accepts one more layer fails here until the table has its row.  (L2A_RNN_MAX_LAYERS = 4: a four-layer stack
    of 256-unit cells is refused outright - no 16-candidate kernel holds its 1024 state columns in LDS, and `gmicro_ok` asks for
    one - so no four-layer row is required.)"""
    for inst in rm.INSTANCES:
        m, n = (rm.PLANS3[0].m, rm.PLANS3[0].n) if inst.mtm == 3 else (rm.PLANS4[0].m, rm.PLANS4[0].n)
        eligible = []
        for depth in (1, 2, 3, 4):
            for shape in ((3, 1), (64, 16)):
                g = _micro(inst.cell, (256 * inst.uw,) * depth, m, n, shape)
                ok = g is not None and (g["family"], g["mtm"]) == ("generic_micro", inst.mtm)
                if shape == (3, 1):
                    first = ok
                assert ok == first, (inst, depth)       # eligibility does not hang on the input shape
            if ok:
                eligible.append(depth)
        assert tuple(eligible) == rm.DEPTHS[inst], (inst, eligible)
    # one LSTM layer of 256 or 512 units is the tuned kernel's model; no four-layer stack and no two-layer 512 stack is taken
    assert _micro("lstm", (256,))["family"] == "lstm_micro" and _micro("lstm", (512,))["family"] == "lstm_micro"
    for cell in ("lstm", "gru", "rnn"):
        assert _micro(cell, (256,) * 4) is None and _micro(cell, (512,) * 2) is None


def test_the_deal_reaches_every_body_and_one_of_them_only_with_more_envs_than_cus():
    """Every (m <= 320, n <= 132) plan of every instance's shallowest and deepest model on 256 CUs: the pairs the launcher
    deals are exactly REACHABLE = the enumeration minus UNREACHABLE (empty: every body runs).  The arithmetic of the table's
    comment, checked: with m <= CUs no plan runs MT = 1 on a four-tile instance and MT = 2 runs there for five quads on more
    than CUs / 2 envs alone; with m > CUs the four-tile instances take every plan, one quad per env included."""
    assert not rm.UNREACHABLE and rm.REACHABLE == rm.RNN_MICRO_ENUMERATED
    seen, small_of_4 = set(), set()
    for uw, cell in sorted({(i.uw, i.cell) for i in rm.INSTANCES}):
        depths = sorted({d for i in rm.INSTANCES if (i.uw, i.cell) == (uw, cell) for d in rm.DEPTHS[i]})
        for depth in (depths[0], depths[-1]):
            units = (256 * uw,) * depth
            for m in range(1, 321):
                for n in range(1, 133):
                    g = _lib.lstm_plan_geometry(20, 6, list(units), cell, m, n, rm.H, micro=2, cus=256)
                    if g["family"] != "generic_micro":
                        continue
                    assert 1 <= g["mc_r"] <= g["mc_w"] and 1 <= g["mc_hi"] <= g["mtm"] and g["mtm"] in (3, 4)
                    quads = (n + 3) // 4
                    assert (g["mtm"] == 4) == (quads > 3 * (256 // m))      # the four-tile instance: where three per workgroup do not hold the plan
                    assert g["mc_r"] * g["mc_hi"] + (g["mc_w"] - g["mc_r"]) * (g["mc_hi"] - 1) == quads       # every quad dealt once
                    for mt in rm.workgroup_sizes(g):
                        assert mt >= 1
                        seen.add((uw, cell, g["mtm"], mt))
                        if g["mtm"] == 4 and mt <= 2:
                            small_of_4.add((mt, "m <= 128" if m <= 128 else "m <= 256" if m <= 256 else "m > 256", quads))
    assert seen == set(rm.REACHABLE), (sorted(seen - set(rm.REACHABLE)), sorted(set(rm.REACHABLE) - seen))
    assert small_of_4 == {(2, "m <= 256", 5), (2, "m > 256", 5), (2, "m > 256", 2), (1, "m > 256", 1)}, sorted(small_of_4)
    # the plans behind the `mt32of4` and `mt1of4` rows are of those families
    assert [(p.m, (p.n + 3) // 4, p.mts) for p in rm.PLANS4[1:]] == [(129, 5, (3, 2)), (257, 1, (1,))]


@pytest.mark.parametrize("row", rm.ROWS + rm.REFRESH_ROWS, ids=[r.id for r in rm.ROWS + rm.REFRESH_ROWS])
def test_oracle_stays_finite_and_separable(row):
    import test_gpu_rnn_micro_matrix as gpu
    case = gpu.oracle_case(row)
    print("%s: top-2 margin of the oracle's returns %.3e, largest |return| %.3e" % (row.id, gpu.margin(case.want), np.max(np.abs(case.want))))
    assert case.want.shape == (row.m, row.n)
    assert np.all(np.isfinite(case.want)) and np.max(np.abs(case.want)) < 1e3
    assert gpu.margin(case.want) >= gpu.MARGIN, "change the salt of %s in rnn_micro_matrix.SALTS" % row.id
    # states that differ per env
    _, _, h_flat, _ = case.host_inputs
    assert np.all(np.abs(h_flat) > 0) and len({h_flat[i].tobytes() for i in range(row.m)}) == row.m
    if isinstance(row, rm.RefreshRow):      # the second weight set: another model, separable too
        params, _ = gpu.model_of(row, "second weights")
        want = gpu.oracle_returns(row, params, case.norm, case.oracle_inputs)
        assert np.all(np.isfinite(want)) and gpu.margin(want) >= gpu.MARGIN
        assert gpu._tol_returns(want, case.want) > 100 * gpu.RTOL


def test_gpu_file_runs_every_row():
    import test_gpu_rnn_micro_matrix as gpu
    for fn, rows in ((gpu.test_rnn_micro_body_matches_oracle, rm.ROWS), (gpu.test_second_set_weights_refreshes_the_micro_pack, rm.REFRESH_ROWS)):
        marks = list(fn.pytestmark)
        assert [m.name for m in marks] == ["parametrize"], marks             # no skip / xfail mark on the test
        args = marks[0].args[1]
        assert list(args) == list(rows) and all(type(a) in (rm.Row, rm.RefreshRow) for a in args)     # plain rows: no marked parameter
        assert list(marks[0].kwargs["ids"]) == [r.id for r in rows]
    assert gpu.pytestmark.name == "gpu"
    assert [(r.cell, r.units) for r in rm.REFRESH_ROWS] == [("lstm", (256, 256)), ("gru", (256,)), ("rnn", (256,)), ("gru", (512,)),
                                                           ("rnn", (512,))]
    assert (gpu.RTOL, gpu.MARGIN, gpu.PAIR_TOL, gpu.DISCOUNT) == (1e-4, 1e-3, {256: 2e-6, 512: 4e-6}, 0.97) and gpu.OFFSET != 0
