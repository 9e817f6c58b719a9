"""The table of the GrBAL adaptation kernels (tests/adapt_matrix.py) against the sources, itself and its judge, without a GPU.

(a) the constants `branches` computes with are parsed out of csrc/l2a_adapt.h and are still the ones the rows were chosen
    under; the loops and predicates it restates are still spelled in the kernels the way it assumes;
(b) every row's branch set equals the committed one (tests/adapt_matrix_branches.json) and `WHY` names exactly what the row
    adds over every smaller model; `ALL_BRANCHES` is covered; a row that adds nothing says why it is kept;
(c) the loop boundaries sit where the table's rows assume: staged at 128 inputs / unstaged at 129, one forward batch at
    K = 512 / two at 516, one batch of vector groups at 512 units / two at 528, one narrow batch at 256 / two at 260;
(d) the judge is pinned on the CPU: the float64 autograd step equals oracle/adapt.py's hand-written backward pass, and for the
    identity nonlinearity a NumPy backward pass written out here;
(e) no row is vacuous: in float64 every parameter tensor of every task of every row moves by max |lr g| >= 2.5e-4;
(f) the GPU file runs every row: none skipped, deselected by a mark or expected to fail.
"""

import json
import os
import re

import numpy as np
import pytest

import adapt_matrix as am
from learning_to_adapt_amd import _lib
from oracle import adapt as oadapt

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adapt_matrix_branches.json")
IDS = [r.name for r in am.ROWS]


def test_constants_and_predicates_are_the_sources():
    assert am.C == am.CONSTANTS_AT_TABLE_TIME, "retuned: re-derive the rows of tests/adapt_matrix.py (and its json table)"
    k = am._source("l2a_adapt.h")
    # the loops and predicates `branches` restates, as the kernels spell them
    for text in ("const bool staged = k_in <= L2A_XS_MAX;",
                 "const int chunk = (k_in + L2A_AW - 1) / L2A_AW;",
                 "constexpr int NX = (L2A_XS_MAX * L2A_AR + 64 * L2A_AW - 1) / (64 * L2A_AW);",
                 "const bool do_y = blockIdx.x == 0;",
                 "const int steps = (k_in + 3) / 4, per = (steps + L2A_AW - 1) / L2A_AW;",
                 "for (int s = s0; s < s1; s += L2A_SB) {",
                 "return (p.dims[l + 1] & 3) == 0 && (reinterpret_cast<unsigned long long>(p.w[l]) & 15ull) == 0;",
                 "if ((n_out & 15) == 0 && (reinterpret_cast<unsigned long long>(p.w[l]) & 15ull) == 0) {",
                 "const int groups = n_out >> 4, perg = (groups + L2A_AW - 1) / L2A_AW;",
                 "for (int g = g0; g < g1; g += GB) {",
                 "const int u4 = 16 * (ok ? g + jg : g0) + 4 * q;",
                 "const int steps = (n_out + 3) / 4, per = (steps + L2A_AW - 1) / L2A_AW;",
                 "for (int s = s0; s < s1; s += SBB) {",
                 "return ((p.dims[l + 1] + 255) / 256) * ((p.dims[l] + L2A_UK - 1) / L2A_UK);",
                 "const int b = 2 * ((int)blockIdx.x - S) + (int)(threadIdx.x >> 8);",
                 "if (k1 - k0 == L2A_UK) {",
                 "const bool mk_vec = d.has_mk && !(l == p.n_layers - 1 && d.mk_o4 && u >= 16);",
                 "for (int k = part; k < k_in0; k += L2A_AW) {"):
        assert k.count(text) == 1, text
    api = am._source("l2a_api.hip")
    for text in ("md->micro_ok = md->mfma_ok && (md->H == 256 || md->H == 512);",
                 "md->m_o4 = (md->micro_ok && md->OT == 2 && md->KG0 == 2 && n_hidden > 1 && obs_dim - 16 <= 4) ? 1 : 0;",
                 "d.has_pk = md->mfma_ok ? 1 : 0;", "d.has_mk = md->micro_ok ? 1 : 0;",
                 "if (md->in_dim > L2A_XS_MAX)",
                 "if (rows < 1 || rows > L2A_AR)"):
        assert api.count(text) == 1, text
    # what the library accepts: the envelope the table walks
    assert "if (hidden[i] < 1 || hidden[i] > 1024)" in api and "if (n_hidden < 1 || n_hidden > L2A_MAX_LAYERS - 1)" in api


def test_eligibility_restatement_is_the_librarys():
    lib = _lib.load()
    import ctypes
    shapes = [(od, ad) for od in (1, 16, 17, 20, 21, 41, 64, 65) for ad in (1, 6, 16, 17)] + [(70, 10), (64, 16), (65, 15)]
    for hidden in ((128,), (256, 256), (512,) * 3, (128,) * 8, (64,), (96, 96), (256, 128), (200, 72), (1024, 1024), (128,) * 4):
        hid = (ctypes.c_int * len(hidden))(*hidden)
        for od, ad in shapes:
            assert bool(lib.l2a_mfma_eligible(od, ad, len(hidden), hid)) == am.mfma_eligible(od, ad, hidden), (od, ad, hidden)
    # the micro-tile copy and its O4 scatter: l2a_micro_layout_floats is non-zero exactly where model_shape sets micro_ok
    for row in am.ROWS:
        pk, mk, o4 = am.model_copies(row.od, row.ad, row.hidden)
        floats = lib.l2a_micro_layout_floats(row.od, row.ad, len(row.hidden), row.hidden[0]) if pk else 0
        assert (floats > 0) == mk, row.name
    assert am.model_copies(20, 6, (256, 256)) == (True, True, True) and am.model_copies(20, 6, (256,)) == (True, True, False)
    assert am.model_copies(21, 6, (256, 256))[2] is False and am.model_copies(20, 6, (128, 128)) == (True, False, False)


@pytest.mark.parametrize("row", am.ROWS, ids=IDS)
def test_row_reaches_its_branches(row):
    with open(TABLE) as f:
        table = json.load(f)
    got = am.row_branches(row)
    assert sorted(got) == table[row.name], (sorted(got - set(table[row.name])), sorted(set(table[row.name]) - got))
    assert got <= set(am.ALL_BRANCHES), sorted(got - set(am.ALL_BRANCHES))
    assert set(am.WHY[row.name]) <= got
    assert row.n_sets == row.m + 2 and 1 <= row.rows <= am.C["L2A_AR"] and row.lr in (0.01, 0.1, 1.0)
    assert row.entry in ("device", "host", "raw") and row.act in ("relu", "tanh", "sigmoid", "identity")
    assert 1 <= len(row.hidden) <= 8 and all(1 <= h <= 1024 for h in row.hidden) and row.ad <= 16
    if row.entry == "raw":
        assert row.od + row.ad <= am.C["L2A_XS_MAX"]


def test_table_covers_every_branch_and_no_row_is_redundant_without_saying_so():
    with open(TABLE) as f:
        assert sorted(json.load(f)) == sorted(IDS) and len(set(IDS)) == len(IDS) == len(am.WHY)
    assert len(set(am.ALL_BRANCHES)) == len(am.ALL_BRANCHES)
    reached = set().union(*(am.row_branches(r) for r in am.ROWS))
    assert reached == set(am.ALL_BRANCHES), (sorted(set(am.ALL_BRANCHES) - reached), sorted(reached - set(am.ALL_BRANCHES)))
    new = am.new_branches()
    for row in am.ROWS:
        assert set(am.WHY[row.name]) == new[row.name], (row.name, sorted(new[row.name]))
        assert new[row.name] or row.combo, "%s reaches nothing a smaller row does not: drop it or say why it is kept" % row.name
    # the spread of the table
    assert {r.m for r in am.ROWS} >= {1, 2, 3, 5} and {r.rows for r in am.ROWS} >= {1, 3, 7, 15, 16}
    raw = [r for r in am.ROWS if r.entry == "raw"]
    assert {r.od + r.ad for r in raw} >= {4, 49, 128} and {r.rows for r in raw} >= {1, 7, 16} and {r.hidden[0] for r in raw} == {50, 64, 200}
    assert any(r.od * am.C["L2A_AR"] > 1536 for r in raw)
    mis = [r for r in am.ROWS if not r.aligned]
    assert len(mis) == 3 and any(r.hidden == (1024, 1024) for r in mis)
    for r in mis:       # each beside the aligned run of the same model
        twin = am.BY_NAME[r.name[:-4]]
        assert r.name.endswith("-mis") and twin.aligned and twin._replace(name=r.name, aligned=False, combo=r.combo) == r
    assert {len(r.hidden) for r in am.ROWS} >= {1, 2, 3, 4, 8} and {r.od for r in am.ROWS} >= {65, 100, 130}
    packed = {(r.hidden[0], len(r.hidden)) for r in am.ROWS if am.mfma_eligible(r.od, r.ad, r.hidden)}
    assert packed >= {(w, d) for w in (128, 256, 512) for d in (1, 2, 3)}
    assert {(r.od, r.ad) for r in am.ROWS if r.name.startswith("p")} == {(41, 8), (20, 6), (17, 1), (64, 16)}
    assert set(am.TWICE) <= set(IDS) and len(am.TWICE) == 3 and any("l0.unstaged" in am.row_branches(am.BY_NAME[n]) for n in am.TWICE)
    host = am.BY_NAME["in129-h70-50-host"]
    assert host.entry == "host" and host.od + host.ad == 129


def test_the_boundaries_hold():
    b = lambda od, ad, hidden, aligned=True, entry="device": am.branches(od, ad, hidden, 16, aligned, entry)  # noqa: E731
    assert "l0.staged" in b(112, 16, (70, 50)) and "l0.unstaged" in b(113, 16, (70, 50))
    assert am.forward_geometry(512)["batches"] == 1 and am.forward_geometry(512)["lens"] == [16] * 8
    assert am.forward_geometry(516)["batches"] == 2 and am.forward_geometry(516)["lens"] == [17] * 7 + [10]
    assert am.forward_geometry(1024)["lens"] == [32] * 8 and not am.forward_geometry(1024)["partial"]
    assert "fwd.batches=1" in b(20, 6, (512, 64)) and "fwd.batches=2" not in b(20, 6, (512, 64))
    assert {"fwd.batches=2", "fwd.batch_of_one"} <= b(20, 6, (516, 64))
    g512, g528 = am.backward_geometry(512, True), am.backward_geometry(528, True)
    assert (g512["path"], g512["batches"], g512["lens"]) == ("vec", 1, [4] * 8)
    assert (g528["path"], g528["batches"], g528["lens"]) == ("vec", 2, [5] * 6 + [3, 0])
    assert "bwd.vec.batches=2" not in b(20, 6, (64, 512, 64)) and {"bwd.vec.batches=2", "bwd.vec.batch_of_one"} <= b(20, 6, (64, 528, 64))
    n256, n260 = am.backward_geometry(256, False), am.backward_geometry(260, True)
    assert (n256["path"], n256["batches"], n256["lens"]) == ("nar", 1, [8] * 8)
    assert (n260["path"], n260["batches"], n260["lens"]) == ("nar", 2, [9] * 7 + [2])
    assert "bwd.nar.batches=2" in b(20, 6, (64, 260)) and "bwd.nar.batches=2" not in b(20, 6, (64, 252))
    # what (516, 64) and (300, 528) do NOT reach - the backward pass of layer l walks dims[l + 1], which is 64, 20 and
    # 528 (a multiple of 16: the vector path) there - and why the table has (64, 260) for the narrow path's second batch
    for hidden in ((516, 64), (300, 528)):
        assert not any(x.startswith("bwd.nar.batches=") and x != "bwd.nar.batches=1" for x in b(20, 6, hidden))
    # raw mode's per-thread element budget: four elements of x at 128 inputs, the fourth of y above 96 observation dims
    assert "raw.x_q=4" in b(112, 16, (200,), entry="raw") and "raw.y_q=4" in b(112, 16, (200,), entry="raw")
    assert {"raw.x_q=3", "raw.y_q=3"} <= b(80, 16, (64,), entry="raw") and "raw.y_q=3" in b(96, 16, (200,), entry="raw")
    # update geometry
    assert {"upd.ublocks=3", "upd.odd_blocks"} <= b(20, 6, (16, 600)) and "upd.ublocks=4" in b(20, 6, (1024, 1024))


def _numpy_identity_step(base, x, y, lr):
    """theta - lr * grad mean((y - f(x))^2) for a purely linear stack, written out: dZ_L = 2 (f - y) / size, dW_l = A_l^T dZ_{l+1},
    db_l = column sums, dZ_l = dZ_{l+1} W_l^T."""
    params = [np.asarray(p, dtype=np.float64) for p in base]
    a = [np.asarray(x, dtype=np.float64)]
    for li in range(len(params) // 2):
        a.append(a[-1] @ params[2 * li] + params[2 * li + 1])
    dz = 2.0 * (a[-1] - np.asarray(y, dtype=np.float64)) / a[-1].size
    out = [None] * len(params)
    for li in range(len(params) // 2 - 1, -1, -1):
        out[2 * li] = params[2 * li] - lr * (a[li].T @ dz)
        out[2 * li + 1] = params[2 * li + 1] - lr * dz.sum(axis=0)
        dz = dz @ params[2 * li].T
    return out


@pytest.mark.parametrize("row", am.ROWS, ids=IDS)
def test_judge_is_pinned_and_the_row_is_not_vacuous(row):
    inp = am.inputs(row)
    ref = am.reference(row.name)
    assert len(ref) == row.m and inp["x"].shape == (row.m, row.rows, row.od + row.ad) and inp["y"].shape == (row.m, row.rows, row.od)
    assert inp["x"].dtype == np.float32 and np.all(np.isfinite(inp["x"])) and np.abs(inp["x"]).max() < 1e3
    smallest = np.inf
    for e, (want, steps) in enumerate(ref):
        grads = oadapt.loss_gradients([np.asarray(p, dtype=np.float64) for p in inp["base"]], inp["x"][e].astype(np.float64),
                                      inp["y"][e].astype(np.float64), row.act, None, dtype=np.float64)
        other = _numpy_identity_step(inp["base"], inp["x"][e], inp["y"][e], row.lr) if row.act == "identity" else None
        for pi, (p, w, s, g) in enumerate(zip(inp["base"], want, steps, grads)):
            scale = max(1.0, float(np.abs(s).max()))
            assert np.abs(s - row.lr * g).max() <= 1e-12 * scale, (row.name, e, pi)
            assert np.array_equal(w, np.asarray(p, dtype=np.float64) - s)
            if other is not None:
                assert np.abs(w - other[pi]).max() <= 1e-12 * scale, (row.name, e, pi)
            smallest = min(smallest, float(np.abs(s).max()))
    print("%s: smallest max |lr g| over tasks and tensors %.3e" % (row.name, smallest))
    assert smallest >= am.MIN_STEP, "pick a larger lr for %s" % row.name
    # tasks differ, sentinels differ from the base and from one another
    assert len({inp["x"][e].tobytes() for e in range(row.m)}) == row.m
    heads = [am.sentinel(row, e)[0].tobytes() for e in range(row.n_sets)] + [inp["base"][0].tobytes()]
    assert len(set(heads)) == row.n_sets + 1
    if row.entry == "raw":
        j = row.od // 2
        assert inp["norm"]["obs"][1][j] == 0.0 and np.all(inp["x"][:, :, j] == 0.0) and np.all(np.isfinite(inp["x"]))


def test_bar_is_the_projects():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_random_shapes.py")).read()
    assert "assert np.abs(w1 - want).max() <= 3e-5 * max(step, 1e-3) + 2e-7" in src
    assert am.bar(0.0) == 3e-5 * 1e-3 + 2e-7 and am.bar(0.5) == 3e-5 * 0.5 + 2e-7 and am.MIN_STEP == 2.5e-4


def test_gpu_file_runs_every_row():
    import test_gpu_adapt_matrix as gpu
    marks = list(gpu.test_row_matches_the_float64_step.pytestmark)
    assert [m.name for m in marks] == ["parametrize"], marks
    assert list(marks[0].args[1]) == list(am.ROWS) and all(type(a) is am.Row for a in marks[0].args[1])
    assert list(marks[0].kwargs["ids"]) == IDS
    marks = list(gpu.test_second_step_depends_on_the_base_alone.pytestmark)
    assert [m.name for m in marks] == ["parametrize"] and list(marks[0].args[1]) == list(am.TWICE)
    assert not hasattr(gpu.test_refusals_leave_every_set_alone, "pytestmark")
    assert gpu.pytestmark.name == "gpu"
    assert (gpu.PLAN_N, gpu.PLAN_H, gpu.PREDICT_ROWS, gpu.PREDICT_TOL) == (37, 3, 24, 2e-4)
    src = open(gpu.__file__).read()
    assert not re.search(r"skip|xfail", src)
