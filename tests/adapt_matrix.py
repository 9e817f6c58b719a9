"""One row per loop end and branch of the GrBAL adaptation kernels: the table behind tests/test_adapt_matrix.py (the restatement
of the kernels' predicates, coverage and the float64 judge, no GPU) and tests/test_gpu_adapt_matrix.py (every row against a
float64 autograd step on the GPU).

``csrc/l2a_adapt.h`` holds ``l2a_adapt_fwd0_k`` (layer 0, a lane-per-unit FMA loop over a batch staged in LDS - or read in
place when the input layer is wider than ``L2A_XS_MAX``), ``l2a_adapt_fwd_k`` (layers >= 1 on the matrix core: the eight waves
split the k-steps, operands fetched in batches of ``L2A_SB`` steps) and ``l2a_adapt_bwdu_k`` (dZ_l on the matrix core - 16-byte
weight loads in batches of ``GB`` groups of sixteen units, or a narrow path in batches of ``SBB`` steps - beside the update
blocks of layer l, and layer 0's update by the last backward launch).  ``branches`` restates, from the constants PARSED out of
that header, which of those loops run how often and which clamps are live for a model; a retuned constant moves the answers and
the committed table (tests/adapt_matrix_branches.json) fails instead of a branch silently losing its row.

A row is (name, od, ad, hidden, act, m, n_sets, rows, lr, entry, aligned) plus ``combo`` - the reason a row that reaches nothing
new is kept; ``WHY`` names, per row, the branches the row is there for: the ones no smaller row (fewer parameters) reaches.
``entry``: ``device`` (``l2a_model_adapt_sgd``), ``host`` (``l2a_model_adapt_sgd_host``) or ``raw``
(``l2a_model_adapt_sgd_raw``).  ``aligned`` False: every base tensor is a view one float into a larger buffer (contiguous,
``data_ptr() % 16 == 4``).  ``lr`` is 0.1 or 1, chosen per row so that every tensor's float64 step reaches
``MIN_STEP`` (asserted in test_adapt_matrix.py).
"""

import functools
import os
import re
from collections import namedtuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "learning_to_adapt_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def parse_constants():
    """The tuning constants of csrc/l2a_adapt.h (and the matrix-core limits of csrc/l2a_kernels.h), each defined exactly once."""
    adapt, kernels = _source("l2a_adapt.h"), _source("l2a_kernels.h")
    out = {}
    for name in ("L2A_AR", "L2A_AW", "L2A_SB", "L2A_XS_MAX", "L2A_UK"):
        found = re.findall(r"^#define %s (\d+)\b" % name, adapt, flags=re.M)
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    for name in ("GB", "SBB"):
        found = re.findall(r"constexpr int %s = (\d+);" % name, adapt)
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    for name in ("L2A_OTMAX", "L2A_KG0MAX", "L2A_MAX_LAYERS"):
        found = re.findall(r"^#define %s (\d+)\b" % name, kernels, flags=re.M)
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    return out


C = parse_constants()
# what the rows were chosen under; test_adapt_matrix.py asserts the parsed values are still these
CONSTANTS_AT_TABLE_TIME = dict(L2A_AR=16, L2A_AW=8, L2A_SB=16, L2A_XS_MAX=128, L2A_UK=16, GB=4, SBB=8, L2A_OTMAX=4, L2A_KG0MAX=5,
                               L2A_MAX_LAYERS=9)


def _cdiv(a, b):
    return (a + b - 1) // b


def mfma_eligible(od, ad, hidden):
    """``mfma_eligible`` of csrc/l2a_api.hip: the planner's matrix-core kernels take the model -> the update writes the MFMA
    fragment order beside the raw layout (``has_pk``)."""
    H = hidden[0]
    return (1 <= len(hidden) <= C["L2A_MAX_LAYERS"] - 1 and H in (128, 256, 512) and all(h == H for h in hidden)
            and 1 <= od <= 16 * C["L2A_OTMAX"] and 1 <= ad <= 16 and od + ad <= 16 * C["L2A_KG0MAX"])


def model_copies(od, ad, hidden):
    """(has_pk, has_mk, m_o4) as ``model_shape`` of csrc/l2a_api.hip derives them."""
    pk = mfma_eligible(od, ad, hidden)
    mk = pk and hidden[0] in (256, 512)
    KG0, OT = _cdiv(od + ad, 16), _cdiv(od, 16)
    o4 = mk and OT == 2 and KG0 == 2 and len(hidden) > 1 and od - 16 <= 4
    return pk, mk, o4


def _split(total, per, waves):
    """The waves' shares [s0, s1) of `total` steps, `per` each (``s0 = min(w * per, total)``, ``s1 = min(s0 + per, total)``)."""
    out = []
    for w in range(waves):
        s0 = min(w * per, total)
        out.append((s0, min(s0 + per, total)))
    return out


def forward_geometry(k_in):
    """Layer l >= 1, forward: k-steps of four, the waves' shares, batches of L2A_SB per wave."""
    steps = _cdiv(k_in, 4)
    per = _cdiv(steps, C["L2A_AW"])
    shares = _split(steps, per, C["L2A_AW"])
    lens = [s1 - s0 for s0, s1 in shares]
    return dict(steps=steps, per=per, lens=lens, batches=max(_cdiv(n, C["L2A_SB"]) for n in lens),
                partial=any(n % C["L2A_SB"] for n in lens if n), full=any(n and n % C["L2A_SB"] == 0 for n in lens),
                empty=sum(1 for n in lens if n == 0))


def backward_geometry(n_out, aligned):
    """Layer l >= 1, backward: the vector path (groups of sixteen u, batches of GB) or the narrow one (u-steps of four, SBB)."""
    if n_out % 16 == 0 and aligned:
        total, batch, path = n_out // 16, C["GB"], "vec"
    else:
        total, batch, path = _cdiv(n_out, 4), C["SBB"], "nar"
    per = _cdiv(total, C["L2A_AW"])
    lens = [s1 - s0 for s0, s1 in _split(total, per, C["L2A_AW"])]
    return dict(path=path, total=total, per=per, lens=lens, batches=max(_cdiv(n, batch) for n in lens),
                partial=any(n % batch for n in lens if n), full=any(n and n % batch == 0 for n in lens),
                empty=sum(1 for n in lens if n == 0))


def branches(od, ad, hidden, rows, aligned, entry):
    """The named branches one adaptation step of this model takes, computed the way the kernels and the launcher compute them."""
    AW, XS, AR, UK = C["L2A_AW"], C["L2A_XS_MAX"], C["L2A_AR"], C["L2A_UK"]
    dims = [od + ad] + list(hidden) + [od]
    L = len(dims) - 1
    out = {"entry.%s" % entry, "depth=%d" % len(hidden), "rows=16" if rows == AR else "rows<16",
           "base.aligned" if aligned else "base.misaligned"}

    # ---- l2a_adapt_fwd0_k ---------------------------------------------------------------------------------------------------
    k_in, n_out = dims[0], dims[1]
    staged = k_in <= XS
    out.add("l0.staged" if staged else "l0.unstaged")
    chunk = _cdiv(k_in, AW)
    lens = [e - s for s, e in _split(k_in, chunk, AW)]
    out.add("l0.chunk=1" if chunk == 1 else ("l0.chunk=max" if chunk == _cdiv(XS, AW) else
                                             ("l0.chunk>max" if chunk > _cdiv(XS, AW) else "l0.chunk.mid")))
    if any(n == 0 for n in lens):
        out.add("l0.empty_waves")
    if any(0 < n < chunk for n in lens):
        out.add("l0.ragged_wave")
    out.add("l0.n_out<64" if n_out < 64 else ("l0.slices>1" if n_out > 64 else "l0.slices=1"))
    if n_out >= 64 and n_out % 64:
        out.add("l0.partial_slice")
    if entry == "raw":
        # NX = 4 elements per thread: element i = tid + q * 512; the last q is live for x above 1536 elements, for y likewise
        nx = _cdiv(XS * AR, 64 * AW)
        out.add("raw.x_q=%d" % _cdiv(k_in * AR, 64 * AW))
        out.add("raw.y_q=%d" % _cdiv(od * AR, 64 * AW))
        assert _cdiv(k_in * AR, 64 * AW) <= nx
        if n_out > 64:
            out.add("raw.y_by_block0_of_many")
    # layer 0's update (l2a_adapt_update0_cols -> l2a_adapt_put, element by element)
    pk, mk, o4 = model_copies(od, ad, hidden)
    out.add("upd0.pk+mk" if mk else ("upd0.pk" if pk else "upd0.raw_only"))
    if pk:
        out.add("pk.H=%d" % hidden[0])
        out.add("pk.KG0=%d" % _cdiv(od + ad, 16))
        out.add("pk.OT=%d" % _cdiv(od, 16))
    if k_in < AW:
        out.add("upd0.idle_parts")

    for l in range(1, L):
        k_in, n_out = dims[l], dims[l + 1]
        last = l == L - 1
        tag = "out" if last else "hid"
        # ---- l2a_adapt_fwd_k ------------------------------------------------------------------------------------------------
        if n_out % 4:
            out.add("fwd.%s.novec_width" % tag)
        elif not aligned:
            out.add("fwd.%s.novec_align" % tag)
        else:
            out.add("fwd.%s.vec" % tag)
        g = forward_geometry(k_in)
        out.add("fwd.batches=%d" % g["batches"])
        if g["batches"] > 1:
            out.add("fwd.batch2." + ("partial" if g["partial"] else "full"))
        if g["partial"]:
            out.add("fwd.partial_batch")
        if g["full"]:
            out.add("fwd.full_batch")
        if g["empty"]:
            out.add("fwd.empty_waves")
        if g["empty"] >= AW - 2:
            out.add("fwd.one_wave" if g["empty"] == AW - 1 else "fwd.two_waves")
        if g["batches"] > 1 and max(g["lens"]) % C["L2A_SB"] == 1:
            out.add("fwd.batch_of_one")
        if any(0 < n < g["per"] for n in g["lens"]):
            out.add("fwd.ragged_wave")
        if k_in % 4:
            out.add("fwd.k_tail")
        if n_out > 64:
            out.add("fwd.%s.slices>1" % tag)
        if n_out % 64:
            out.add("fwd.%s.dead_units" % tag)
        # ---- l2a_adapt_bwdu_k: dZ_l -------------------------------------------------------------------------------------------
        b = backward_geometry(n_out, aligned)
        if b["path"] == "nar":
            out.add("bwd.nar.width" if n_out % 16 else "bwd.nar.align")
            if n_out % 4:
                out.add("bwd.nar.u_tail")
        out.add("bwd.%s.batches=%d" % (b["path"], b["batches"]))
        if b["partial"]:
            out.add("bwd.%s.partial_batch" % b["path"])
        if b["full"]:
            out.add("bwd.%s.full_batch" % b["path"])
        if b["batches"] > 1 and b["partial"] and max(b["lens"]) % (C["GB"] if b["path"] == "vec" else C["SBB"]) == 1:
            out.add("bwd.%s.batch_of_one" % b["path"])
        if b["empty"]:
            out.add("bwd.%s.empty_waves" % b["path"])
        if k_in % 64:
            out.add("bwd.kok_tail")
        if k_in > 64:
            out.add("bwd.slices>1")
        # ---- l2a_adapt_bwdu_k: the update blocks of layer l ---------------------------------------------------------------------
        ublocks, kblocks = _cdiv(n_out, 256), _cdiv(k_in, UK)
        out.add("upd.ublocks=%d" % ublocks)
        if k_in >= UK:
            out.add("upd.whole_block")
        if k_in % UK:
            out.add("upd.partial_block")
        out.add("upd.one_block" if ublocks * kblocks == 1 else ("upd.odd_blocks" if (ublocks * kblocks) % 2 else "upd.even_blocks"))
        if n_out % 256:
            out.add("upd.dead_threads")
        if not pk:
            out.add("upd.raw_only")
        else:
            out.add("upd.pk")
            if mk:
                # mk_vec = has_mk && !(last layer && o4 && u >= 16)
                out.add("upd.mk_vec")
                if last and o4 and n_out > 16:
                    out.add("upd.mk_o4_scatter")
    return out


Row = namedtuple("Row", "name od ad hidden act m n_sets rows lr entry aligned seed combo")


def _row(name, od, ad, hidden, act, m, rows, lr=0.1, entry="device", aligned=True, seed=0, combo=None):
    return Row(name, od, ad, tuple(hidden), act, m, m + 2, rows, lr, entry, aligned, seed, combo)


ROWS = [
    # ---- one wave with work, widths below 64, non-VEC hidden layers, k tails -------------------------------------------------------
    _row("in4-h8", 3, 1, (8,), "tanh", 1, 1, lr=1.0),
    _row("h1", 5, 2, (1,), "tanh", 2, 3, lr=1.0),
    _row("h3-5-7", 6, 2, (3, 5, 7), "tanh", 2, 7, lr=1.0),
    _row("h50", 20, 6, (50,), "relu", 3, 15),
    _row("h70-50", 17, 1, (70, 50), "sigmoid", 5, 3, lr=1.0),
    # ---- the staging boundary of layer 0 ------------------------------------------------------------------------------------------
    _row("in128-h70-50", 112, 16, (70, 50), "tanh", 2, 5, lr=1.0),
    _row("in129-h70-50", 113, 16, (70, 50), "tanh", 2, 5, lr=1.0),
    _row("in129-h70-50-host", 113, 16, (70, 50), "tanh", 2, 5, lr=1.0, entry="host", seed=1,
         combo="the unstaged loop reading host-mapped memory element by element"),
    _row("in136-h128", 120, 16, (128,), "relu", 1, 16, combo="the unstaged loop with every row live and no ragged wave (chunk 17 x 8)"),
    # ---- second batches -------------------------------------------------------------------------------------------------------------
    _row("w516-64", 20, 6, (516, 64), "identity", 1, 16),
    _row("w64-260", 20, 6, (64, 260), "relu", 2, 7),
    _row("w300-528", 20, 6, (300, 528), "relu", 1, 16,
         combo="the vector path's second batch right behind the narrow output layer, over five slices of 300 units with a kok tail"),
    _row("w64-528-64", 20, 6, (64, 528, 64), "relu", 3, 15,
         combo="the vector path's second batch of one group with a matrix-core layer on either side of the 528 units"),
    _row("w1024x2", 20, 6, (1024, 1024), "relu", 2, 16),
    # ---- depth ------------------------------------------------------------------------------------------------------------------------
    _row("d4-64", 17, 1, (64,) * 4, "relu", 1, 16),
    _row("d8-64-relu", 20, 6, (64,) * 8, "relu", 2, 7),
    _row("d8-64-tanh", 20, 6, (64,) * 8, "tanh", 3, 3, lr=1.0, combo="eight derivative factors that are not 0 / 1"),
    _row("d4-128-sigmoid", 17, 1, (128,) * 4, "sigmoid", 1, 16, lr=1.0, combo="depth 4 on the packed copies (H = 128, no micro tiles), sigmoid"),
    # ---- the identity hidden nonlinearity --------------------------------------------------------------------------------------------
    _row("id-256x2", 41, 8, (256, 256), "identity", 2, 7, combo="identity on the packed and micro-tile copies"),
    _row("id-200-72", 33, 15, (200, 72), "identity", 3, 15, combo="identity off the tile sizes: narrow backward path, dead lanes"),
    # ---- more than 64 observation dims: two slices of the last forward launch, no packed copies -------------------------------------
    _row("od65-h64", 65, 4, (64,), "relu", 1, 16, combo="the smallest second output slice: one live unit"),
    _row("od100-h72-40", 100, 16, (72, 40), "tanh", 2, 7, lr=1.0, combo="output slices after a hidden layer that is no multiple of 4"),
    _row("od130-h64-64", 130, 16, (64, 64), "relu", 5, 3, combo="three output slices, unstaged input layer"),
    # ---- update geometry ----------------------------------------------------------------------------------------------------------------
    _row("w16-600", 20, 6, (16, 600), "relu", 1, 16),
    _row("w48-300", 20, 6, (48, 300), "tanh", 2, 15),
    # ---- the packed copies: every width x depth once, the four input shapes in turn ----------------------------------------------------
    _row("p128x1-41-8", 41, 8, (128,), "relu", 1, 16),
    _row("p128x2-20-6", 20, 6, (128, 128), "tanh", 2, 7, combo="H = 128 at depth 2 on the O4 input shape (no micro tiles: no scatter)"),
    _row("p128x3-17-1", 17, 1, (128, 128, 128), "relu", 3, 3, combo="H = 128 at depth 3"),
    _row("p256x1-64-16", 64, 16, (256,), "tanh", 5, 1),
    _row("p256x2-20-6", 20, 6, (256, 256), "relu", 1, 15),
    _row("p256x3-41-8", 41, 8, (256, 256, 256), "sigmoid", 2, 16, lr=1.0, combo="H = 256 at depth 3, sigmoid"),
    _row("p512x1-17-1", 17, 1, (512,), "relu", 3, 7),
    _row("p512x2-64-16", 64, 16, (512, 512), "relu", 1, 3, combo="H = 512 with KG0 = 5, OT = 4"),
    _row("p512x3-20-6", 20, 6, (512, 512, 512), "tanh", 2, 16, combo="the O4 scatter at H = 512, depth 3"),
    # ---- misaligned base tensors: both fallbacks ---------------------------------------------------------------------------------------
    _row("p256x2-20-6-mis", 20, 6, (256, 256), "relu", 1, 15, aligned=False),
    _row("w64-528-64-mis", 20, 6, (64, 528, 64), "relu", 3, 15, aligned=False, combo="the narrow path over 528 units: three batches"),
    _row("w1024x2-mis", 20, 6, (1024, 1024), "relu", 2, 16, aligned=False),
    # ---- the raw entry: un-normalised float64 transitions, normalised by the first launch ------------------------------------------------
    _row("raw-in4-h50", 3, 1, (50,), "tanh", 1, 1, lr=1.0, entry="raw"),
    _row("raw-in49-h64", 41, 8, (64,), "relu", 2, 7, entry="raw"),
    _row("raw-in128-h200", 112, 16, (200,), "relu", 3, 16, entry="raw"),
    _row("raw-in96-h64", 80, 16, (64,), "tanh", 2, 3, lr=1.0, entry="raw"),
    # ---- (appended: a row's seed is its position) the host entry on a staged batch; every loop's second batch at full depth -----------
    _row("h50-host", 20, 6, (50,), "relu", 3, 15, entry="host", combo="host-mapped batches through the LDS staging, ragged rows"),
    _row("d8-1024", 20, 6, (1024,) * 8, "relu", 2, 16, lr=1.0, combo="the widest and deepest model the library takes: second batches in fifteen of its seventeen launches"),
]
BY_NAME = {r.name: r for r in ROWS}

# What each row is there for: the branches no row of a smaller model reaches (test_adapt_matrix.py recomputes this from `branches`
# and `cost`; a row with an empty entry carries its reason in `combo`).  The rows' FULL branch sets are in adapt_matrix_branches.json.
WHY = {
    "in4-h8": ("fwd.two_waves",),
    "h1": ("act.tanh", "base.aligned", "bwd.kok_tail", "bwd.nar.batches=1", "bwd.nar.empty_waves", "bwd.nar.partial_batch",
           "bwd.nar.u_tail", "bwd.nar.width", "depth=1", "entry.device", "fwd.batches=1", "fwd.empty_waves", "fwd.k_tail",
           "fwd.one_wave", "fwd.out.dead_units", "fwd.out.novec_width", "fwd.partial_batch", "l0.chunk=1", "l0.empty_waves",
           "l0.n_out<64", "l0.staged", "rows<16", "upd.dead_threads", "upd.one_block", "upd.partial_block", "upd.raw_only",
           "upd.ublocks=1", "upd0.idle_parts", "upd0.raw_only"),
    "h3-5-7": ("depth=3", "fwd.hid.dead_units", "fwd.hid.novec_width"),
    "h50": ("act.relu", "fwd.out.vec", "l0.chunk.mid", "l0.ragged_wave"),
    "h70-50": ("act.sigmoid", "bwd.slices>1", "depth=2", "l0.partial_slice", "l0.slices>1", "upd.odd_blocks"),
    "in128-h70-50": ("l0.chunk=max",),
    "in129-h70-50": ("l0.chunk>max", "l0.unstaged"),
    "in129-h70-50-host": (),
    "in136-h128": (),
    "w516-64": ("fwd.batch_of_one",),
    "w64-260": ("bwd.nar.batch_of_one",),
    "w300-528": (),
    "w64-528-64": ("bwd.vec.batch_of_one", "bwd.vec.batches=2"),
    "w1024x2": ("fwd.batch2.full", "upd.ublocks=4"),
    "d4-64": ("depth=4", "fwd.hid.vec"),
    "d8-64-relu": ("depth=8",),
    "d8-64-tanh": (),
    "d4-128-sigmoid": (),
    "id-256x2": (),
    "id-200-72": ("act.identity",),
    "od65-h64": ("fwd.out.slices>1", "rows=16"),
    "od100-h72-40": (),
    "od130-h64-64": (),
    "w16-600": ("bwd.nar.batches=3", "fwd.batch2.partial", "fwd.batches=2", "upd.ublocks=3"),
    "w48-300": ("bwd.nar.batches=2", "fwd.hid.slices>1", "upd.ublocks=2"),
    "p128x1-41-8": ("pk.H=128", "pk.KG0=4", "pk.OT=3", "upd.pk", "upd0.pk"),
    "p128x2-20-6": (),
    "p128x3-17-1": (),
    "p256x1-64-16": ("pk.H=256", "pk.KG0=5", "pk.OT=4"),
    "p256x2-20-6": ("upd.mk_o4_scatter",),
    "p256x3-41-8": (),
    "p512x1-17-1": ("fwd.full_batch", "pk.H=512", "pk.KG0=2", "pk.OT=2", "upd.mk_vec", "upd0.pk+mk"),
    "p512x2-64-16": ("bwd.vec.full_batch",),
    "p512x3-20-6": (),
    "p256x2-20-6-mis": ("bwd.nar.full_batch",),
    "w64-528-64-mis": ("base.misaligned", "bwd.nar.align", "fwd.hid.novec_align", "fwd.out.novec_align"),
    "w1024x2-mis": ("bwd.nar.batches=4",),
    "raw-in4-h50": ("entry.raw", "fwd.ragged_wave", "raw.x_q=1", "raw.y_q=1", "upd.even_blocks", "upd.whole_block"),
    "raw-in49-h64": ("l0.slices=1", "raw.x_q=2", "raw.y_q=2"),
    "raw-in128-h200": ("raw.x_q=4", "raw.y_by_block0_of_many", "raw.y_q=4"),
    "raw-in96-h64": ("bwd.vec.batches=1", "bwd.vec.empty_waves", "bwd.vec.partial_batch", "raw.x_q=3", "raw.y_q=3"),
    "h50-host": ("entry.host",),
    "d8-1024": (),
}

# Two consecutive steps with different batches (the second result depends on the base alone): the unstaged row among them
TWICE = ("in129-h70-50", "p256x2-20-6", "raw-in49-h64")

# Every branch name `branches` can produce for a model the library accepts and the table is expected to reach, written out.
ALL_BRANCHES = [
    "entry.device", "entry.host", "entry.raw",
    "depth=1", "depth=2", "depth=3", "depth=4", "depth=8",
    "rows=16", "rows<16", "base.aligned", "base.misaligned", "act.relu", "act.tanh", "act.sigmoid", "act.identity",
    "l0.staged", "l0.unstaged", "l0.chunk=1", "l0.chunk.mid", "l0.chunk=max", "l0.chunk>max", "l0.empty_waves", "l0.ragged_wave",
    "l0.n_out<64", "l0.slices=1", "l0.slices>1", "l0.partial_slice",
    "raw.x_q=1", "raw.x_q=2", "raw.x_q=3", "raw.x_q=4", "raw.y_q=1", "raw.y_q=2", "raw.y_q=3", "raw.y_q=4", "raw.y_by_block0_of_many",
    "upd0.raw_only", "upd0.pk", "upd0.pk+mk", "upd0.idle_parts",
    "pk.H=128", "pk.H=256", "pk.H=512", "pk.KG0=2", "pk.KG0=4", "pk.KG0=5", "pk.OT=2", "pk.OT=3", "pk.OT=4",
    "fwd.hid.vec", "fwd.hid.novec_width", "fwd.hid.novec_align", "fwd.out.vec", "fwd.out.novec_width", "fwd.out.novec_align",
    "fwd.batches=1", "fwd.batches=2", "fwd.batch2.partial", "fwd.batch2.full", "fwd.partial_batch", "fwd.full_batch",
    "fwd.batch_of_one",
    "fwd.empty_waves", "fwd.one_wave", "fwd.two_waves", "fwd.ragged_wave", "fwd.k_tail",
    "fwd.hid.slices>1", "fwd.out.slices>1", "fwd.hid.dead_units", "fwd.out.dead_units",
    "bwd.nar.width", "bwd.nar.align", "bwd.nar.u_tail",
    "bwd.vec.batches=1", "bwd.vec.batches=2", "bwd.vec.partial_batch", "bwd.vec.full_batch", "bwd.vec.batch_of_one", "bwd.vec.empty_waves",
    "bwd.nar.batches=1", "bwd.nar.batches=2", "bwd.nar.batches=3", "bwd.nar.batches=4", "bwd.nar.partial_batch", "bwd.nar.full_batch",
    "bwd.nar.batch_of_one", "bwd.nar.empty_waves",
    "bwd.kok_tail", "bwd.slices>1",
    "upd.ublocks=1", "upd.ublocks=2", "upd.ublocks=3", "upd.ublocks=4", "upd.whole_block", "upd.partial_block", "upd.one_block",
    "upd.odd_blocks", "upd.even_blocks", "upd.dead_threads", "upd.raw_only", "upd.pk", "upd.mk_vec", "upd.mk_o4_scatter",
]


def row_branches(row):
    """`branches` of the row's model, and the row's case of the `l2a_act1` / `l2a_act_grad_from_output` switches."""
    return branches(row.od, row.ad, row.hidden, row.rows, row.aligned, row.entry) | {"act.%s" % row.act}


def new_branches():
    """Per row, the branches no smaller row reaches (rows in the order of `cost`, ties in table order)."""
    seen, out = set(), {}
    for i in sorted(range(len(ROWS)), key=lambda i: (cost(ROWS[i]), i)):
        b = row_branches(ROWS[i])
        out[ROWS[i].name] = b - seen
        seen |= b
    return out


def cost(row):
    """What "smaller" means for the rows: the parameters of the model."""
    dims = [row.od + row.ad] + list(row.hidden) + [row.od]
    return sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))


# ---- inputs and the judge -----------------------------------------------------------------------------------------------------------

def _seed(row):
    return 7000 + 97 * ROWS.index(BY_NAME[row.name]) + 13 * row.seed


def inputs(row, salt=0):
    """The base parameters (fp32), the sentinel sets, and the batches of a row: ``x`` / ``y`` fp32 normalised ``[m, rows, dim]``.
    Raw rows also carry the un-normalised float64 transitions and the normalisation they were normalised with ON THE HOST, in
    float64 and then cast - what MetaMLPDynamicsModel.adapt does; one std component is exactly 0 (the 1e-10 of the divisor is all
    that is left: that obs column equals its mean, so the normalised value is 0, not 1e10)."""
    from learning_to_adapt_amd.utils import synthetic
    rs = np.random.RandomState(_seed(row) + 1000003 * salt)
    od, ad, m, rows = row.od, row.ad, row.m, row.rows
    base = synthetic.make_weight_set(od, ad, list(row.hidden), _seed(row) + 1)
    out = dict(base=base)
    if row.entry == "raw":
        norm = {"obs": (10.0 * rs.randn(od), 0.01 + rs.rand(od)), "act": (rs.randn(ad), 50.0 + 100.0 * rs.rand(ad)),
                "delta": (0.1 * rs.randn(od), 1e-3 + 0.1 * rs.rand(od))}
        norm["obs"][1][od // 2] = 0.0
        ob = norm["obs"][0] + norm["obs"][1] * rs.randn(m, rows, od)
        ob[:, :, od // 2] = norm["obs"][0][od // 2]
        ac = rs.uniform(-150, 150, (m, rows, ad))
        nx = ob + norm["delta"][0] + norm["delta"][1] * rs.randn(m, rows, od)
        nz = lambda v, k: (v - norm[k][0]) / (norm[k][1] + 1e-10)  # noqa: E731
        out.update(norm=norm, obs=ob, act=ac, obs_next=nx)
        out["x"] = np.concatenate([nz(ob, "obs"), nz(ac, "act")], axis=2).astype(np.float32)
        out["y"] = nz(nx - ob, "delta").astype(np.float32)
    else:
        out["x"] = rs.randn(m, rows, od + ad).astype(np.float32)
        out["y"] = rs.randn(m, rows, od).astype(np.float32)
    return out


def sentinel(row, e):
    """The distinct model set `e` holds before the step."""
    from learning_to_adapt_amd.utils import synthetic
    return synthetic.make_weight_set(row.od, row.ad, list(row.hidden), 900000 + 31 * ROWS.index(BY_NAME[row.name]) + e)


def autograd_step(base, x, y, act, lr):
    """One task's float64 step theta - lr * grad mean((y - f(x))^2) by torch autograd (meta_mlp_dynamics.py:409-421, loss :118):
    (adapted parameters, lr * gradients), float64 arrays."""
    import torch
    fn = {"relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "identity": lambda t: t}[act]
    params = [torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=True) for w in base]
    depth = len(params) // 2 - 1
    t = torch.from_numpy(np.asarray(x, dtype=np.float64))
    for li in range(depth + 1):
        t = t @ params[2 * li] + params[2 * li + 1]
        if li < depth:
            t = fn(t)
    loss = torch.mean((torch.from_numpy(np.asarray(y, dtype=np.float64)) - t) ** 2)
    grads = torch.autograd.grad(loss, params)
    return ([(w - lr * g).detach().numpy() for w, g in zip(params, grads)], [lr * g.numpy() for g in grads])


@functools.lru_cache(maxsize=None)
def reference(name, salt=0):
    """The float64 judge of a row, computed once: per task (adapted parameters, steps).  Callers must not write into it."""
    row = BY_NAME[name]
    inp = inputs(row, salt)
    return [autograd_step(inp["base"], inp["x"][e], inp["y"][e], row.act, row.lr) for e in range(row.m)]


def bar(step):
    """The project's bar for an adapted tensor against the float64 step (tests/test_gpu_random_shapes.py)."""
    return 3e-5 * max(step, 1e-3) + 2e-7


MIN_STEP = 2.5e-4       # every parameter tensor of every task of every row moves by at least this much (max |lr g|, float64)
