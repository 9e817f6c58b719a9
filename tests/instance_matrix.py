"""One row per compiled rollout-kernel instance: the table behind tests/test_instance_matrix.py (routing, no GPU) and
tests/test_gpu_instance_matrix.py (every row against the float64 oracle).

The rollout kernels are templates; the launcher picks an instance from the observation / action widths, the hidden width, the
depth, the activation and the plan size.  ``ENUMERATED`` writes out, unit by unit, what ``csrc/l2a_mfma_inst.hip``,
``csrc/l2a_micro_inst.hip`` and ``csrc/l2a_lstm_inst.hip`` name; ``UNREACHABLE`` lists the members of that cross product no
launch can take (the sources guard them out, so they are not compiled); every other instance has at least one ``Row`` here
whose shape sits on an EDGE of its (OT, KG0) = (ceil(obs / 16), ceil((obs + act) / 16)) and whose plan is the smallest that
reaches its unit on a 256-CU device.

A row is (instance) -> (obs_dim, act_dim, hidden, activation, E, mode, m, n, h, policy); ``expect`` holds the fields of
``_lib.plan_geometry`` that identify the unit, ``reward`` the reward form ('vel': velocity of the LAST observation dim, the last
live unit of the last observation tile; 'dist': distance over the last three), ``valu`` marks the one row per unit and
(OT, KG0, variant) that is also compared with the generic VALU kernel.
"""

from collections import OrderedDict, namedtuple

Instance = namedtuple("Instance", "family unit ot kg0 variant gact n1")
Row = namedtuple("Row", "id instance obs_dim act_dim hidden activation E mode m n h policy expect reward valu")

H = 3           # the exchange buffers carry two step parities: the third step reuses the first one's
N_SMALL = 37    # three 16-candidate tiles, the last one ragged (ten micro tiles, the last one of one candidate)

# ---- the enumeration of instances, written out from the sources ---------------------------------------------------------------

# l2a_mfma_inst.hip, launch_shape: case ot * 8 + kg0
SHAPES = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (4, 5)]
SHAPES_NT2 = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3), (3, 4)]           # "#if L2A_INST_NT == 1" around OT = 4

# csrc/build.py INSTANCES, FAN_INSTANCES, WHOLE_INSTANCES: unit -> (NT, hidden width = 64 * TPW, geo of l2a_launch_mfma)
MFMA_UNITS = OrderedDict([
    ("1_2", (1, 128, 0)), ("1_4", (1, 256, 0)), ("1_8", (1, 512, 0)), ("2_2", (2, 128, 0)), ("2_4", (2, 256, 0)),
    ("fan_1_2", (1, 128, 1)), ("fan_1_4", (1, 256, 1)), ("fan_1_8", (1, 512, 1)), ("fan_2_8", (2, 512, 1)),
    ("whole_1_8", (1, 512, 2)), ("whole_2_8", (2, 512, 2)),
])


def _mfma_unit_instances(unit):
    nt = MFMA_UNITS[unit][0]
    out = []
    for ot, kg0 in (SHAPES if nt == 1 else SHAPES_NT2):
        out += [Instance("mlp", unit, ot, kg0, "", False, False),       # launch_one<OT, KG0, false>
                Instance("mlp", unit, ot, kg0, "", True, False),        # launch_one<OT, KG0, true>
                Instance("mlp", unit, ot, kg0, "", True, True)]         # one hidden layer: launch_one<OT, KG0, true, 4, true>
    out += [Instance("mlp", unit, 2, 2, "o4", False, False), Instance("mlp", unit, 2, 2, "o4", True, False),
            Instance("mlp", unit, 3, 4, "k0l1", False, False), Instance("mlp", unit, 3, 4, "k0l1", True, False)]
    return out


ENUMERATED = [i for unit in MFMA_UNITS for i in _mfma_unit_instances(unit)]
# l2a_micro_inst.hip: l2a_mlp_micro_k<UW, GACT>, l2a_lstm_micro_k<UW>
ENUMERATED += [Instance("mlp_micro", "uw%d" % uw, 0, 0, "", gact, False) for uw in (1, 2) for gact in (False, True)]
ENUMERATED += [Instance("lstm_micro", "uw%d" % uw, 0, 0, "", False, False) for uw in (1, 2)]
# l2a_lstm_inst.hip: l2a_lstm_mfma_k<1, UTW, OT, KG0, SPLIT>
ENUMERATED += [Instance("lstm", "utw%d" % utw, ot, kg0, variant, False, False)
               for utw in (2, 4, 8) for ot, kg0 in SHAPES for variant in ("whole", "split")]

# Members of the cross product no launch takes, each with the condition that excludes it.  The instance sources guard
# exactly these out (l2a_mfma_inst.hip: `L2A_INST_FAN != 2` around the OT = 4 cases, `if constexpr (!GACT)` around K0L = 1).
UNREACHABLE = OrderedDict()
for _ot, _kg0 in ((4, 4), (4, 5)):
    for _gact, _n1 in ((False, False), (True, False), (True, True)):
        UNREACHABLE[Instance("mlp", "whole_1_8", _ot, _kg0, "", _gact, _n1)] = \
            "l2a_api.hip:395 - the whole-tiles route of one tile per workgroup requires OT <= 3"
for _unit in MFMA_UNITS:
    UNREACHABLE[Instance("mlp", _unit, 3, 4, "k0l1", True, False)] = \
        "l2a_mfma_inst.hip:52 - K0L = 1 is chosen for the fast activations only (no line of l2a_api.hip: the unit's own switch)"

COMPILED = [i for i in ENUMERATED if i not in UNREACHABLE]

# ---- shapes on the edges of each (OT, KG0) ------------------------------------------------------------------------------------

_DIMS = {
    (1, 1): [(9, 7), (3, 1)],           # 16 inputs exactly; the smallest model
    (1, 2): [(16, 1)],                  # a full observation tile, one feature in the second k-group
    (2, 2): [(23, 7), (31, 1), (21, 11)],   # past the O4 range (obs - 16 > 4); 21 is the first width past it, 32 inputs exactly
    (2, 3): [(32, 1), (17, 16)],
    (3, 3): [(33, 15)],                 # 48 inputs exactly
    (3, 4): [(48, 16), (33, 16)],       # 64 inputs exactly; 49 inputs (generic activation / one hidden layer: not K0L = 1)
    (4, 4): [(49, 15)],
    (4, 5): [(64, 1), (64, 16)],        # the widest model
}
_DIMS_O4 = [(17, 15), (19, 1)]          # one and three live units in the quarter tile (20 + 6, four, is the HalfCheetah golden)
_DIMS_K0L1 = [(48, 1), (33, 16), (41, 8)]   # in_dim == 49 with three boundaries between observation and action features


def dims_for(inst):
    if inst.variant == "o4":
        return list(_DIMS_O4)
    if inst.variant == "k0l1":
        return list(_DIMS_K0L1)
    dims = list(_DIMS[(inst.ot, inst.kg0)])
    if (inst.ot, inst.kg0) == (3, 4) and not inst.gact:
        dims = [(48, 16)]               # 33 + 16 with relu is the K0L = 1 instance
    if (inst.ot, inst.kg0) == (2, 2) and inst.n1:
        dims.append((17, 15))           # one hidden layer: no O4 instance, the quarter-tile shape runs the plain one
    if inst.family == "lstm" and (inst.ot, inst.kg0) == (2, 2):
        dims.append((17, 15))
    if inst.family == "lstm" and (inst.ot, inst.kg0) == (3, 4):
        dims.append((48, 1))
    return dims


def dispatched_instance(family, unit, obs_dim, act_dim, depth, activation):
    """What launch_shape / launch_one of l2a_mfma_inst.hip select inside a unit (restated: the kernels are not introspectable)."""
    ot, kg0 = (obs_dim + 15) // 16, (obs_dim + act_dim + 15) // 16
    n1 = depth == 1
    gact = n1 or activation not in ("relu", "identity")
    variant = ""
    if not n1 and (ot, kg0) == (2, 2) and 1 <= obs_dim - 16 <= 4:
        variant = "o4"
    if not n1 and (ot, kg0) == (3, 4) and not gact and obs_dim + act_dim == 49:
        variant = "k0l1"
    return Instance(family, unit, ot, kg0, variant, gact, n1)


# ---- plans and policies that reach each unit ----------------------------------------------------------------------------------

def _geo(nt=1, split=0, fan=False, whole=False, front=0, kernel="mfma16"):
    return dict(kernel=kernel, nt=nt, split=split, fan=fan, whole_instance=whole, front_workgroups=front)


def _pol(split=1, fan=1, micro=0, double=1):
    return dict(split=split, fan=fan, micro=micro, double=double)


def _plans(unit, depth):
    """[(plan name, E, mode, n, policy, expected geometry)] of a unit: every launch flavour its instances serve."""
    nt, _, geo = MFMA_UNITS[unit]
    if geo == 0 and nt == 1:
        plans = [
            # one workgroup per tile (width 512: without the double-round policy, or a single model takes whole_1_8)
            ("unsplit", 1, "single", N_SMALL, _pol(split=0, fan=0, double=0 if unit == "1_8" else 1), _geo()),
            # two workgroups per tile, whole sets each
            ("wholeset", 2, "mean", N_SMALL, _pol(split=2), _geo(split=1)),
        ]
        if depth >= 2:      # ... sharing the only set: each runs half of the last hidden layer and of the output layer
            plans.append(("half", 1, "single", N_SMALL, _pol(split=1, fan=0), _geo(split=2)))
        return plans
    if geo == 0:            # 512 tiles: one round of double tiles (1.9) beats two rounds of single ones
        return [("double", 1, "single", 8192, _pol(), _geo(nt=2))]
    if geo == 1 and nt == 1:
        return [("fan", 3, "mean", N_SMALL, _pol(), _geo(split=3, fan=True))]
    if geo == 1:            # 90 tiles x 3 members > 256 CUs, 45 double tiles x 3 fit
        return [("fan2", 3, "mean", 1430, _pol(), _geo(nt=2, split=3, fan=True))]
    if nt == 1:
        return [("whole", 1, "single", N_SMALL, _pol(split=0), _geo(whole=True))]
    return [("allfront", 1, "single", 8192, _pol(), _geo(nt=2, whole=True))]        # 512 tiles: all on double tiles


def _row(inst, obs_dim, act_dim, depth, activation, plan, reward="vel", valu=False):
    name, E, mode, n, policy, expect = plan
    hidden = [MFMA_UNITS[inst.unit][1]] * depth if inst.family == "mlp" else None
    rid = "%s-%s-ot%dkg%d%s-%s%s-o%da%d-%s-d%d-%s%s%s" % (
        inst.family, inst.unit, inst.ot, inst.kg0, "-" + inst.variant if inst.variant else "", "g" if inst.gact else "f",
        "-n1" if inst.n1 else "", obs_dim, act_dim, activation, depth, name, "-E%d" % E if E > 1 else "",
        "-dist" if reward == "dist" else "")
    return Row(rid, inst, obs_dim, act_dim, hidden, activation, E, mode, 1, n, H, policy, expect, reward, valu)


def _mlp_rows():
    rows = []
    for unit in MFMA_UNITS:
        nt, _, geo = MFMA_UNITS[unit]
        valu_done = set()
        for inst in _mfma_unit_instances(unit):
            if inst in UNREACHABLE:
                continue
            depth = 1 if inst.n1 else 2
            for k, (od, ad) in enumerate(dims_for(inst)):
                # one hidden layer: the instance serves both activation families
                activation = ("relu", "tanh")[k % 2] if inst.n1 else "tanh" if inst.gact else "relu"
                plans = _plans(unit, depth)
                for plan in plans:
                    # the VALU comparison rides on the unit's last launch flavour (general units: the shared half member)
                    key = (inst.ot, inst.kg0, inst.variant)
                    valu = key not in valu_done and plan is plans[-1]
                    if valu:
                        valu_done.add(key)
                    rows.append(_row(inst, od, ad, depth, activation, plan, valu=valu))
            # the distance reward on one row per (OT, KG0): the plain relu instance, its first shape, the unit's last flavour
            if inst.variant == "" and not inst.gact:
                od, ad = dims_for(inst)[0]
                rows.append(_row(inst, od, ad, 2, "relu", _plans(unit, 2)[-1], reward="dist"))
        # three hidden layers, so that the inner-layer loop runs: the quarter-tile shape with three live units; on the general
        # units an odd ensemble under the tile split (groups + the shared middle set)
        o4 = Instance("mlp", unit, 2, 2, "o4", False, False)
        plan = _plans(unit, 3)[-1]
        if geo == 0 and nt == 1:
            plan = ("half", 3, "mean", N_SMALL, _pol(split=1, fan=0), _geo(split=2))
        rows.append(_row(o4, 19, 1, 3, "relu", plan))
        if geo == 1:        # five members: 3 x 5 workgroups; two-tile fan: 45 x 5 <= 256 (OT <= 2: every member's term fits the LDS)
            plain = Instance("mlp", unit, 2, 2, "", False, False)
            name, _, mode, n, policy, expect = _plans(unit, 2)[-1]
            rows.append(_row(plain, 23, 7, 2, "relu", (name, 5, mode, n, policy, expect)))
        if unit == "whole_2_8":     # 549 tiles: 512 in front on double tiles, a rest launch of 37 whole tiles behind them
            k0l1 = Instance("mlp", unit, 3, 4, "k0l1", False, False)
            rows.append(_row(k0l1, 41, 8, 2, "relu",
                             ("front+rest", 1, "single", 8192 + 37 * 16, _pol(split=0), _geo(nt=1, whole=True, front=256))))
    return rows


def _micro_rows():
    rows = []
    for uw, width in ((1, 256), (2, 512)):
        for gact in (False, True):
            inst = Instance("mlp_micro", "uw%d" % uw, 0, 0, "", gact, False)
            shapes = [(3, 1, 2), (17, 15, 2), (19, 1, 2), (41, 8, 2), (64, 16, 3), (21, 11, 2)]      # (obs, act, depth)
            if gact:
                shapes.append((33, 16, 1))      # one hidden layer runs the generic-activation instance
            for k, (od, ad, depth) in enumerate(shapes):
                activation = "tanh" if gact and depth > 1 else "relu"
                rid = "mlp_micro-uw%d-%s-o%da%d-%s-d%d" % (uw, "g" if gact else "f", od, ad, activation, depth)
                rows.append(Row(rid, inst, od, ad, [width] * depth, activation, 1, "single", 1, N_SMALL, H,
                                _pol(micro=2), _geo(nt=0, kernel="micro"), "dist" if k == 3 else "vel", k == 0))
    return rows


def _lstm_rows():
    rows = []
    for utw in (2, 4, 8):
        for ot, kg0 in SHAPES:
            for variant in ("whole", "split"):
                inst = Instance("lstm", "utw%d" % utw, ot, kg0, variant, False, False)
                for od, ad in dims_for(inst):
                    rid = "lstm-utw%d-ot%dkg%d-%s-o%da%d" % (utw, ot, kg0, variant, od, ad)
                    rows.append(Row(rid, inst, od, ad, 64 * utw, "tanh", 1, "single", 1, N_SMALL, H,
                                    _pol(split=1 if variant == "split" else 0, micro=0), None, "vel", False))
    for uw, units in ((1, 256), (2, 512)):
        inst = Instance("lstm_micro", "uw%d" % uw, 0, 0, "", False, False)
        for k, (od, ad) in enumerate([(3, 1), (17, 15), (41, 8), (64, 16)]):
            rid = "lstm_micro-uw%d-o%da%d" % (uw, od, ad)
            rows.append(Row(rid, inst, od, ad, units, "tanh", 1, "single", 1, N_SMALL, H, _pol(micro=2), None,
                            "dist" if k == 2 else "vel", False))
    return rows


MLP_ROWS = _mlp_rows() + _micro_rows()
LSTM_ROWS = _lstm_rows()
ROWS = MLP_ROWS + LSTM_ROWS

# ---- the generic recurrent kernel: one row per run-time branch -------------------------------------------------------------------
#
# l2a_rnn_mfma_k (csrc/l2a_rnn_mfma.h) is not templated over the model: it branches at run time on each layer's width
# (UT = ceil(U / 16) unit tiles, KGx = ceil(inputs / 16) input k-groups).  A row is the smallest model that reaches a branch;
# every row also runs on l2a_rnn_valu_k.  ``why`` names the line of l2a_rnn_mfma.h the row is there for.
GenericRow = namedtuple("GenericRow", "id cell obs_dim act_dim units activation reward why")
GENERIC_M, GENERIC_N = 2, N_SMALL


def _generic(cell, obs_dim, act_dim, units, activation, why, reward="vel"):
    rid = "%s-%s-o%da%d-%s" % (cell, "x".join(str(u) for u in units), obs_dim, act_dim, activation)
    return GenericRow(rid, cell, obs_dim, act_dim, tuple(units), activation, reward, why)


GENERIC_ROWS = [
    # width classes (20 + 6 inputs: KGx = 2).  UT = 8: ring of 10 k-groups, tail 2
    _generic("gru", 20, 6, [120], "tanh", ":339 prod2 and :307 prod1 with TB = 2, UT even"),
    _generic("rnn", 20, 6, [120], "relu", ":307 prod1 with TB = 2, UT even"),
    # UT = 9: the last block of two reads a zero tile (:302, :322 skip it); ring of 11, tail 3
    _generic("gru", 20, 6, [130], "sigmoid", ":339 / :307 TB = 2, UT odd: :322 and :302 skip the zero tile"),
    _generic("rnn", 20, 6, [130], "tanh", ":307 TB = 2, UT odd: :302 skips the zero tile"),
    # UT = 17 (41 + 8 inputs: KGx = 4; ring of 21, tail 1): four tiles per call, the last block holds three zero tiles; the GRU
    # gates stay at two tiles per call with an odd UT
    _generic("gru", 41, 8, [264], "tanh", ":306 prod1 with TB = 4, three zero tiles; :339 TB = 2 with UT odd", "dist"),
    _generic("rnn", 41, 8, [264], "swish", ":306 prod1 with TB = 4, three zero tiles"),
    # a stack of LSTM layers whose top width has U % 4 != 0: a lane's f32x4 of c / h is partly live (:278, :283); rings of 7 and 7
    _generic("lstm", 20, 6, [72, 23], "tanh", ":262 LSTM blocks, :278 `live` inside an f32x4"),
    # 16 inputs exactly, one unit tile: a ring of TWO k-groups (:97 clamps the third request), an output layer of ONE (:383)
    _generic("gru", 9, 7, [16], "tanh", ":97 ring clamp with KGx + UT = 2; :383 output layer of a single k-group"),
    # three layers of different widths: rings of 5 (tail 1), 12 (tail 0) and 11 (tail 3); the input stride changes per layer (:370)
    _generic("rnn", 20, 6, [40, 130, 24], "tanh", ":124 ring with no tail (3 + 9 k-groups); :370-372 a new input stride per layer"),
    # 40 action dims: no prefetch, the actions are read in place (ring of 8, tail 0)
    _generic("gru", 20, 40, [64], "tanh", ":208 apf off, :234 actions read in place"),
    # 65 observation dims: five observation tiles for four waves - wave 0 takes tiles 0 and 4; the reward reads dim 64
    _generic("gru", 65, 3, [48], "tanh", ":380 a fifth observation tile (wave 0: c = 0 and c = 4)"),
]


def generic_rings(row):
    """KGx + UT of every layer's product and the k-groups of the output layer: the lengths of the operand rings of a row."""
    kin, out = row.obs_dim + row.act_dim, []
    for u in row.units:
        out.append((kin + 15) // 16 + (u + 15) // 16)
        kin = u
    return out, (kin + 15) // 16
