"""One row per body of the generic recurrent micro-tile kernel: the table behind tests/test_rnn_micro_matrix.py (enumeration,
routing and the oracle's margins, no GPU) and tests/test_gpu_rnn_micro_matrix.py (every row against the float64 oracle and the
16-candidate kernel).

``l2a_rnn_micro_k<UW, CELL, MTM>`` (csrc/l2a_rnn_micro.h) is compiled eight times by csrc/l2a_rnn_micro_inst.hip and dispatches on
the workgroup's micro-tile count to ``l2a_rnn_micro_body<MT, UW, CELL, MTM>``, MT = 1 .. MTM: 27 bodies, each with its own
register allocation, operand-ring depth and LDS layout.  ``RNN_MICRO_ENUMERATED`` writes the 27 (UW, cell, MTM, MT) pairs out;
``UNREACHABLE`` would list the pairs the deal ``l2a_deal_micro`` (csrc/l2a_host.h) never produces, with the arithmetic reason; it
is empty - test_rnn_micro_matrix.py exhausts the deal - and every pair has rows here.

A row is (instance, the bodies ``mts`` its one launch runs) -> cell, layers, obs_dim, act_dim, activation, m, n, h, reward
('vel': velocity of the LAST observation dim; 'dist': distance over the last three, as in tests/instance_matrix.py) and a
``salt`` of the inputs' seed (see ``SALTS``).  The plans are the smallest that reach their bodies on a 256-CU device; the nine
input shapes of ``EDGES`` are spread over the rows so that every INSTANCE (not every body) sees each of them.
"""

from collections import OrderedDict, namedtuple

Instance = namedtuple("Instance", "uw cell mtm")
Plan = namedtuple("Plan", "name m n mtm mts")
Row = namedtuple("Row", "id instance mts cell units obs_dim act_dim activation m n h reward salt")

H = 3           # the hidden-state rows carry two step parities: the third step reuses the first one's

# ---- the enumeration, written out from the sources -------------------------------------------------------------------------------

# l2a_rnn_micro_inst.hip, l2a_launch_rnn_micro: launch_rnn<UW, CELL, MTM>
INSTANCES = [
    Instance(1, "lstm", 3), Instance(1, "gru", 3), Instance(1, "rnn", 3),       # units == 256 && mtm == 3
    Instance(1, "lstm", 4), Instance(1, "gru", 4), Instance(1, "rnn", 4),       # units == 256 && mtm == 4
    Instance(2, "gru", 3), Instance(2, "rnn", 3),                               # units == 512 && mtm == 3
]
# l2a_rnn_micro.h, l2a_rnn_micro_k: `if constexpr (MTM == 4)` body<4>, then body<3>, body<2>, body<1>
RNN_MICRO_ENUMERATED = [(i.uw, i.cell, i.mtm, mt) for i in INSTANCES for mt in range(1, i.mtm + 1)]

# The deal (l2a_deal_micro through plan_rnn_launch, l2a_lstm_api.hip) takes the four-tile instances only when three micro tiles
# per workgroup do not hold the plan.  With at most as many envs as CUs that is quads = ceil(n / 4) > 3 W0, W0 = CUs / m >= 1,
# so quads >= 4; it then deals W = ceil(quads / 4) workgroups of hi = ceil(quads / W) and hi - 1 micro tiles, and
# W < quads / 4 + 1 gives quads / W > 4 quads / (quads + 4) >= 2 with equality only at quads = 4, where W = 1 and hi = 4: hi >= 3,
# every workgroup holds at least two micro tiles, and MT = 2 runs for quads = 5 alone (W = 2, hi = 3: one workgroup of three
# and one of two), which needs W0 = 1 - more than half as many envs as CUs.  So no plan of m <= CUs envs runs MT = 1 in an
# MTM = 4 instance.  A plan of MORE envs than CUs does: W0 = 0 is "no deal of three" whatever n is, the forced deal gives each
# env ceil(quads / 4) workgroups, and quads = 1 is one workgroup of ONE micro tile on the four-tile instance (m = 257, n <= 4).
# Every compiled body is therefore reachable; the dict stays for the day a pair is not.
UNREACHABLE = OrderedDict()

REACHABLE = [p for p in RNN_MICRO_ENUMERATED if p not in UNREACHABLE]

# ---- plans: (m, n) -> the launch's instance width mtm and the workgroup sizes it deals on 256 CUs --------------------------------
# every n leaves the last micro tile ragged (n % 4 == 1: one candidate in the last quad; mt1of4: three)
PLANS3 = [
    Plan("mt1", 2, 37, 3, (1,)),            # ten quads on ten workgroups per env
    Plan("mt32", 64, 37, 3, (3, 2)),        # ten quads on four workgroups: 3, 3, 2, 2
    Plan("mt21", 64, 25, 3, (2, 1)),        # seven quads on four workgroups: 2, 2, 2, 1
]
PLANS4 = [
    Plan("mt43", 65, 37, 4, (4, 3)),        # three workgroups per env hold nine quads of ten: the forced deal is 4, 3, 3
    Plan("mt32of4", 129, 17, 4, (3, 2)),    # one workgroup per env, five quads: the forced deal is 3, 2 (two rounds of 129)
    Plan("mt1of4", 257, 3, 4, (1,)),        # more envs than CUs: no deal of three; one quad (of three candidates) per env
]

# ---- the input edges: (obs_dim, act_dim) -> what the shape exercises ----------------------------------------------------------------
EDGES = OrderedDict([
    ((3, 1), "the smallest model"),
    ((9, 7), "16 inputs exactly, KG0 = 1 padded to 2"),
    ((16, 1), "ga0 = 1: the first action slot is a group of its own"),
    ((17, 16), "KG0 = 3 padded to 4, actions across two groups"),
    ((33, 15), "48 inputs exactly"),
    ((48, 16), "64 inputs exactly"),
    ((49, 15), "OT = 4"),
    ((64, 1), "KG0 = 5 padded to 6"),
    ((64, 16), "every limit"),
])
DIST_EDGES = (3, 8)             # the distance reward on (17, 16) and (64, 16); the velocity reward on the other shapes
ACTIVATIONS = ("tanh", "relu", "swish")     # l2a_fast_tanh | l2a_act1 with a kink | l2a_act1 with a sigmoid

# ---- depths: the layers of the rows of an instance (checked against the launcher in test_rnn_micro_matrix.py: the deepest
#      stack it still gives micro tiles is among them; one LSTM layer is the tuned kernel's model, not this kernel's) -----------------
DEPTHS = OrderedDict([
    (Instance(1, "lstm", 3), (2, 3)), (Instance(1, "gru", 3), (1, 2, 3)), (Instance(1, "rnn", 3), (1, 2, 3)),
    # LDS rows for sixteen candidates: two GRU / LSTM layers, three BasicRNN ones
    (Instance(1, "lstm", 4), (2,)), (Instance(1, "gru", 4), (1, 2)), (Instance(1, "rnn", 4), (1, 2, 3)),
    (Instance(2, "gru", 3), (1,)), (Instance(2, "rnn", 3), (1,)),
])

# Seeds of the inputs: a row's inputs are drawn from (row id, salt).  The salt is the smallest for which the float64 oracle
# separates every env's two best returns by MARGIN (test_rnn_micro_matrix.py asserts it for every row) - a condition on the
# inputs, so that the arg-max assertions of the GPU file do not hang on a rounding.
SALTS = {
    "uw1-lstm-mtm3-mt21-d2-o16a1-swish": 1,
    "uw1-lstm-mtm3-mt21-d3-o48a16-tanh": 1,
    "uw1-lstm-mtm3-mt32-d2-o64a1-tanh": 3,
    "uw1-lstm-mtm3-mt21-d2-o64a16-relu-dist": 1,
    "uw1-gru-mtm3-mt32-d3-o64a1-tanh": 3,
    "uw1-gru-mtm3-mt21-d3-o64a16-relu-dist": 1,
    "uw1-rnn-mtm3-mt21-d3-o64a16-relu-dist": 1,
    "uw1-lstm-mtm4-mt43-d2-o3a1-tanh": 1,
    "uw1-lstm-mtm4-mt32of4-d2-o9a7-relu": 1,
    "uw1-lstm-mtm4-mt1of4-d2-o16a1-swish": 2,
    "uw1-lstm-mtm4-mt32of4-d2-o33a15-swish": 1,
    "uw1-lstm-mtm4-mt32of4-d2-o64a1-tanh": 3,
    "uw1-gru-mtm4-mt32of4-d1-o9a7-relu": 1,
    "uw1-gru-mtm4-mt32of4-d1-o64a1-tanh": 7,
    "uw2-gru-mtm3-mt32-d1-o64a1-tanh": 1,
    "uw2-rnn-mtm3-mt21-d1-o64a16-relu-dist": 1,
}


def _rows():
    rows = []
    for inst in INSTANCES:
        plans = PLANS3 if inst.mtm == 3 else PLANS4
        depths = DEPTHS[inst]
        for k, (od, ad) in enumerate(EDGES):
            plan = plans[k % len(plans)]
            depth = depths[(k // len(plans)) % len(depths)]
            activation = ACTIVATIONS[(k + k // 3) % 3]
            reward = "dist" if k in DIST_EDGES else "vel"
            rid = "uw%d-%s-mtm%d-%s-d%d-o%da%d-%s%s" % (inst.uw, inst.cell, inst.mtm, plan.name, depth, od, ad, activation,
                                                       "-dist" if reward == "dist" else "")
            rows.append(Row(rid, inst, plan.mts, inst.cell, (256 * inst.uw,) * depth, od, ad, activation, plan.m, plan.n, H,
                            reward, SALTS.get(rid, 0)))
    return rows


ROWS = _rows()

# ---- a second set_weights: one model per cell type and width, on the MT = 1 plan -------------------------------------------------
RefreshRow = namedtuple("RefreshRow", "id cell units obs_dim act_dim activation m n h reward salt")
REFRESH_ROWS = [
    RefreshRow("refresh-%s-%s" % (cell, "x".join(str(u) for u in units)), cell, units, 17, 16, "tanh", PLANS3[0].m, PLANS3[0].n, H,
               "vel", 0)
    for cell, units in (("lstm", (256, 256)), ("gru", (256,)), ("rnn", (256,)), ("gru", (512,)), ("rnn", (512,)))
]


def workgroup_sizes(geometry):
    """The micro-tile counts of the workgroups of a launch (l2a_rnn_micro_k: mc_r workgroups of mc_hi, the other mc_w - mc_r
    of mc_hi - 1)."""
    sizes = {geometry["mc_hi"]}
    if geometry["mc_r"] < geometry["mc_w"]:
        sizes.add(geometry["mc_hi"] - 1)
    return sizes
