"""One row or more per launch geometry of the reward-model scorer (``l2a_score_mlp_k``): the table behind
the routing test in tests/test_reward_model.py (no GPU) and tests/test_reward_model_geometries_gpu.py (every row against the
float64 restatement and against the geometry-free bits of ``predict``).

The launcher picks ``(RT, CT, S)``: ``RT`` row tiles of 16 rows per pass, of them ``CT`` candidate tiles x ``S`` steps; a horizon
longer than ``S`` takes ``ceil(h / S)`` passes, the last one possibly ragged.  ``RT`` is bounded by the widest hidden layer
(``RT * width / 64 <= 32``) and the LDS image; ``CT > 1`` is taken only when one 16-candidate tile per workgroup would need more
than one round of workgroups, i.e. when ``rows = m * n > 16 * CUs``.

A row is ``(id, obs, act, hidden, activation, m, a, b, h, expect)``: the plan has ``m * n >= a * 16 * cus + b`` rows on a device of
``cus`` compute units (``plan_n``), ``expect`` is the ``(RT, CT, S)`` the row is there for - the same at 32, 64, 256 and 304 CUs
(asserted without a GPU against ``l2a_reward_model_geometry``).  ``b = 37`` leaves the last workgroup with one ragged candidate
tile and, at ``CT >= 2``, with empty ones.  ``m = 3`` puts env boundaries inside a workgroup.  Rows with many candidates keep to
one or two hidden layers: their float64 restatement on the host is what a test's time goes to.
"""

from collections import namedtuple

Row = namedtuple("Row", "id obs act hidden activation m a b h expect")

CUS = (32, 64, 256, 304)            # device sizes at which every row's geometry is asserted without a GPU
LDS = 160 * 1024                    # bytes of LDS a gfx950 workgroup may take
B = 37

ROWS = [
    # ---- width 64 (TPW 1): all ten (RT, CT, S) -----------------------------------------------------------------------------
    Row("g111_h1", 3, 1, (64,), "identity", 1, 0, B, 1, (1, 1, 1)),
    Row("g212_h2", 17, 5, (64, 64), "relu", 1, 0, B, 2, (2, 1, 2)),
    Row("g414_h10", 20, 6, (64,), "tanh", 1, 0, B, 10, (4, 1, 4)),                  # 3 passes, the last of 2
    Row("g818_h13_m3", 41, 8, (64, 64), "sigmoid", 3, 0, B, 13, (8, 1, 8)),         # 2 passes, the last of 5
    Row("g818_h30", 20, 6, (64,), "swish", 1, 0, B, 30, (8, 1, 8)),                 # 4 passes, the last of 6: config 2's horizon
    Row("g221_h1_m3", 3, 1, (64,), "relu", 3, 1, B, 1, (2, 2, 1)),
    Row("g422_h5", 17, 5, (64,), "tanh", 1, 1, B, 5, (4, 2, 2)),                    # 3 passes, the last of 1
    Row("g824_h10", 20, 6, (64, 64), "identity", 1, 1, B, 10, (8, 2, 4)),           # 3 passes, the last of 2
    Row("g441_h1_m3_kg0", 64, 16, (64,), "sigmoid", 3, 2, B, 1, (4, 4, 1)),         # kgs = KG0 = 9: the first layer is the widest
    Row("g441_h3", 41, 8, (64,), "swish", 1, 3, B, 3, (4, 4, 1)),                   # 3 passes with S = 1
    Row("g842_h9", 20, 6, (64,), "relu", 1, 2, B, 9, (8, 4, 2)),                    # 5 passes, the last of 1
    Row("g881_h1_m3", 20, 6, (64,), "tanh", 3, 4, B, 1, (8, 8, 1)),                 # through score_trajectory
    Row("g881_h1_predict", 20, 6, (64,), "tanh", 1, 4, B, 1, (8, 8, 1)),            # its twin through predict
    # ---- width 512 (TPW 8): RT <= 4, a 128 KiB image -----------------------------------------------------------------------
    Row("w512_g414_h7", 64, 16, (512, 512), "swish", 1, 0, B, 7, (4, 1, 4)),        # 2 passes, the last of 3
    Row("w64x512_g422_h5", 20, 6, (64, 512), "relu", 1, 1, B, 5, (4, 2, 2)),        # unequal widths, 3 passes, the last of 1
    Row("w512x64_g441_h1", 17, 5, (512, 64), "sigmoid", 1, 2, B, 1, (4, 4, 1)),     # unequal widths
    # ---- the other widths -----------------------------------------------------------------------------------------------------
    Row("w320_g414_h6", 41, 8, (320,), "identity", 1, 0, B, 6, (4, 1, 4)),          # TPW 5, 2 passes, the last of 2
    Row("w256_g818_h20", 20, 6, (256, 256), "tanh", 1, 0, B, 20, (8, 1, 8)),        # 128 KiB image at RT = 8, 3 passes, the last of 4
    Row("w192_g818_h13", 3, 1, (192,), "relu", 1, 0, B, 13, (8, 1, 8)),             # TPW 3, 2 passes, the last of 5
    Row("w384_g414_h7", 17, 5, (384,), "sigmoid", 1, 0, B, 7, (4, 1, 4)),           # TPW 6, 2 passes, the last of 3
    Row("w128x448x64_g414_h5", 20, 6, (128, 448, 64), "swish", 1, 0, B, 5, (4, 1, 4)),     # TPW 2, 7, 1; 2 passes, the last of 1
]

PREDICT = ("g881_h1_predict",)      # rows scored with l2a_reward_model_predict (h = 1, per-row observations)

# every (RT, CT, S) with S | RT the launcher can pick
GEOMETRIES = [(rt, rt // s, s) for rt in (8, 4, 2, 1) for s in (8, 4, 2, 1) if s <= rt]


def plan_n(row, cus):
    """Candidates per env: ``m * n >= a * 16 * cus + b``; for ``m > 1`` the smallest such ``n`` that is no multiple of 16."""
    need = row.a * 16 * cus + row.b
    n = (need + row.m - 1) // row.m
    if row.m > 1 and n % 16 == 0:
        n += 1
    return n


def by_id(rid):
    return next(r for r in ROWS if r.id == rid)
