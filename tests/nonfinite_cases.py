"""Diverged rollouts with a known outcome: seeded MLP models, norms, start states and candidate actions whose returns fall
into chosen classes - finite, +inf, -inf, NaN - at chosen candidates.  CPU-importable (NumPy only): the fixtures'
self-checks run without a GPU (test_nonfinite_cases.py), the comparisons with the kernels in test_gpu_nonfinite.py.

The divergence is injected as an infinite ACTION feature at one step, so inf and NaN arise by exact IEEE arithmetic in
fp32 and in float64 alike, while every finite candidate stays many orders of magnitude below the fp32 range: rounding
cannot move a candidate from one class to another.  Hidden units are split into four classes by u % 4; action k = 0, 1, 2
carries a weight of +S into units of class k and -S into all others (a zero weight would give inf x 0 = NaN everywhere):

* a0 = +inf  -> class-0 units +inf, the rest -inf -> relu 0; hidden layers keep the block structure (+S inside a class,
  -S across) and the velocity column of the output layer is +S on class 0: delta_vel = +inf -> return +inf;
* a1 = +inf  -> the same through class 1, output column -S on class 1: return -inf;
* a2 = +inf  -> class 2, output column of alternating sign: inf - inf in the OUTPUT pre-activation (identity layer) -> NaN;
* a0 = a1 = +inf -> inf - inf in the first HIDDEN pre-activation of classes 0 and 1 -> relu(NaN) = NaN in np.maximum /
  torch.relu -> return NaN (an fmaxf-style relu would give 0 there and a finite return).

Kinds: ``mixed`` (a: all four classes, the first NaN past the first 16-candidate tile), ``inf`` (b: +-inf only, the
arg-max is the first +inf), ``hidden_nan`` / ``out_nan`` (c: NaN from one hidden / output pre-activation only) - the
divergence at the LAST step, so that the velocity reward sees a finite previous state - and ``onesign`` (d: every weight
positive, a0 = +inf at step 0, distance reward with a negative coefficient: the state is +inf in every dimension for the
rest of the horizon and the return +inf, never NaN; obs_dim off a multiple of 16 puts padding lanes next to it) - and
``vel``: the same all-positive model under the VELOCITY reward, diverging at step 0 of several: the oracle's reward
``next - obs`` is +inf at step 0 and inf - inf = NaN from step 1 on, so the return is NaN (a kernel that takes the
velocity from the delta alone would report +inf).
"""

import numpy as np

from learning_to_adapt_amd.envs import RewardSpec
from learning_to_adapt_amd.utils import synthetic
from oracle import OracleMLPDynamics
from oracle.planner import rollout_returns

FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+inf", "-inf", "nan")
KINDS = ("mixed", "inf", "hidden_nan", "out_nan", "onesign", "vel")
MARGIN = 1e30           # every finite candidate's states and return stay below this (fp32 overflows at 3.4e38)
_S = 0.25

# candidate -> injection, per kind (env i shifts the first entry by i: per-env arg-max differs)
_PLACES = {
    "mixed": {"pos": [3, 40], "neg": [5, 61], "out_nan": [37, 80], "hid_nan": [50]},
    "inf": {"pos": [21, 70], "neg": [4, 90]},
    "hidden_nan": {"hid_nan": [33, 71]},
    "out_nan": {"out_nan": [45, 77]},
    "onesign": {"pos": [18, 52]},
    "vel": {"vel_nan": [26, 63]},
}
_EXPECT = {"pos": POS_INF, "neg": NEG_INF, "out_nan": NAN, "hid_nan": NAN, "vel_nan": NAN}


def classify(x):
    """Class code per element: FINITE, POS_INF, NEG_INF or NAN."""
    x = np.asarray(x)
    c = np.full(x.shape, FINITE, dtype=np.int8)
    c[np.isposinf(x)] = POS_INF
    c[np.isneginf(x)] = NEG_INF
    c[np.isnan(x)] = NAN
    return c


def _block_set(obs_dim, act_dim, hidden, seed, onesign):
    rs = np.random.RandomState(seed)
    params = synthetic.make_weight_set(obs_dim, act_dim, hidden, seed)
    if onesign:     # every weight positive: an infinite input can only give +inf downstream
        out = []
        for li in range(0, len(params), 2):
            w = params[li]
            out += [(rs.uniform(0.2, 1.0, w.shape) / w.shape[0]).astype(np.float32), params[li + 1]]
        return out
    cls = np.arange(hidden[0]) % 4
    w0 = params[0]
    for k in range(3):
        w0[obs_dim + k] = np.where(cls == k, _S, -_S).astype(np.float32)
    for li in range(2, 2 * len(hidden), 2):
        w = params[li]
        for k in range(3):
            w[cls == k] = np.where(cls == k, _S, -_S).astype(np.float32) / len(cls)
    wout = params[-2]
    vel = obs_dim - 1
    wout[cls == 0, vel] = _S
    wout[cls == 1, vel] = -_S
    wout[cls == 2, vel] = np.where(np.arange(np.sum(cls == 2)) % 2 == 0, _S, -_S)
    return params


def mlp_case(kind, obs_dim=20, act_dim=6, width=128, depth=2, mode="single", E=1, m=1, n=100, h=3, seed=0):
    """One fixture: a dict with the model (``sets``, ``norms``, ``hidden``, ``mode``), the plan (``obs0`` [m, obs_dim],
    ``acts`` float64 [h, m * n, act_dim], ``spec``, ``discount``) and the intended classes ``pattern`` [m, n]."""
    assert kind in KINDS and act_dim >= 3 and n >= 100 and h >= (2 if kind == "vel" else 1)
    assert mode in ("single", "mean", "per_block") and (E == 1) == (mode == "single")
    if mode == "per_block":
        assert m == E
    hidden = [width] * depth
    onesign = kind in ("onesign", "vel")
    rs = np.random.RandomState(7000 + seed)
    low, high = -np.ones(act_dim), np.ones(act_dim)
    sets = [_block_set(obs_dim, act_dim, hidden, 31 * seed + e + 1, onesign) for e in range(E)]
    norms = [synthetic.make_norm(obs_dim, act_dim, low, high, 97 * seed + e) for e in range(E)]
    obs0 = rs.randn(m, obs_dim)
    acts = rs.uniform(low, high, (h, m * n, act_dim))
    if onesign:
        acts = np.abs(acts)
        spec = RewardSpec.make(dist_coef=-1.0, alive=0.05, dist_index=obs_dim - 3) if kind == "onesign" else \
            RewardSpec.make(w_vel=1.0, dt=0.05, alive=0.05, vel_index=obs_dim - 1)
        t_inj = 0
    else:
        spec = RewardSpec.make(w_vel=1.0, dt=0.05, alive=0.05, vel_index=obs_dim - 1)
        t_inj = h - 1
    pattern = np.full((m, n), FINITE, dtype=np.int8)
    for i in range(m):
        for what, idxs in _PLACES[kind].items():
            for r, j in enumerate(idxs):
                j = j + i if r == 0 else j
                row = i * n + j
                if what in ("pos", "hid_nan", "vel_nan"):
                    acts[t_inj, row, 0] = np.inf
                if what in ("neg", "hid_nan"):
                    acts[t_inj, row, 1] = np.inf
                if what == "out_nan":
                    acts[t_inj, row, 2] = np.inf
                pattern[i, j] = _EXPECT[what]
    return dict(kind=kind, obs_dim=obs_dim, act_dim=act_dim, hidden=hidden, mode=mode, E=E, m=m, n=n, h=h, sets=sets,
                norms=norms, obs0=obs0, acts=acts, spec=spec, discount=0.95, pattern=pattern, low=low, high=high)


def oracle_dynamics(case, mlp_dtype=np.float32):
    return OracleMLPDynamics(case["obs_dim"], case["act_dim"], case["sets"], case["norms"], mode=case["mode"],
                             hidden_nonlinearity="relu", mlp_dtype=mlp_dtype)


def oracle_returns(case, mlp_dtype=np.float32, track=None):
    """Float64 returns [m, n] of the oracle planner (fp32 MLP; ``mlp_dtype=np.float64``: float64 end to end).
    ``track`` (a list) receives every step's next states [m * n, obs_dim]."""
    dyn = oracle_dynamics(case, mlp_dtype)
    if track is not None:
        inner = dyn.predict

        def predict(obs, act):
            nxt = inner(obs, act)
            track.append(nxt)
            return nxt
        dyn.predict = predict
    with np.errstate(over="ignore", invalid="ignore"):
        r = rollout_returns(dyn, case["spec"].evaluate, case["obs0"], case["acts"], case["n"], case["discount"])
    return r.reshape(case["m"], case["n"])


# the sweep of test_gpu_nonfinite.py / the self-checks (kind, kwargs)
MLP_CASES = [
    ("mixed", dict(obs_dim=20, width=512, depth=2, mode="single", m=1, n=100, h=3)),
    ("mixed", dict(obs_dim=17, width=128, depth=3, mode="mean", E=3, m=2, n=100, h=2)),
    ("mixed", dict(obs_dim=41, width=96, depth=1, mode="per_block", E=2, m=2, n=130, h=2)),
    ("inf", dict(obs_dim=20, width=512, depth=1, mode="mean", E=5, m=1, n=100, h=2)),
    ("inf", dict(obs_dim=33, width=72, depth=2, mode="single", m=2, n=100, h=3)),
    ("hidden_nan", dict(obs_dim=20, width=512, depth=3, mode="single", m=2, n=100, h=2)),
    ("hidden_nan", dict(obs_dim=17, width=128, depth=1, mode="per_block", E=3, m=3, n=100, h=3)),
    ("out_nan", dict(obs_dim=20, width=512, depth=2, mode="mean", E=2, m=1, n=100, h=2)),
    ("out_nan", dict(obs_dim=41, width=96, depth=2, mode="single", m=1, n=100, h=2)),
    ("onesign", dict(obs_dim=20, width=512, depth=2, mode="single", m=2, n=100, h=4)),
    ("onesign", dict(obs_dim=17, width=128, depth=3, mode="mean", E=3, m=1, n=100, h=5)),
    ("onesign", dict(obs_dim=41, width=256, depth=1, mode="per_block", E=2, m=2, n=100, h=3)),
    # the micro-tile plan (5 x 500, h = 10 at width 512) and a plan with a double round (width 512, many tiles)
    ("mixed", dict(obs_dim=20, width=512, depth=2, mode="per_block", E=5, m=5, n=500, h=10)),
    ("onesign", dict(obs_dim=20, width=512, depth=1, mode="mean", E=2, m=2, n=2600, h=2)),
    # width 512, depth 2 off the 17 - 20 observation widths (no 4x4x1 output tile)
    ("mixed", dict(obs_dim=41, width=512, depth=2, mode="single", m=1, n=100, h=3)),
    ("onesign", dict(obs_dim=41, width=512, depth=2, mode="mean", E=2, m=1, n=100, h=3)),
    # divergence before the last step under the velocity reward: the headline shape and two others
    ("vel", dict(obs_dim=20, width=512, depth=2, mode="mean", E=5, m=1, n=2000, h=4)),
    ("vel", dict(obs_dim=17, width=128, depth=2, mode="single", m=2, n=100, h=3)),
    ("vel", dict(obs_dim=41, width=96, depth=1, mode="per_block", E=2, m=2, n=100, h=2)),
]


def case_id(kind, kw):
    return "%s_o%d_w%d_d%d_%s_m%d_n%d_h%d" % (kind, kw["obs_dim"], kw["width"], kw["depth"], kw["mode"], kw["m"],
                                             kw["n"], kw["h"])


def rnn_case(cell, sizes, cell_act="tanh", obs_dim=20, act_dim=6, m=2, n=100, h=3, seed=0):
    """Recurrent stack (``cell`` lstm / gru / rnn, layer ``sizes``) whose first-layer kernels carry +S from action 0 and -S
    from action 1 into every gate: a0 = a1 = +inf at step 0 gives inf - inf in every gate pre-activation -> NaN state and
    return for the rest of the horizon; every other candidate stays finite.  Zero initial hidden state."""
    from learning_to_adapt_amd.dynamics import rnn_cells
    params = synthetic.make_rnn_stack_set(obs_dim, act_dim, sizes, cell, 4000 + seed)
    spec_names = [name for name, _ in rnn_cells.param_spec(obs_dim, act_dim, sizes, cell)]
    for p, name in zip(params, spec_names):
        if p.ndim == 2 and p.shape[0] >= obs_dim + act_dim and not name.startswith("output") and \
                ("cell_0/" in name or "multi_rnn_cell" not in name):
            p[obs_dim + 0] = _S
            p[obs_dim + 1] = -_S
    rs = np.random.RandomState(8000 + seed)
    low, high = -np.ones(act_dim), np.ones(act_dim)
    norm = synthetic.make_norm(obs_dim, act_dim, low, high, 5 + seed)
    obs0 = rs.randn(m, obs_dim)
    acts = rs.uniform(low, high, (h, m * n, act_dim))
    spec = RewardSpec.make(w_vel=1.0, dt=0.05, alive=0.05, vel_index=obs_dim - 1)
    pattern = np.full((m, n), FINITE, dtype=np.int8)
    for i in range(m):
        for j in (29 + i, 64):
            acts[0, i * n + j, 0:2] = np.inf
            pattern[i, j] = NAN
    return dict(cell=cell, sizes=list(sizes), cell_act=cell_act, obs_dim=obs_dim, act_dim=act_dim, m=m, n=n, h=h,
                params=params, norm=norm, obs0=obs0, acts=acts, spec=spec, discount=0.95, pattern=pattern)


def rnn_oracle_returns(case, dtype=np.float32):
    from oracle.rnn_cells import OracleRNNStackDynamics
    from oracle.rnn_planner import rnn_rollout_returns
    dyn = OracleRNNStackDynamics(case["obs_dim"], case["act_dim"], case["sizes"], case["cell"], case["params"], case["norm"],
                                 hidden_nonlinearity=case["cell_act"], dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        r = rnn_rollout_returns(dyn, case["spec"].evaluate, case["obs0"], dyn.get_initial_hidden(case["m"]), case["acts"],
                                case["n"], case["discount"])
    return r.reshape(case["m"], case["n"])


# (cell, layer sizes, cell activation): the LSTM kernels at 128 / 256 units (matrix core, micro tiles at 256, VALU), the
# generic stack kernels (GRU / BasicRNN, one and two layers, relu cells)
RNN_CASES = [
    ("lstm", [128], "tanh"), ("lstm", [256], "relu"), ("gru", [256], "tanh"), ("gru", [64, 64], "relu"),
    ("rnn", [256], "relu"), ("rnn", [96, 40], "tanh"),
]
