"""Restatements of the particle plans (``include/l2a.h``: ``l2a_plan_rs_particles``, ``l2a_particle_score``) for the tests.

* ``member_returns64`` / ``score64``: float64, from the unchanged oracle.  ``OracleMLPDynamics(mode="per_block")`` holding the E sets
  once per env, the observations replicated E-fold and the actions broadcast to ``[h, m E n, A]`` is E single-member rollouts of
  every candidate (``test_particles.py`` checks that equality on the CPU); then ``mean - lambda std`` (biased std) in float64.
* ``score_f32``: the scorer's fixed fp32 arithmetic, operation by operation in ``np.float32`` - what the kernel must equal bit for
  bit - and ``keys``: ``l2a_key_encode`` over a score table, first maximum, NaN highest.

Bounds (derived; nothing here is measured and then set):

* ``score_f32`` against ``score64`` of the same fp32 table, ``score_bound``, to first order in u = 2^-24 with B = max_e |R_e| of
  the candidate.  Mean: E - 1 additions of partial sums of at most E B, divided by E, and the division's own rounding:
  |mean32 - mean| <= (E - 1) u B + u B = E u B.  Deviations: d_e inherits the mean's error and rounds a value of at most 2 B:
  (E + 2) u B each, and the root mean square is 1-Lipschitz in the sup norm of its inputs.  The root mean square of the rounded
  d_e: squares (u), a sum of E non-negative terms ((E - 1) u), the division (u), halved by the root, which adds its own u -
  (E + 3) u / 2 relative to a value of at most 2 B.  So |std32 - std| <= (E + 2) u B + (E + 3) u B = (2 E + 5) u B.  Score: the
  product adds u |lambda| 2 B, the difference u (1 + 2 |lambda|) B.  In all
  |score32 - score| <= u B ((E + 1) + |lambda| (2 E + 9)) <= (1 + |lambda|) (2 E + 10) u B - a few ulps of B times (1 + |lambda|).
  The spread alone is held to the same expression at lambda = 0.
* GPU against the oracle (``test_particles_gpu.py``): the project's bar, 1e-4 of max |R| per member return; the score within
  (1 + |lambda|) times that, the mean being an average and std 1-Lipschitz in the sup norm of the member errors.
"""

import ctypes

import numpy as np

from learning_to_adapt_amd import _lib

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------- float64
def member_returns64(env, sets, norms, observations, actions, n, discount=1.0, activation="relu", reward_fn=None):
    """``[m, E, n]`` float64: member e's return of candidate j of env i.  ``actions`` float64 ``[h, m n, A]``, row ``i n + j``."""
    from oracle import OracleMLPDynamics, planner
    obs = np.asarray(observations, dtype=np.float64)
    m, E = len(obs), len(sets)
    h, A = actions.shape[0], actions.shape[2]
    dyn = OracleMLPDynamics(env.observation_space.shape[0], env.action_space.shape[0], list(sets) * m, list(norms) * m,
                            mode="per_block", hidden_nonlinearity=activation)
    obs_x = np.repeat(obs, E, axis=0)                                                       # block i E + e: env i
    act_x = np.broadcast_to(np.asarray(actions, dtype=np.float64).reshape(h, m, 1, n, A), (h, m, E, n, A)).reshape(h, m * E * n, A)
    ret = planner.rollout_returns(dyn, reward_fn or env.reward, obs_x, np.ascontiguousarray(act_x), n, discount)
    return ret.reshape(m, E, n)


def score64(member_returns, lam):
    """``(score, std, mean)`` ``[m, n]`` in float64 (biased standard deviation over the member axis)."""
    R = np.asarray(member_returns, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = R.mean(axis=1)
        std = np.sqrt(((R - mean[:, None]) ** 2).mean(axis=1))
        score = mean if lam == 0 else mean - float(lam) * std
    return score, std, mean


# --------------------------------------------------------------------------------------------------------------------- fp32
def score_f32(member_returns, lam):
    """``(score, std)`` fp32 ``[m, n]``: the kernel's arithmetic, one rounding per operation, e ascending."""
    R = np.ascontiguousarray(member_returns, dtype=np.float32)
    m, E, n = R.shape
    fe = np.float32(E)
    lam = np.float32(lam)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = R[:, 0].copy()
        for e in range(1, E):
            s = s + R[:, e]
        mean = s / fe
        v = np.zeros((m, n), dtype=np.float32)
        for e in range(E):
            d = R[:, e] - mean
            v = v + d * d
        std = np.sqrt(v / fe)
        score = mean.copy() if lam == 0 else mean - lam * std
    assert score.dtype == np.float32 and std.dtype == np.float32
    return score, std


def key_encode(ret, index):
    lib = _lib.load()
    return int(lib.l2a_key_encode(ctypes.c_float(float(ret)), int(index)))


def keys(score, cand_offset=0):
    """uint64 ``[m]``: the largest packed key per env - ``np.argmax`` with NaN as the maximum, the first one winning."""
    score = np.asarray(score, dtype=np.float32)
    out = np.zeros(score.shape[0], dtype=np.uint64)
    for i, row in enumerate(score):
        out[i] = max(key_encode(r, cand_offset + j) for j, r in enumerate(row))
    return out


def argmax_nan_first(row):
    """Index the keys decode to: the first NaN if any, else the first maximum."""
    row = np.asarray(row)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def score_bound(member_returns, lam):
    """|score_f32 - score64| per candidate for finite tables (see the module docstring)."""
    R = np.abs(np.asarray(member_returns, dtype=np.float64))
    E = R.shape[1]
    return (1.0 + abs(float(lam))) * (2 * E + 10) * U * R.max(axis=1)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def random_table(rs, m, E, n, scale=3.0, offset=0.0):
    return (offset + scale * rs.randn(m, E, n)).astype(np.float32)


RISK_RECIPES = (        # (E, np.random.seed, oracle's choice at lambda = 0 / 1 / 4): make_members(half_cheetah, (128, 128), E), n = 50, h = 7
    (2, 0, (3, 46, 46)),
    (3, 0, (42, 31, 31)),
    (5, 2, (15, 49, 49)),
)
RISK_LAMBDAS = (0.0, 1.0, 4.0)
