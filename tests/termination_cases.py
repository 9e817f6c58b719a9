"""Shared builders of the termination tests (CPU and GPU): kernel inputs with their guards, and the plan cases - golden cases
whose guard bounds are taken from the float64 oracle's own trace."""

import numpy as np

import cases
import termination_reference as tref
from learning_to_adapt_amd.envs import TerminationProgram

INF = float("inf")

#               m,   n, obs, act, h
KERNEL_SHAPES = [(1, 64, 20, 6, 3),         # whole block
                 (1, 33, 17, 5, 1),         # ragged block, odd dims, h = 1
                 (3, 70, 41, 8, 4),         # blocks straddling env boundaries
                 (2, 130, 64, 16, 2),       # the dimension limits of the matrix-core rollout kernels
                 (1, 129, 17, 5, 3)]        # unaligned steps: an odd number of odd rows
KERNEL_IDS = ["m%d_n%d_o%d_a%d_h%d" % s for s in KERNEL_SHAPES]


def kernel_inputs(seed, m, n, od, ad, h):
    """``tests/test_reward_program_gpu._inputs``: magnitudes 0.1 .. 10 with random signs, fp32."""
    rs = np.random.RandomState(seed)

    def draw(*shape):
        return (rs.uniform(0.1, 10.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
    return draw(m, od), draw(h, m * n, od), draw(h, m * n, ad)


def kernel_guards(od):
    """[-8, 8] on one coordinate plus a three-element guard with an infinite side: about 30 % of the rows die per step."""
    return [(1, 1, -8.0, 8.0), (od - 4, 3, -INF, 9.0)]


def never_guards(od):
    return [(0, od, -INF, INF)]


def program_of(guards, terminal_reward=0.0):
    term = TerminationProgram(terminal_reward=terminal_reward)
    for index, length, lo, hi in guards:
        term.alive_in_range(index, lo, hi, length=length)
    return term


def keep_off_bounds(traj, guards, margin=1e-3):
    """Move guarded values that lie within ``margin`` of a finite bound to ``2 * margin`` above it (in place)."""
    for index, length, lo, hi in guards:
        part = traj[..., index:index + length]
        for b in (lo, hi):
            if np.isfinite(b):
                part[np.abs(part - b) < margin] = b + 2 * margin
    return traj


def survived(guards, traj, steps_alive):
    h = traj.shape[0]
    return np.array([steps_alive[r] == h and not tref.is_terminal(guards, traj[h - 1, r]) for r in range(traj.shape[1])])


# ---- plan cases ----------------------------------------------------------------------------------------------------------
# golden case -> (coordinate, lower quantile or None, upper quantile or None) of the oracle's trace over rows and steps.  Found on
# the CPU with the oracle alone (tests/test_termination.py checks the conditions again): at most 1 % ambiguous rows, at least
# 20 % of the rows terminate before h, at least 20 % survive.
PLAN_GUARDS = {"hc_rs_ragged_n37_h3_s0": (11, 15, 85),
               "hc_rs_m2_n100_h7_e2_s0": (10, 30, None),
               "ant_rs_n300_h6_e3_s0": (17, None, 70)}
PLAN_CASES = list(PLAN_GUARDS)
_PLAN = {}


def plan_case(cid):
    """The oracle's side of a plan case, built once and never modified: candidates, float64 trace, guards (bounds rounded to fp32,
    so that the fp32 program and the float64 reference hold the same numbers)."""
    if cid not in _PLAN:
        from oracle.planner import rollout_trace, sample_rs_actions
        from oracle.rewards import make_reward
        case, seed = cases.split_id(cid)
        env = cases.recipe(case)[0]
        np.random.seed(seed)
        actions = sample_rs_actions(env.action_space.low, env.action_space.high, case["n"], case["m"], case["h"])
        gold = cases.load_golden(cid)
        rf = make_reward(case["env"], env.dt)
        disc = case.get("discount", 1.0)
        total, trace = rollout_trace(cases.oracle_dynamics(case), rf, gold["obs0"], actions, case["n"], disc)
        coord, ql, qh = PLAN_GUARDS[cid]
        lo = -INF if ql is None else float(np.float32(np.percentile(trace[:, :, coord], ql)))
        hi = INF if qh is None else float(np.float32(np.percentile(trace[:, :, coord], qh)))
        guards = [(coord, 1, lo, hi)]
        obs_rows = np.repeat(np.asarray(gold["obs0"], dtype=np.float64), case["n"], axis=0)
        _PLAN[cid] = dict(case=case, env=env, actions=actions, obs0=gold["obs0"], obs_rows=obs_rows, trace=trace, total=total,
                          guards=guards, discount=disc, reward_fn=rf)
    return _PLAN[cid]


def plan_want(p, reward_fn, terminal_reward=0.0, terminal_values=None, value_coef=1.0):
    """The float64 reference of a plan case under ``reward_fn``: ``(returns, steps_alive, ambiguous, survived)`` per row."""
    rewards = tref.step_rewards_f64(reward_fn, p["obs_rows"], p["trace"], p["actions"])
    want, steps = tref.returns_f64(p["guards"], terminal_reward, p["trace"], rewards, p["discount"], terminal_values, value_coef)
    return want, steps, tref.ambiguous_rows(p["guards"], p["trace"], steps), survived(p["guards"], p["trace"], steps)
