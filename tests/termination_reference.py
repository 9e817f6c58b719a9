"""Float64 restatement of the termination semantics of include/l2a.h ("plans on envs that terminate"), written as plain loops
over rows, steps and guards - independent of ``TerminationProgram`` and of NumPy's vectorised comparisons.

A guard is a tuple ``(index, length, lo, hi)``; it holds iff every ``x`` in ``next_obs[index : index + length]`` satisfies
``lo <= x <= hi`` (a NaN is outside).  A transition is terminal iff any guard fails.  Per row::

    alive = True; R = 0; steps_alive = h
    for t in 0 .. h-1, while alive:
        R += discount ** t * r_t
        if any guard fails on traj[t]:
            if terminal_reward != 0: R += discount ** t * terminal_reward
            alive = False; steps_alive = t + 1
    if alive and terminal_values given: R += value_coef * discount ** h * terminal_values[row]
"""

import math

import numpy as np


def guard_holds(guard, x):
    index, length, lo, hi = guard
    for k in range(length):
        v = float(x[index + k])
        if math.isnan(v) or not (lo <= v <= hi):
            return False
    return True


def is_terminal(guards, next_obs):
    for g in guards:
        if not guard_holds(g, next_obs):
            return True
    return False


def returns_f64(guards, terminal_reward, traj, step_rewards, discount, terminal_values=None, value_coef=1.0):
    """``traj`` ``[h, rows, obs_dim]``, ``step_rewards`` ``[h, rows]`` -> ``(returns [rows] float64, steps_alive [rows] int32)``."""
    traj = np.asarray(traj, dtype=np.float64)
    step_rewards = np.asarray(step_rewards, dtype=np.float64)
    h, rows = traj.shape[0], traj.shape[1]
    out = np.zeros((rows,), dtype=np.float64)
    steps = np.zeros((rows,), dtype=np.int32)
    for r in range(rows):
        total, disc, alive, lived = 0.0, 1.0, True, h
        for t in range(h):
            total += disc * step_rewards[t, r]
            if is_terminal(guards, traj[t, r]):
                if terminal_reward != 0.0:
                    total += disc * float(terminal_reward)
                alive, lived = False, t + 1
                break
            disc *= float(discount)
        if alive and terminal_values is not None and value_coef != 0.0:
            total += float(value_coef) * disc * float(terminal_values[r])
        out[r], steps[r] = total, lived
    return out, steps


def step_rewards_f64(reward_fn, obs_rows, traj, actions):
    """``reward_fn(obs, act, next_obs)`` (float64, vectorised over rows) on every step of whole trajectories: ``[h, rows]``."""
    traj = np.asarray(traj, dtype=np.float64)
    state = np.asarray(obs_rows, dtype=np.float64)
    out = []
    for t in range(traj.shape[0]):
        out.append(np.asarray(reward_fn(state, np.asarray(actions[t], dtype=np.float64), traj[t]), dtype=np.float64))
        state = traj[t]
    return np.stack(out)


def ambiguous_rows(guards, traj, steps_alive, rel=1e-4):
    """Rows with a guarded value within ``rel * max(1, |bound|)`` of a finite bound at any step up to their terminal step: a
    rollout that agrees with ``traj`` to well below ``rel`` may decide such a row the other way."""
    traj = np.asarray(traj, dtype=np.float64)
    rows = traj.shape[1]
    out = np.zeros((rows,), dtype=bool)
    for r in range(rows):
        for t in range(int(steps_alive[r])):
            for index, length, lo, hi in guards:
                for k in range(length):
                    v = traj[t, r, index + k]
                    for b in (lo, hi):
                        if math.isfinite(b) and abs(v - b) <= rel * max(1.0, abs(b)):
                            out[r] = True
    return out
