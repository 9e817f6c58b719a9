"""Termination rules as data, so that a scoring kernel can end a candidate's episode where the env would.

Hopper, Walker2d, gym's Ant and Humanoid end an episode when the state leaves a healthy range; a planner that does not know
trades a fall for forward velocity.  A ``TerminationProgram`` (``struct l2a_termination`` in ``include/l2a.h``) is 1 .. 8
guards over the NEXT observation of a step: guard ``{index, len, lo, hi}`` holds iff every ``x`` in
``next_obs[index : index + len]`` satisfies ``lo <= x <= hi`` (a NaN is outside), and a transition is terminal iff any guard
fails.  An env sets ``termination_spec = program``; ``MPCController`` then plans on returns that stop at a candidate's
terminal step (``l2a_plan_rs_term``).
"""

import ctypes

import numpy as np

TERMINATION_MAX_GUARDS = 8


class Guard(ctypes.Structure):
    _fields_ = [
        ("index", ctypes.c_int),
        ("len", ctypes.c_int),
        ("lo", ctypes.c_float),
        ("hi", ctypes.c_float),
    ]


class TerminationProgram(ctypes.Structure):
    """Mirrors ``struct l2a_termination`` field for field.  Built with the chaining builder::

        term = (TerminationProgram(terminal_reward=-1.0)
                .alive_in_range(0, 0.7, float("inf"))            # torso height
                .alive_in_range(1, -0.2, 0.2)                    # torso angle
                .alive_in_range(2, -100.0, 100.0, length=9))     # every other state coordinate

    The float64 bounds the builder was given are kept beside the fp32 C fields (as ``RewardProgram`` does): ``alive`` is the
    float64 rule an env's ``step`` applies, ``returns_f32`` restates the kernel's fp32 arithmetic bit for bit."""

    _fields_ = [
        ("n_guards", ctypes.c_int),
        ("reserved", ctypes.c_int),
        ("terminal_reward", ctypes.c_float),
        ("reserved2", ctypes.c_float),
        ("guards", Guard * TERMINATION_MAX_GUARDS),
    ]

    def __init__(self, terminal_reward=0.0):
        super(TerminationProgram, self).__init__()
        self.terminal_reward = terminal_reward
        self.exact = []         # (lo, hi) in float64, guard by guard

    def _exact(self):
        ex = self.__dict__.get("exact")
        if ex is None or len(ex) != self.n_guards:      # a program filled field by field: the fp32 fields are all there is
            ex = self.exact = [(float(g.lo), float(g.hi)) for g in self.guards[:self.n_guards]]
        return ex

    def alive_in_range(self, index, lo, hi, length=1):
        """The episode goes on only while ``lo <= next_obs[index + k] <= hi`` for every ``k < length``."""
        ex = self._exact()
        if self.n_guards >= TERMINATION_MAX_GUARDS:
            raise ValueError("a termination program holds at most %d guards" % TERMINATION_MAX_GUARDS)
        self.guards[self.n_guards] = Guard(int(index), int(length), lo, hi)
        self.n_guards += 1
        ex.append((float(lo), float(hi)))
        return self

    def check(self, obs_dim):
        """``l2a_termination_check`` (host only): raises ``ValueError`` with the library's message."""
        from .. import _lib
        lib = _lib.load()
        if lib.l2a_termination_check(ctypes.byref(self), int(obs_dim)) != 0:
            raise ValueError(lib.l2a_last_error(None).decode())
        return self

    # ---- host evaluation ---------------------------------------------------------------------
    def alive(self, next_obs):
        """Float64 NumPy, vectorised over rows: True where every guard holds on ``next_obs`` ``[rows, obs_dim]``."""
        x = np.asarray(next_obs, dtype=np.float64)
        ok = np.ones((x.shape[0],), dtype=bool)
        with np.errstate(invalid="ignore"):
            for g, (lo, hi) in zip(self.guards[:self.n_guards], self._exact()):
                part = x[:, g.index:g.index + g.len]
                ok &= np.all((part >= lo) & (part <= hi), axis=1)
        return ok

    def alive_f32(self, next_obs):
        """The kernel's test: fp32 values against the fp32 bounds."""
        f = np.float32
        x = np.asarray(next_obs, dtype=f)
        ok = np.ones((x.shape[0],), dtype=bool)
        with np.errstate(invalid="ignore"):
            for g in self.guards[:self.n_guards]:
                part = x[:, g.index:g.index + g.len]
                ok &= np.all((part >= f(g.lo)) & (part <= f(g.hi)), axis=1)
        return ok

    def returns_f32(self, obs_rows, traj, actions, discount, program=None, step_rewards=None, terminal_values=None,
                    value_coef=1.0):
        """``l2a_score_term_k`` restated in float32 NumPy, bit for bit: ``(returns [rows], steps_alive [rows] int32)``.
        Exactly one of ``program`` (a ``RewardProgram``; ``obs_rows`` ``[rows, obs_dim]`` is the observation in front of step 0
        per row, ``actions`` ``[h, rows, act_dim]``) and ``step_rewards`` (``[h, rows]``; ``obs_rows`` and ``actions`` are not
        looked at).  ``traj`` ``[h, rows, obs_dim]``; ``terminal_values`` ``[rows]`` or None, folded into surviving rows with
        ``w = fp32(value_coef * discount ** h)``."""
        assert (program is None) != (step_rewards is None)
        f = np.float32
        traj = np.asarray(traj, dtype=f)
        h, rows = traj.shape[0], traj.shape[1]
        total = np.zeros((rows,), dtype=f)
        steps = np.full((rows,), h, dtype=np.int32)
        alive = np.ones((rows,), dtype=bool)
        tr = f(self.terminal_reward)
        disc = 1.0
        state = obs_rows
        with np.errstate(all="ignore"):
            for t in range(h):
                if program is not None:
                    r = program.evaluate_f32(state, actions[t], traj[t])
                else:
                    r = np.asarray(step_rewards[t], dtype=f)
                d = f(disc)
                total = np.where(alive, total + d * r, total)
                dies = alive & ~self.alive_f32(traj[t])
                if tr != f(0.0):
                    total = np.where(dies, total + d * tr, total)
                steps[dies] = t + 1
                alive &= ~dies
                disc *= float(discount)
                state = traj[t]
            if terminal_values is not None:
                w = f(float(value_coef) * disc)
                if w != f(0.0):
                    total = np.where(alive, total + w * np.asarray(terminal_values, dtype=f), total)
        return total, steps


def termination_spec_for_env(env):
    """``env.termination_spec`` (a ``TerminationProgram``) or ``None``: none of the reference's envs terminates."""
    return getattr(env, "termination_spec", None)
