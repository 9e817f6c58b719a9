"""Closed-form planning rewards as data, so the rollout kernel can fuse them.

The reference evaluates ``env.reward(obs, act, next_obs)`` on the host once per horizon
step (``policies/mpc_controller.py:125``).  All five reference rewards are instances of

    r = w_vel * (next[vel_index] - obs[vel_index]) / dt + alive
        - ctrl_coef * sum(act**2) - dist_coef * ||next[dist_index : dist_index+3]||

* HalfCheetah (+Blocks, +HField): ``envs/half_cheetah_env.py:58-65`` - w_vel 1,
  vel_index obs_dim-3, ctrl_coef 0.05.
* Ant: ``envs/ant_env.py:56-66`` - w_vel 1, alive 0.05, ctrl_coef 0.
* Arm7Dof: ``envs/arm_7dof_env.py:91-99`` - dist_coef 1 over next[-3:], ctrl_coef 0.005.

``RewardSpec`` mirrors ``struct l2a_reward`` in ``include/l2a.h`` field for field.

Any OTHER closed-form reward is declared as a ``RewardProgram`` (``struct l2a_reward_program``): a short list of
terms over ``obs``, ``act``, ``next_obs`` that a scoring kernel evaluates behind the rollout
(``l2a_plan_rs_program``).  An env sets ``reward_spec = program`` and ``reward = program.evaluate``.
"""

import ctypes

import numpy as np


class RewardSpec(ctypes.Structure):
    _fields_ = [
        ("w_vel", ctypes.c_float),
        ("inv_dt", ctypes.c_float),
        ("alive", ctypes.c_float),
        ("ctrl_coef", ctypes.c_float),
        ("dist_coef", ctypes.c_float),
        ("vel_index", ctypes.c_int),
        ("dist_index", ctypes.c_int),
        ("reserved", ctypes.c_int),
    ]

    @classmethod
    def make(cls, w_vel=0.0, dt=1.0, alive=0.0, ctrl_coef=0.0, dist_coef=0.0, vel_index=0, dist_index=0):
        """Build a spec; the float64 coefficients are kept beside the fp32 C fields so that the
        host-side ``evaluate`` reproduces the reference's float64 arithmetic exactly."""
        spec = cls(w_vel, (1.0 / dt) if w_vel != 0.0 else 0.0, alive, ctrl_coef, dist_coef,
                   int(vel_index), int(dist_index), 0)
        spec.exact = dict(w_vel=float(w_vel), dt=float(dt), alive=float(alive), ctrl_coef=float(ctrl_coef),
                          dist_coef=float(dist_coef))
        return spec

    @classmethod
    def half_cheetah(cls, obs_dim, dt):
        return cls.make(w_vel=1.0, dt=dt, ctrl_coef=1e-1 * 0.5, vel_index=obs_dim - 3)

    @classmethod
    def ant(cls, obs_dim, dt):
        return cls.make(w_vel=1.0, dt=dt, alive=0.05, vel_index=obs_dim - 3)

    @classmethod
    def arm_7dof(cls, obs_dim):
        return cls.make(ctrl_coef=0.01 * 0.5, dist_coef=1.0, dist_index=obs_dim - 3)

    @classmethod
    def none(cls):
        """All-zero reward (used by ``predict``-only launches)."""
        return cls.make()

    def evaluate(self, obs, act, next_obs):
        """Host NumPy evaluation of the same closed form (float64)."""
        ex = getattr(self, "exact", None) or dict(
            w_vel=float(self.w_vel), dt=(1.0 / float(self.inv_dt)) if self.inv_dt else 1.0,
            alive=float(self.alive), ctrl_coef=float(self.ctrl_coef), dist_coef=float(self.dist_coef))
        r = np.zeros((obs.shape[0],))
        if ex["w_vel"] != 0.0:
            r = r + ex["w_vel"] * (next_obs[:, self.vel_index] - obs[:, self.vel_index]) / ex["dt"]
        if ex["dist_coef"] != 0.0:
            d = self.dist_index
            r = r - ex["dist_coef"] * np.linalg.norm(next_obs[:, d:d + 3], axis=1)
        if ex["ctrl_coef"] != 0.0:
            r = r - ex["ctrl_coef"] * np.sum(np.square(act), axis=1)
        return r + ex["alive"]


# ---- reward programs (include/l2a.h: l2a_reward_program) ----------------------------------------
SRC_OBS, SRC_ACT, SRC_NEXT, SRC_DELTA = 0, 1, 2, 3
TERM_LINEAR, TERM_SQSUM, TERM_NORM, TERM_INRANGE = 0, 1, 2, 3
PROGRAM_MAX_TERMS = 16
PROGRAM_MAX_CONSTS = 64
_SRC_NAMES = {"obs": SRC_OBS, "act": SRC_ACT, "next": SRC_NEXT, "delta": SRC_DELTA}


class RewardTerm(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int),
        ("source", ctypes.c_int),
        ("index", ctypes.c_int),
        ("len", ctypes.c_int),
        ("target", ctypes.c_int),
        ("coef", ctypes.c_float),
        ("lo", ctypes.c_float),
        ("hi", ctypes.c_float),
    ]


class RewardProgram(ctypes.Structure):
    """``r = bias + sum over terms, in program order, of coef * v(term)`` - mirrors ``struct l2a_reward_program`` field
    for field.  Built with the chaining builders below::

        prog = (RewardProgram().with_bias(0.05)
                .linear("delta", 17, 1.0, div=env.dt)          # forward progress
                .in_range("next", 2, 0.2, 1.0)                 # alive while the torso height is in range
                .sqsum("act", 0, act_dim, -0.1)                # control cost
                .norm("next", 0, 3, -1.0, target=goal))        # distance of next[0:3] to a goal

    The float64 values the builders were given are kept beside the fp32 C fields (as ``RewardSpec.make`` does), so that
    ``evaluate`` is the float64 reward an env hands to the reference planner, while ``evaluate_f32`` restates the kernel's
    fp32 arithmetic bit for bit."""

    _fields_ = [
        ("n_terms", ctypes.c_int),
        ("n_consts", ctypes.c_int),
        ("bias", ctypes.c_float),
        ("reserved", ctypes.c_int),
        ("terms", RewardTerm * PROGRAM_MAX_TERMS),
        ("consts", ctypes.c_float * PROGRAM_MAX_CONSTS),
    ]

    # ---- builders ----------------------------------------------------------------------------
    def _exact(self):
        ex = self.__dict__.get("exact")
        if ex is None:          # a program filled field by field: the fp32 fields are all there is
            ex = self.exact = dict(bias=float(self.bias), terms=[
                dict(coef=float(t.coef), div=None, lo=float(t.lo), hi=float(t.hi),
                     target=None if t.target < 0 else np.array(self.consts[t.target:t.target + t.len], dtype=np.float64))
                for t in self.terms[:self.n_terms]])
        return ex

    def _add(self, kind, source, index, length, coef, div=None, target=None, lo=0.0, hi=0.0):
        ex = self._exact()
        if self.n_terms >= PROGRAM_MAX_TERMS:
            raise ValueError("a reward program holds at most %d terms" % PROGRAM_MAX_TERMS)
        source = _SRC_NAMES[source] if isinstance(source, str) else int(source)
        off = -1
        if target is not None:
            target = np.asarray(target, dtype=np.float64).reshape(-1)
            if target.shape[0] != int(length):
                raise ValueError("target has %d values for a range of %d" % (target.shape[0], length))
            off = int(self.n_consts)
            if off + target.shape[0] > PROGRAM_MAX_CONSTS:
                raise ValueError("a reward program holds at most %d constants" % PROGRAM_MAX_CONSTS)
            for k, v in enumerate(target):
                self.consts[off + k] = v
            self.n_consts = off + target.shape[0]
        c64 = float(coef) if div is None else float(coef) / float(div)
        self.terms[self.n_terms] = RewardTerm(int(kind), source, int(index), int(length), off, c64, lo, hi)
        self.n_terms += 1
        ex["terms"].append(dict(coef=float(coef), div=None if div is None else float(div), lo=float(lo), hi=float(hi),
                                target=target))
        return self

    def with_bias(self, value):
        self._exact()["bias"] = float(value)
        self.bias = value
        return self

    def linear(self, source, index, coef, div=None):
        """``coef * x[index]`` (``coef * x[index] / div`` in float64 when ``div`` is given; the fp32 coefficient is
        ``coef / div``)."""
        return self._add(TERM_LINEAR, source, index, 1, coef, div=div)

    def sqsum(self, source, index, length, coef, target=None):
        """``coef * sum_k (x[index + k] - target[k]) ** 2``; ``target``: ``length`` values or None for zeros."""
        return self._add(TERM_SQSUM, source, index, length, coef, target=target)

    def norm(self, source, index, length, coef, target=None):
        """``coef * sqrt(sum_k (x[index + k] - target[k]) ** 2)``."""
        return self._add(TERM_NORM, source, index, length, coef, target=target)

    def in_range(self, source, index, lo, hi, coef=1.0):
        """``coef`` while ``lo <= x[index] <= hi`` (a NaN is outside)."""
        return self._add(TERM_INRANGE, source, index, 1, coef, lo=lo, hi=hi)

    @classmethod
    def from_spec(cls, spec, obs_dim, act_dim):
        """A ``RewardSpec`` as a program (the five reference rewards): velocity term, distance norm, control cost in the
        order ``RewardSpec.evaluate`` adds them, the alive bonus as the bias."""
        ex = getattr(spec, "exact", None) or dict(
            w_vel=float(spec.w_vel), dt=(1.0 / float(spec.inv_dt)) if spec.inv_dt else 1.0, alive=float(spec.alive),
            ctrl_coef=float(spec.ctrl_coef), dist_coef=float(spec.dist_coef))
        prog = cls().with_bias(ex["alive"])
        if ex["w_vel"] != 0.0:
            prog.linear(SRC_DELTA, spec.vel_index, ex["w_vel"], div=ex["dt"])
        if ex["dist_coef"] != 0.0:
            prog.norm(SRC_NEXT, spec.dist_index, min(3, int(obs_dim) - spec.dist_index), -ex["dist_coef"])
        if ex["ctrl_coef"] != 0.0:
            prog.sqsum(SRC_ACT, 0, int(act_dim), -ex["ctrl_coef"])
        return prog

    def check(self, obs_dim, act_dim):
        """``l2a_reward_program_check`` (host only): raises ``ValueError`` with the library's message."""
        from .. import _lib
        lib = _lib.load()
        if lib.l2a_reward_program_check(ctypes.byref(self), int(obs_dim), int(act_dim)) != 0:
            raise ValueError(lib.l2a_last_error(None).decode())
        return self

    # ---- host evaluation ---------------------------------------------------------------------
    @staticmethod
    def _source(source, obs, act, next_obs, lo, hi):
        if source == SRC_OBS:
            return obs[:, lo:hi]
        if source == SRC_ACT:
            return act[:, lo:hi]
        if source == SRC_NEXT:
            return next_obs[:, lo:hi]
        return next_obs[:, lo:hi] - obs[:, lo:hi]

    def _value(self, t, x, target, lo, hi, dtype):
        """v(term) on the rows of ``x`` ``[rows, len]``: one multiply and one add per element, k ascending."""
        if t.kind == TERM_LINEAR:
            return x[:, 0]
        if t.kind == TERM_INRANGE:
            return ((x[:, 0] >= lo) & (x[:, 0] <= hi)).astype(dtype)
        d = x - (target if target is not None else dtype(0.0))
        s = np.zeros((x.shape[0],), dtype=dtype)
        for k in range(t.len):
            s = s + d[:, k] * d[:, k]
        return np.sqrt(s) if t.kind == TERM_NORM else s

    def evaluate(self, obs, act, next_obs):
        """The reward in float64 NumPy, vectorised over rows - what an env's ``reward`` returns."""
        obs, act, next_obs = (np.asarray(a, dtype=np.float64) for a in (obs, act, next_obs))
        ex = self._exact()
        with np.errstate(all="ignore"):
            r = np.full((obs.shape[0],), ex["bias"], dtype=np.float64)
            for t, e in zip(self.terms[:self.n_terms], ex["terms"]):
                x = self._source(t.source, obs, act, next_obs, t.index, t.index + t.len)
                c = e["coef"] * self._value(t, x, e["target"], e["lo"], e["hi"], np.float64)
                r = r + (c if e["div"] is None else c / e["div"])
        return r

    def evaluate_f32(self, obs, act, next_obs):
        """The scoring kernel's arithmetic restated in float32 NumPy (include/l2a.h: round to nearest, nothing
        contracted): bit-equal to what ``l2a_score_trajectory`` adds up per step."""
        f = np.float32
        obs, act, next_obs = (np.asarray(a, dtype=f) for a in (obs, act, next_obs))
        with np.errstate(all="ignore"):
            r = np.full((obs.shape[0],), f(self.bias), dtype=f)
            for t in self.terms[:self.n_terms]:
                x = self._source(t.source, obs, act, next_obs, t.index, t.index + t.len)
                target = None if t.target < 0 else np.array(self.consts[t.target:t.target + t.len], dtype=f)
                r = r + f(t.coef) * self._value(t, x, target, f(t.lo), f(t.hi), f)
        return r

    def returns_f32(self, obs_rows, traj, actions, discount):
        """Discounted fp32 returns of whole trajectories as the kernel accumulates them: ``obs_rows`` ``[rows, obs_dim]``
        (the observation in front of step 0, per row), ``traj`` ``[h, rows, obs_dim]``, ``actions`` ``[h, rows, act_dim]``."""
        f = np.float32
        total = np.zeros((np.shape(obs_rows)[0],), dtype=f)
        disc = 1.0
        state = obs_rows
        with np.errstate(all="ignore"):
            for t in range(np.shape(traj)[0]):
                total = total + f(disc) * self.evaluate_f32(state, actions[t], traj[t])
                disc *= float(discount)
                state = traj[t]
        return total


_BY_CLASS_NAME = {
    "HalfCheetahEnv": "half_cheetah",
    "HalfCheetahBlocksEnv": "half_cheetah",
    "HalfCheetahHFieldEnv": "half_cheetah",
    "AntEnv": "ant",
    "Arm7DofEnv": "arm_7dof",
}


def _innermost(env):
    seen = 0
    while seen < 16:
        inner = None
        for attr in ("wrapped_env", "_wrapped_env"):
            inner = env.__dict__.get(attr) if hasattr(env, "__dict__") else None
            if inner is not None:
                break
        if inner is None:
            return env
        env, seen = inner, seen + 1
    return env


def reward_spec_for_env(env):
    """Find the fusable closed form for ``env`` or return ``None``.

    1. an explicit ``env.reward_spec`` attribute wins;
    2. otherwise the class name of the innermost wrapped env is matched against the
       reference's env classes (note N1 of SURVEY.md: ``NormalizedEnv`` keeps the real env
       in ``_wrapped_env`` and forwards attribute reads).
    """
    spec = getattr(env, "reward_spec", None)
    if spec is not None:
        return spec
    core = _innermost(env)
    kind = _BY_CLASS_NAME.get(type(core).__name__)
    if kind is None:
        return None
    obs_dim = int(env.observation_space.shape[0])
    if kind == "half_cheetah":
        return RewardSpec.half_cheetah(obs_dim, float(env.dt))
    if kind == "ant":
        return RewardSpec.ant(obs_dim, float(env.dt))
    return RewardSpec.arm_7dof(obs_dim)
