"""Plain NumPy restatement of the TS1 step boundary (``include/l2a.h``: ``l2a_particle_step``) for the tests; no library calls.

* ``step``: the step reward of every particle - ``RewardProgram.evaluate_f32`` of its pre-state, action and post-state, or the
  given rewards - then ``R' = R + fp32(disc_t) * r`` as one fp32 multiply and one fp32 add (``R`` the literal 0 at step 0: the
  addition is still made), then ``particle_ts1_reference.shuffle`` of the post-states and of ``R'``.  ``table=None`` is the last
  step: nothing is dealt.  States pass through as whatever dtype comes in (the GPU tests compare them as 32-bit words).
* ``chain``: ``step`` along a horizon of GIVEN post-states, the discount formed by the host's repeated product ``d *= discount`` -
  what the plan entries do with the rollout's states in place of the given ones.
* ``inrange_margin``: per particle, the smallest distance over the horizon of an ``INRANGE`` term's input to one of its bounds,
  relative to ``max(1, |bound|)`` - a state within rounding of a bound flips a whole coefficient, which no tolerance on the
  return covers; the GPU tests leave such particles out (and cap how many)."""

import numpy as np

import particle_ts1_reference as t1
from learning_to_adapt_amd.envs import reward_spec as rsp


def _f32(a):
    """``a`` as fp32 VALUES: 32-bit integer arrays are bit patterns and are reinterpreted, never converted."""
    a = np.ascontiguousarray(a)
    return a.view(np.float32) if a.dtype in (np.uint32, np.int32) else a.astype(np.float32, copy=False)


def step(pre, post, act, ret_in, disc_t, table, program=None, rewards=None):
    """``pre [m, E, n, O]`` or ``[m, E, O]`` (one row per member block), ``post [m, E, n, O]``, ``act [m, E, n, A]``, ``ret_in
    [m, E, n]`` or ``None``, ``table [m, n, E]`` or ``None`` -> ``(state_out or None, ret_out)``."""
    assert (program is None) != (rewards is None), "exactly one of program and rewards"
    f = np.float32
    post = np.asarray(post)
    m, E, n, O = post.shape
    if rewards is None:
        pre = np.asarray(pre)
        if pre.ndim == 3:
            pre = np.broadcast_to(pre[:, :, None, :], post.shape)
        r = program.evaluate_f32(_f32(pre).reshape(-1, O), _f32(act).reshape(m * E * n, -1), _f32(post).reshape(-1, O)).reshape(m, E, n)
    else:
        r = _f32(rewards).reshape(m, E, n)
    R = np.zeros((m, E, n), dtype=f) if ret_in is None else _f32(ret_in)
    with np.errstate(all="ignore"):
        total = f(R + f(disc_t) * r)
    assert total.dtype == f
    if table is None:
        return None, total
    return t1.shuffle(post, total, table)


def chain(pre0, posts, acts, tables, discount, program=None, rewards=None):
    """``pre0 [m, E, O]``, ``posts [h, m, E, n, O]``, ``acts [h, m, E, n, A]``, ``tables [h - 1, m, n, E]``, ``rewards
    [h, m, E, n]`` or ``None`` -> the returns ``[m, E, n]`` behind the last step.  Step ``t + 1`` reads the states step ``t`` dealt."""
    h = len(posts)
    state, ret, d = pre0, None, 1.0
    for t in range(h):
        state, ret = step(state, posts[t], acts[t], ret, d, tables[t] if t < h - 1 else None, program=program,
                          rewards=None if rewards is None else rewards[t])
        d *= float(discount)
    return ret


def inrange_margin(program, obs, act, nxt):
    """float64 ``[rows]``: the smallest ``|x - bound| / max(1, |bound|)`` over the program's ``INRANGE`` terms and their two bounds
    (``inf`` without such a term)."""
    obs, act, nxt = (np.asarray(a, dtype=np.float64) for a in (obs, act, nxt))
    out = np.full(obs.shape[0], np.inf)
    for t in program.terms[:program.n_terms]:
        if t.kind != rsp.TERM_INRANGE:
            continue
        x = {rsp.SRC_OBS: obs, rsp.SRC_ACT: act, rsp.SRC_NEXT: nxt}.get(t.source)
        x = (nxt - obs)[:, t.index] if x is None else x[:, t.index]
        for bound in (float(t.lo), float(t.hi)):
            out = np.minimum(out, np.abs(x - bound) / max(1.0, abs(bound)))
    return out


def particle_margins64(program, sets, norms, observations, actions, n, tables, activation="relu"):
    """``[m, E, n]``: ``inrange_margin`` of the particle that ENDS in block ``e``, its smallest over the horizon, along the float64
    rollout of ``particle_ts1_reference.particle_returns64`` (the margins move with the particles as the returns do)."""
    class _Env(object):
        def __init__(self):
            self.steps = []

        def reward(self, obs, act, nxt):
            self.steps.append(inrange_margin(program, obs, act, nxt))
            return np.zeros(len(obs))

    # the restatement SUMS what `reward` returns: record every step's margins in the step's own row order instead, and fold their
    # minimum below by replaying the shuffles
    env = _Env()
    t1.particle_returns64(env, sets, norms, observations, actions, n, tables)
    m, E = len(observations), len(sets)
    best = None
    for t, marg in enumerate(env.steps):
        marg = marg.reshape(m, E, n)
        best = marg if best is None else np.minimum(best, marg)
        if t < len(env.steps) - 1:
            best = t1.shuffle(np.zeros((m, E, n, 1)), best, tables[t])[1]
    return best
