"""Plain NumPy restatement of the TS1 particle plans (``include/l2a.h``: ``l2a_particle_perm``, ``l2a_particle_shuffle``,
``l2a_plan_rs_particles_ts1``) for the tests; no library calls.

* ``perm``: the permutation of boundary ``t``, env ``i`` and candidates ``gj`` from the vectorised Philox of ``tests/cem_reference.py``
  - Fisher-Yates from the identity, ``k = E - 1`` down to 1, ``r = (word (k + 1)) >> 32``, draw ``d = E - 1 - k`` is word ``d & 3`` of
  the group with third counter word ``'perm' + (d >> 2)``, counter ``((offset + t m + i) << 31) | gj``.  Everything is integer
  arithmetic: the library must equal it exactly.
* ``shuffle``: ``out[i][e][j] = in[i][perm[i][j][e]][j]`` as index arithmetic on whatever dtype comes in (the GPU tests pass bit
  patterns as ``uint32``).
* ``particle_returns64``: float64, one horizon step at a time through the unchanged ``OracleMLPDynamics(mode="per_block")`` and the
  env's reward, state and return rows permuted between two steps - what the TS1 plan's particle returns are held to, at the
  project's bar of 1e-4 of max |R| (``tests/particle_reference.py``)."""

import numpy as np

import cem_reference as cr

PHILOX_PERM = 0x7065726D             # 'perm': third counter word of the shuffle's first word group
MAX_E = 16
SLOT_LIMIT = 1 << 33


def perm(seed, offset, t, m, i, gj, E):
    """uint8 ``[len(gj), E]``: row ``c``, entry ``e`` = the block the particle that lands in block ``e`` of candidate ``gj[c]`` comes
    from, at the boundary behind horizon step ``t`` of env ``i``."""
    assert 1 <= E <= MAX_E
    gj = np.atleast_1d(np.asarray(gj, dtype=np.uint64))
    slot = int(offset) + int(t) * int(m) + int(i)
    assert 0 <= slot < SLOT_LIMIT and np.all(gj < np.uint64(1 << 31))
    ctr = np.uint64(slot << 31) | gj
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    zero = np.zeros_like(ctr)
    p = np.tile(np.arange(E, dtype=np.uint64), (len(gj), 1))
    rows = np.arange(len(gj))
    words = None
    for d in range(E - 1):
        k = E - 1 - d
        if d & 3 == 0:
            words = cr.philox4x32_10((ctr & cr._M32, ctr >> cr._S32, zero + np.uint64(PHILOX_PERM + (d >> 2)), zero),
                                     (seed & 0xFFFFFFFF, seed >> 32))
        r = ((words[d & 3] * np.uint64(k + 1)) >> np.uint64(32)).astype(np.int64)       # word < 2^32, k + 1 <= 16: exact in uint64
        a, b = p[rows, k].copy(), p[rows, r].copy()
        p[rows, k], p[rows, r] = b, a
    return p.astype(np.uint8)


def perm_table(seed, offset, t, m, n, E, cand_offset=0):
    """uint8 ``[m, n, E]``: ``perm`` of every env and of candidates ``cand_offset .. cand_offset + n - 1``."""
    gj = np.arange(n, dtype=np.uint64) + np.uint64(cand_offset)
    return np.stack([perm(seed, offset, t, m, i, gj, E) for i in range(m)])


def identity_table(m, n, E, h=None):
    one = np.broadcast_to(np.arange(E, dtype=np.uint8), (m, n, E))
    return np.ascontiguousarray(one if h is None else np.broadcast_to(one, (h - 1, m, n, E)))


def shuffle(state, ret, table):
    """``state [m, E, n, O]``, ``ret [m, E, n]``, ``table [m, n, E]`` -> the shuffled copies.  Table entries at or above E count as
    E - 1 (the library's documented clamp)."""
    state, ret = np.asarray(state), np.asarray(ret)
    m, E, n = ret.shape
    src = np.minimum(np.asarray(table).astype(np.int64), E - 1).transpose(0, 2, 1)       # [m, E, n]: source block of (i, e, j)
    ii = np.arange(m)[:, None, None]
    jj = np.arange(n)[None, None, :]
    return state[ii, src, jj], ret[ii, src, jj]


def particle_returns64(env, sets, norms, observations, actions, n, tables, discount=1.0, activation="relu"):
    """``[m, E, n]`` float64: the return of the particle that ENDS in block ``e`` of candidate ``j`` of env ``i``.  ``actions`` float64
    ``[h, m n, A]`` (row ``i n + j``), ``tables`` ``[h - 1, m, n, E]``: the permutation behind horizon step ``t``."""
    from oracle import OracleMLPDynamics
    obs = np.asarray(observations, dtype=np.float64)
    m, E = len(obs), len(sets)
    h, A = actions.shape[0], actions.shape[2]
    O = obs.shape[1]
    dyn = OracleMLPDynamics(O, A, list(sets) * m, list(norms) * m, mode="per_block", hidden_nonlinearity=activation)
    act_x = np.broadcast_to(np.asarray(actions, dtype=np.float64).reshape(h, m, 1, n, A), (h, m, E, n, A)).reshape(h, m * E * n, A)
    state = np.repeat(np.repeat(obs, E, axis=0), n, axis=0)            # row (i E + e) n + j
    total = np.zeros(m * E * n)
    for t in range(h):
        a = np.ascontiguousarray(act_x[t])
        nxt = dyn.predict(state, a)
        total = total + discount ** t * env.reward(state, a, nxt)
        state = nxt
        if t < h - 1:
            s, r = shuffle(state.reshape(m, E, n, O), total.reshape(m, E, n), tables[t])
            state, total = np.ascontiguousarray(s).reshape(m * E * n, O), np.ascontiguousarray(r).reshape(m * E * n)
    return total.reshape(m, E, n)
