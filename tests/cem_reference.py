"""Plain NumPy float64 restatement of the cross-entropy-method kernels in ``csrc/l2a_cem.hip`` (no GPU, no library calls).

Both readings of ``MPCController.get_cem_action`` (``mpc_controller.py:71-106``) as the kernels' header comment states them:

``reference=True``  the reference's own semantics: the UNCLIPPED samples are rolled out, the candidate-major sample rows
                    ``[n, m, D]`` are fed to the rollout as if they were env-major ``[m, n, D]`` (:88-96), and the elites are
                    the boolean POSITIONS of ``((-returns).argsort() < k).T`` (:101) - sample row ``rank_i(j) * m + i`` for
                    every ``j < k`` -, pooled over the envs and broadcast (:103-104);
``reference=False`` the fixed reading: clipped samples are rolled out, plan row ``i * n + j`` is sample row ``j * m + i``,
                    the elites of env ``i`` are its true top ``k`` candidates, in rank order, statistics per env.

Ranks are the stable descending order with NaN returns mapped to ``-inf`` (ties to the lower index).  ``tests/test_cem_reference.py``
pins every function here against known answers and independent formulations before it judges a kernel."""

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
PHILOX_STREAM = 0x4C32614D           # third counter word of the planner's normal stream


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def philox4x32_10(ctr_words, key_words):
    """Philox4x32-10 (Salmon et al., SC'11).  ``ctr_words``: four, ``key_words``: two 32-bit words (ints or equal-shaped arrays);
    returns the four output words as ``uint64`` arrays holding 32-bit values."""
    c0, c1, c2, c3 = [_u64(w) & _M32 for w in ctr_words]
    k0, k1 = [_u64(w) & _M32 for w in key_words]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def philox_uniforms(seed, indices):
    """The two Box-Muller uniforms of the elements ``indices`` (64-bit counters, wrapping): ``u1`` in (0, 1], ``u2`` in [0, 1),
    both multiples of 2^-24 - exact in fp32 and in float64."""
    idx = _u64(indices)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    zero = np.zeros_like(idx)
    c = philox4x32_10((idx & _M32, idx >> _S32, zero + np.uint64(PHILOX_STREAM), zero), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((c[0] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (c[1] >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def philox_normal(seed, indices):
    """Standard normal of every 64-bit element index: counter ``(lo, hi, 0x4c32614d, 0)``, key ``(seed_lo, seed_hi)``, Box-Muller
    in float64 on the first two output words."""
    u1, u2 = philox_uniforms(seed, indices)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def philox_indices(offset, count):
    """``offset + arange(count)`` modulo 2^64 as ``uint64``."""
    with np.errstate(over="ignore"):
        return np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(count, dtype=np.uint64)


def stable_rank(returns):
    """``returns [m, n]`` -> ``(order, ranks)``: ``order[i, p]`` = the candidate ranked p-th in env i (descending, NaN as -inf,
    ties to the lower index); ``ranks[i, j]`` = the rank of candidate j."""
    r = np.array(returns, dtype=np.float64, ndmin=2)
    r[np.isnan(r)] = -np.inf
    order = np.argsort(-r, axis=1, kind="stable")
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(r.shape[1]), r.shape), axis=1)
    return order, ranks


def elite_rows(returns, k, reference):
    """Flat sample rows (into ``[n * m, D]``) of every env's elites, ``[m, k]``.  Reference reading: entry ``[i, j]`` is position
    ``rank_i(j)`` as row ``rank * m + i`` (a SET per env: compare sorted); fixed reading: ``order[i, :k] * m + i`` in rank order."""
    order, ranks = stable_rank(returns)
    env = np.arange(order.shape[0])[:, None]
    return (ranks[:, :k] if reference else order[:, :k]) * order.shape[0] + env


def refit(mean, a_clip, returns, k, alpha, reference):
    """``(new_mean [m, D], new_std [m, D], rows [m, k])`` from the samples ``a_clip [n, m, D]`` and their ``returns [m, n]``: elite
    mean and biased std in float64 (pooled over the envs and broadcast in the reference reading, per env in the fixed one) and
    ``mean * alpha + (1 - alpha) * elite_mean`` with the fp32 value of ``alpha`` the kernels receive."""
    mean = np.asarray(mean, dtype=np.float64)
    m, D = mean.shape
    flat = np.asarray(a_clip, dtype=np.float64).reshape(-1, D)
    rows = elite_rows(returns, k, reference)
    if reference:
        pooled = flat[rows.reshape(-1)]
        mu = np.broadcast_to(pooled.mean(axis=0), (m, D))
        sd = np.broadcast_to(pooled.std(axis=0), (m, D))
    else:
        per_env = flat[rows]                            # [m, k, D]
        mu, sd = per_env.mean(axis=1), per_env.std(axis=1)
    alpha64 = np.float64(np.float32(alpha))
    return mean * alpha64 + (1.0 - alpha64) * mu, np.array(sd), rows


def seq_index(n, m, h, act_dim, reference, lo, hi):
    """For every element of the rollout's candidate tensor ``seq [h, m * (hi - lo), act_dim]`` the flat index of the sample element
    (in ``[n, m, D]``) it holds.  Plan row ``r = i * n + j`` (env block i, candidate j) reads sample row ``r`` in the reference
    reading - the sample memory taken as ``[m, n, D]`` (:94-96) - and sample row ``j * m + i`` in the fixed one."""
    D = h * act_dim
    i = np.arange(m)[None, :, None, None]
    j = np.arange(lo, hi)[None, None, :, None]
    t = np.arange(h)[:, None, None, None]
    kk = np.arange(act_dim)[None, None, None, :]
    row = (i * n + j) if reference else (j * m + i)
    return (row * D + t * act_dim + kk).reshape(h, m * (hi - lo), act_dim)


def sample(mean, std, z, low, high, n, m, h, act_dim, reference, lo, hi):
    """``(a_raw [n, m, D], a_clip [n, m, D], seq [h, m * (hi - lo), act_dim])`` in float64: ``a = mean + z * std`` (:86), clipped per
    action dimension (:87); ``seq`` holds the unclipped samples (reference reading) or the clipped ones (fixed reading) of the
    candidates ``[lo, hi)``."""
    D = h * act_dim
    mean, std = np.asarray(mean, dtype=np.float64).reshape(m, D), np.asarray(std, dtype=np.float64).reshape(m, D)
    a_raw = mean[None] + np.asarray(z, dtype=np.float64).reshape(n, m, D) * std[None]
    a_clip = clip(a_raw, low, high, h)
    src = a_raw if reference else a_clip
    return a_raw, a_clip, src.reshape(-1)[seq_index(n, m, h, act_dim, reference, lo, hi)]


def clip(a, low, high, h):
    """``np.clip`` of ``a [..., h * act_dim]`` to the per-action bounds repeated over the horizon (:81-82, :87), in ``a``'s dtype."""
    return np.clip(a, np.tile(np.asarray(low, dtype=a.dtype), h), np.tile(np.asarray(high, dtype=a.dtype), h))


def pick(returns, cand, n, m, D, act_dim, reference):
    """``(index [m], return [m], action [m, act_dim])``: ``np.argmax`` per env (the first NaN wins, else the first maximum), the
    first action of that candidate - row ``i * n + j`` of ``cand`` in the reference reading, ``j * m + i`` in the fixed one."""
    returns = np.asarray(returns).reshape(m, n)
    idx = np.argmax(returns, axis=1)
    env = np.arange(m)
    row = env * n + idx if reference else idx * m + env
    return idx, returns[env, idx], np.asarray(cand).reshape(n * m, D)[row, :act_dim]


def stats_bounds(cnt, a_clip_in, mean_in):
    """Derived fp32 error bounds of the kernels' elite statistics, ``(mean_bound, std_bound)``:
    ``gamma = (ceil(cnt / 32) + 16) * 2^-24`` - the longest accumulator chain (cnt / 32 adds), 2 adds joining the four
    accumulators, 8 slice adds, the division, and ``1 - alpha``, the product and the sum of the update -, ``B`` the largest input
    magnitude; ``|mean - ref| <= gamma * B`` and ``|std - ref| <= 2 * gamma * B`` (the std picks up the mean's error once and the
    squared sums' relative error once)."""
    gamma = (-(-int(cnt) // 32) + 16) * 2.0 ** -24
    B = max(float(np.max(np.abs(a_clip_in))), float(np.max(np.abs(mean_in))))
    return gamma * B, 2.0 * gamma * B
