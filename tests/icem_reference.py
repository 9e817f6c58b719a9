"""Plain NumPy restatement of the iCEM planner kernels in ``csrc/l2a_icem.hip`` (no GPU, no library calls), as ``include/l2a.h``
states their semantics: fp32 operation by operation for the sample, float64 for the refit.

Per env ``i``: a plan mean ``mu[i]`` and a spread ``sd[i]`` of shape ``[h, A]`` (``D = h * A``), kept elite rows ``kept[i] [Kk, D]`` and
their count ``kc[i]``.  One iteration: shift (``shift[i] < 0``: ``mu' = 0``, ``sd' = sigma0``, no kept rows; ``> 0``: mean and kept rows
move on one step with the last step repeated, ``sd' = sigma0``; ``0``: all kept), place the kept rows (row ``j < kc'``) and, with
``add_mean``, the clipped mean as row ``n_it - 1`` (it wins over a kept row), draw every other row with AR(1) noise
(``nz_0 = z_0``, ``nz_t = rho nz_(t-1) + c z_t``, ``c = sqrt(1 - rho^2)``) as ``clip(mu' + nz sd')``; then the elites - the top
``min(K, valid)`` valid candidates (return neither NaN nor ``-inf``) in the stable descending order - refit mean and spread with
momentum ``alpha`` and the first ``Kk`` of them are kept.  Sample rows are candidate-major (``[n_it, m, D]``: row ``j * m + i``), plan
rows env-major (``i * n_it + j``): ``cem_reference``'s fixed reading.  ``tests/test_icem_reference.py`` pins every function here before
it judges a kernel."""

import numpy as np

import cem_reference as cr
from cem_reference import philox_indices, philox_normal     # noqa: F401  (the planner's normal stream is CEM's)

REFIT_STATIC_LDS = 4288         # include/l2a.h: L2A_ICEM_REFIT_STATIC_LDS (bytes of LDS l2a_icem_stats_k holds besides its K ints)


def sizes(n, percent_elites, keep, decay, iters):
    """``(K, Kk, [n_it for it in range(iters)])``: ``K = max(int(n * percent_elites), 1)``, ``Kk = int(keep * K)``,
    ``n_it = min(n, max(int(n / decay ** it), 2 K))`` - Python floats, i.e. double precision."""
    K = max(int(n * percent_elites), 1)
    Kk = int(keep * K)
    return K, Kk, [population(n, K, decay, it) for it in range(iters)]


def population(n, K, decay, it):
    return min(int(n), max(int(n / float(decay) ** it), 2 * int(K)))


def shift_rows(x, shift_on, h, act_dim):
    """``x [..., D]`` moved on one step with the last step repeated where ``shift_on``, in ``x``'s dtype."""
    x = np.asarray(x)
    if not shift_on:
        return x.copy()
    t1 = np.minimum(np.arange(h) + 1, h - 1)
    return x.reshape(x.shape[:-1] + (h, act_dim))[..., t1, :].reshape(x.shape)


def seq_index(n, m, h, act_dim):
    """For every element of the rollout's candidate tensor ``seq [h, m * n, act_dim]`` the flat index of the sample element (in
    ``[n, m, D]``) it holds: plan row ``i * n + j`` is sample row ``j * m + i``."""
    return cr.seq_index(n, m, h, act_dim, False, 0, n)


def noise_constants(rho):
    """``(rho, c)`` as the fp32 values the kernel receives: ``c = sqrtf(1 - rho * rho)``, every operation rounded to fp32."""
    r = np.float32(rho)
    return r, np.float32(np.sqrt(np.float32(np.float32(1.0) - np.float32(r * r))))


def kept_count(kc, Kk, shift):
    """``kc'``: 0 for a fresh env (``shift < 0``) or ``Kk = 0``, else the stored count held to ``0 .. Kk``."""
    return 0 if (Kk == 0 or int(shift) < 0) else int(min(max(int(kc), 0), Kk))


def _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, rho, low, high, n, m, h, act_dim, Kk, add_mean, ft):
    D = h * act_dim
    mean_in, std_in = (np.asarray(v, dtype=ft).reshape(m, D) for v in (mean_in, std_in))
    sigma0, low, high = (np.asarray(v, dtype=ft).reshape(act_dim) for v in (sigma0, low, high))
    lowD, highD = np.tile(low, h), np.tile(high, h)
    z = np.asarray(z, dtype=ft).reshape(n, m, h, act_dim)
    r32, c32 = noise_constants(rho)
    rho_t, c_t = ft(r32), ft(c32)
    mu = np.empty((m, D), dtype=ft)
    sd = np.empty((m, D), dtype=ft)
    for i in range(m):
        s = int(shift[i])
        mu[i] = 0 if s < 0 else shift_rows(mean_in[i], s > 0, h, act_dim)
        sd[i] = np.tile(sigma0, h) if s != 0 else std_in[i]
    mu3, sd3 = mu.reshape(m, h, act_dim), sd.reshape(m, h, act_dim)
    a = np.empty((n, m, h, act_dim), dtype=ft)
    nz = None
    for t in range(h):
        if t == 0:
            nz = z[:, :, 0].copy()
        else:
            rn = rho_t * nz
            cz = c_t * z[:, :, t]
            nz = rn + cz
        sc = nz * sd3[None, :, t]
        a[:, :, t] = np.minimum(np.maximum(mu3[None, :, t] + sc, low), high)
    a = a.reshape(n, m, D)
    for i in range(m):
        kc = kept_count(0 if kc_in is None else kc_in[i], Kk, shift[i])
        for j in range(min(kc, n)):
            a[j, i] = shift_rows(np.asarray(kept_in, dtype=ft).reshape(m, Kk, D)[i, j], int(shift[i]) > 0, h, act_dim)
        if add_mean:
            a[n - 1, i] = np.minimum(np.maximum(mu[i], lowD), highD)
    assert a.dtype == ft and mu.dtype == ft and sd.dtype == ft
    return mu, sd, a, a.reshape(-1)[seq_index(n, m, h, act_dim)]


def sample_f32(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, rho, low, high, n, m, h, act_dim, Kk, add_mean):
    """``(mean_out [m, D], std_out [m, D], a_clip [n, m, D], seq [h, m * n, act_dim])`` in fp32 with the kernel's exact operation
    order - every product, sum, maximum and minimum rounded to fp32 on its own: ``nz = rho * nz + c * z`` (``nz_0 = z_0``),
    ``a = mu' + nz * sd'``, ``min(max(a, low), high)``; kept rows and the mean row are copies."""
    return _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, rho, low, high, n, m, h, act_dim, Kk, add_mean, np.float32)


def sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, rho, low, high, n, m, h, act_dim, Kk, add_mean):
    """The same in float64 (with the fp32 values of ``rho`` and ``c`` the kernel uses)."""
    return _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, rho, low, high, n, m, h, act_dim, Kk, add_mean, np.float64)


def recurrence_coefficients(rho, h):
    """``C [h, h]`` (float64) with ``nz_t = sum_s C[t, s] z_s``: ``C[t, 0] = rho^t``, ``C[t, s] = sqrt(1 - rho^2) rho^(t - s)`` for
    ``1 <= s <= t`` - the recurrence written out."""
    rho = float(rho)
    c = np.sqrt(1.0 - rho * rho)
    C = np.zeros((h, h))
    for t in range(h):
        C[t, 0] = rho ** t
        for s in range(1, t + 1):
            C[t, s] = c * rho ** (t - s)
    return C


def recurrence(z, rho):
    """The recurrence itself in float64 over ``z [..., h, A]`` with the exact ``c = sqrt(1 - rho^2)``."""
    z = np.asarray(z, dtype=np.float64)
    c = np.sqrt(1.0 - float(rho) ** 2)
    out = np.empty_like(z)
    out[..., 0, :] = z[..., 0, :]
    for t in range(1, z.shape[-2]):
        out[..., t, :] = float(rho) * out[..., t - 1, :] + c * z[..., t, :]
    return out


def valid_mask(returns):
    r = np.array(returns, dtype=np.float64, ndmin=2)
    return ~np.isnan(r) & (r != -np.inf)


def elites(returns, K):
    """Per env the candidate indices of the elites in rank order (a list of int arrays) and the valid counts ``[m]``: the top
    ``min(K, valid)`` valid candidates, descending, ties to the lower index (rank counting over all pairs - no sort)."""
    r = np.array(returns, dtype=np.float64, ndmin=2)
    ok = valid_mask(r)
    out = []
    for i in range(r.shape[0]):
        cand = np.flatnonzero(ok[i])
        v = r[i, cand]
        before = (v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (cand[None, :] < cand[:, None]))
        rank = before.sum(axis=1)                       # the candidates that sort before each one: a permutation of 0 .. valid - 1
        order = np.empty(len(cand), dtype=np.int64)
        order[rank] = cand
        out.append(order[:min(K, len(cand))])
    return out, ok.sum(axis=1)


def refit(mean, std, a_clip, returns, K, Kk, alpha, low, high, act_dim, ranked=None):
    """What ``l2a_icem_refit`` leaves, as a dict: ``mean`` / ``std`` ``[m, D]`` float64 (``alpha mu' + (1 - alpha) em`` and the same
    for the biased elite std, with the fp32 value of ``alpha``; an env without an elite keeps both), ``elites`` (list of index arrays),
    ``Ke``, ``valid``, ``kept`` (list of ``[min(Kk, Ke), D]`` rows of ``a_clip``, exact copies), ``kc``, ``index`` (-1), ``best_return``
    (fp32, NaN), ``action [m, act_dim]`` (fp32: the best candidate's first action, or ``mu'``'s clipped first step).  ``ranked``: what
    ``elites(returns, K')`` gave for some ``K' >= K`` (its lists are cut to ``K`` here instead of being counted again)."""
    mean32, std32 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    m, D = mean32.shape
    a32 = np.asarray(a_clip, dtype=np.float32).reshape(-1, m, D)
    r32 = np.array(returns, dtype=np.float32, ndmin=2)
    el, valid = elites(r32, K) if ranked is None else ([e[:K] for e in ranked[0]], ranked[1])
    al = np.float64(np.float32(alpha))
    new_mean, new_std = mean32.astype(np.float64), std32.astype(np.float64)
    low, high = np.asarray(low, dtype=np.float32), np.asarray(high, dtype=np.float32)
    kept, kc = [], np.zeros(m, dtype=np.int64)
    index = np.full(m, -1, dtype=np.int64)
    best = np.full(m, np.nan, dtype=np.float32)
    action = np.empty((m, act_dim), dtype=np.float32)
    for i in range(m):
        e = el[i]
        kc[i] = min(Kk, len(e))
        kept.append(a32[e[:kc[i]], i].copy())
        if len(e) == 0:
            action[i] = np.minimum(np.maximum(mean32[i, :act_dim], low), high)
            continue
        rows = a32[e, i].astype(np.float64)
        new_mean[i] = al * new_mean[i] + (1.0 - al) * rows.mean(axis=0)
        new_std[i] = al * new_std[i] + (1.0 - al) * rows.std(axis=0)
        index[i], best[i], action[i] = e[0], r32[i, e[0]], a32[e[0], i, :act_dim]
    return dict(mean=new_mean, std=new_std, elites=el, Ke=np.array([len(e) for e in el]), valid=valid, kept=kept, kc=kc, index=index,
                best_return=best, action=action)


def sum_chain(Ke):
    """``L(Ke)``: the longest sequential add chain of l2a_icem_stats_k's summation order (its header comment): an accumulator's
    ``ceil(Ke / 128)`` adds, 2 adds joining the four accumulators, 32 slice adds."""
    return -(-int(Ke) // 128) + 34


def refit_bounds(Ke, B, L=None):
    """Derived fp32 error bounds of ``l2a_icem_refit``'s statistics, ``(mean_bound, std_bound)``, with ``B`` the largest magnitude
    among the samples, ``mu'`` and ``sd'`` and ``gamma = (L(Ke) + 8) 2^-24``.

    Elite mean: a chain of ``L`` fp32 additions of values within ``[-B, B]`` is off by at most ``L 2^-24`` of the sum of the
    magnitudes, so ``|em - ref| <= (L + 1) 2^-24 B`` with the division.  The update ``alpha mu' + (1 - alpha) em`` adds the
    rounding of ``1 - alpha``, two products and a sum on terms of magnitude at most ``B``: ``4 2^-24 B``; 3 more cover second-order
    terms: ``|mu - ref| <= gamma B``.

    Elite std: the computed mean is off by ``eps <= gamma B``, and ``mean((x - em - eps)^2) = var + eps^2`` exactly, so the
    square root moves by at most ``eps`` (``sqrt(v + eps^2) - sqrt(v) <= eps``); the sum of the (non-negative) squares carries a
    relative error of at most ``(L + 4) 2^-24`` (the chain, the difference's rounding twice, the division), half of it after the
    root, on a std of at most ``B``; the update adds ``4 2^-24 B``: ``|sd - ref| <= 2 gamma B``."""
    L = sum_chain(Ke) if L is None else int(L)
    gamma = (L + 8) * 2.0 ** -24
    return gamma * float(B), 2.0 * gamma * float(B)
