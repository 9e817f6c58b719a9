"""Plain NumPy restatement of the reward-weighted (MPPI) planner kernels in ``csrc/l2a_mppi.hip`` (no GPU, no library calls), as
``include/l2a.h`` states their semantics.

Per env ``i`` a plan mean ``mu[i]`` of shape ``[h, A]`` (``D = h * A``).  One iteration: shift the mean (``shift[i] < 0``: zeros;
``> 0``: ``mu'_t = mu_min(t + 1, h - 1)``; ``0``: kept), filter the scaled normals over the horizon
(``u = z * sigma_k``, ``n_t = beta * u_t + (1 - beta) * n_(t-1)``, ``n_(-1) = 0``), clip ``mu' + n`` to the action bounds; weigh
the candidates by their returns (``w = exp(kappa * (R - Rmax))`` over the valid ones - neither NaN nor ``-inf``) and take the weighted
mean of the clipped samples.  Sample rows are candidate-major (``[n, m, D]``: row ``j * m + i``), plan rows env-major (``i * n + j``):
``cem_reference``'s fixed reading.  ``tests/test_mppi_reference.py`` pins every function here before it judges a kernel."""

import numpy as np

import cem_reference as cr
from cem_reference import philox_indices, philox_normal     # noqa: F401  (the planner's normal stream is CEM's)

UPDATE_STATIC_LDS = 4480        # include/l2a.h: L2A_MPPI_UPDATE_STATIC_LDS (bytes of LDS l2a_mppi_update_k holds besides its n floats)


def shift_mean(mean, shift, h, act_dim):
    """``mu' [m, D]`` in ``mean``'s dtype: row i zeroed (``shift[i] < 0``), moved on one step with the last step repeated (``> 0``) or
    kept (``0``)."""
    mean = np.asarray(mean)
    m = mean.shape[0]
    mu = mean.reshape(m, h, act_dim)
    t1 = np.minimum(np.arange(h) + 1, h - 1)
    out = np.empty_like(mu)
    for i in range(m):
        s = int(shift[i])
        out[i] = 0 if s < 0 else (mu[i, t1] if s > 0 else mu[i])
    return out.reshape(m, h * act_dim)


def seq_index(n, m, h, act_dim):
    """For every element of the rollout's candidate tensor ``seq [h, m * n, act_dim]`` the flat index of the sample element (in
    ``[n, m, D]``) it holds: plan row ``i * n + j`` is sample row ``j * m + i``."""
    return cr.seq_index(n, m, h, act_dim, False, 0, n)


def _sample(mean_in, shift, z, sigma, beta, low, high, n, m, h, act_dim, ft):
    D = h * act_dim
    mu = shift_mean(np.asarray(mean_in, dtype=ft).reshape(m, D), shift, h, act_dim)
    z = np.asarray(z, dtype=ft).reshape(n, m, h, act_dim)
    sigma, low, high = (np.asarray(v, dtype=ft).reshape(act_dim) for v in (sigma, low, high))
    beta = ft(np.float32(beta))                         # the fp32 value the kernel receives
    omb = ft(np.float32(1.0) - np.float32(beta))        # 1 - beta, formed once in fp32
    a = np.empty((n, m, h, act_dim), dtype=ft)
    nz = np.zeros((n, m, act_dim), dtype=ft)
    mu3 = mu.reshape(m, h, act_dim)
    for t in range(h):
        u = z[:, :, t] * sigma
        bu = beta * u
        kn = omb * nz
        nz = bu + kn
        a[:, :, t] = np.minimum(np.maximum(mu3[None, :, t] + nz, low), high)
    a = a.reshape(n, m, D)
    assert a.dtype == ft and mu.dtype == ft
    return mu, a, a.reshape(-1)[seq_index(n, m, h, act_dim)]


def sample_f32(mean_in, shift, z, sigma, beta, low, high, n, m, h, act_dim):
    """``(mean_out [m, D], a_clip [n, m, D], seq [h, m * n, act_dim])`` in fp32 with the kernel's exact operation order - every
    product, sum, maximum and minimum rounded to fp32 on its own (``np.float32`` arithmetic): ``u = z * sigma``,
    ``nz = beta * u + omb * nz``, ``a = mu' + nz``, ``min(max(a, low), high)``."""
    return _sample(mean_in, shift, z, sigma, beta, low, high, n, m, h, act_dim, np.float32)


def sample(mean_in, shift, z, sigma, beta, low, high, n, m, h, act_dim):
    """The same in float64 (with the fp32 values of ``beta`` and ``1 - beta`` the kernel uses)."""
    return _sample(mean_in, shift, z, sigma, beta, low, high, n, m, h, act_dim, np.float64)


def filter_closed_form(u, beta):
    """``n_t = sum_(s <= t) beta (1 - beta)^(t - s) u_s`` for ``u [..., h, A]`` (float64) - the recurrence written out."""
    u = np.asarray(u, dtype=np.float64)
    h = u.shape[-2]
    out = np.zeros_like(u)
    for t in range(h):
        for s in range(t + 1):
            out[..., t, :] += beta * (1.0 - beta) ** (t - s) * u[..., s, :]
    return out


def weights(returns, kappa):
    """``(w [m, n] float64, rmax [m] fp32, index [m], valid [m])`` from fp32 ``returns [m, n]``.  Valid = neither NaN nor ``-inf``;
    invalid candidates weigh 0.  ``rmax`` = the largest valid return (NaN without one), ``index`` its first position (-1).
    ``rmax = +inf``: 1 for the ``+inf`` returns, 0 otherwise.  Else ``exp(kappa * (R - rmax))`` in float64 with the fp32 value of
    ``kappa``; a difference that overflows fp32 (``-inf`` there) gives 0."""
    r32 = np.array(returns, dtype=np.float32, ndmin=2)
    m, n = r32.shape
    r = r32.astype(np.float64)
    ok = ~np.isnan(r) & (r != -np.inf)
    valid = ok.sum(axis=1)
    w = np.zeros((m, n))
    rmax = np.full(m, np.nan, dtype=np.float32)
    index = np.full(m, -1, dtype=np.int64)
    k64 = np.float64(np.float32(kappa))
    for i in range(m):
        if valid[i] == 0:
            continue
        masked = np.where(ok[i], r[i], -np.inf)
        index[i] = int(np.argmax(masked))               # first maximum
        rmax[i] = r32[i, index[i]]                      # (its own bits: -0.0 stays -0.0)
        top = r[i, index[i]]
        if top == np.inf:
            w[i] = np.where(ok[i] & (r[i] == np.inf), 1.0, 0.0)
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.where(ok[i], r[i] - top, -np.inf)
            d = np.where(np.isinf(d.astype(np.float32)), -np.inf, d)    # the fp32 difference overflowed
            w[i] = np.where(ok[i], np.exp(k64 * d), 0.0)
    return w, rmax, index, valid


def update(mean, a_clip, returns, kappa):
    """``(new_mean [m, D] float64, w, rmax, index, valid, ess [m])``: ``mu[i, d] = sum_j w_j a[j, i, d] / sum_j w_j`` over the
    samples ``a_clip [n, m, D]``; an env without a valid candidate keeps ``mean[i]``.  ``ess = (sum w)^2 / sum w^2`` (0 for such
    an env)."""
    mean = np.asarray(mean, dtype=np.float64)
    m, D = mean.shape
    a = np.asarray(a_clip, dtype=np.float64).reshape(-1, m, D)
    w, rmax, index, valid = weights(returns, kappa)
    new = mean.copy()
    ess = np.zeros(m)
    for i in range(m):
        if valid[i] == 0:
            continue
        s = w[i].sum()
        new[i] = (w[i][:, None] * a[:, i]).sum(axis=0) / s
        ess[i] = s * s / (w[i] * w[i]).sum()
    return new, w, rmax, index, valid, ess


def result_row(mean, a_clip, returns, kappa, act_dim):
    """The packed result ``l2a_mppi_update`` writes, as a dict of per-env arrays: ``action [m, act_dim]`` (new ``mu[i, 0, :]``,
    float64), ``rmax`` (fp32, NaN for a degenerate env), ``index`` (-1), ``ess`` (0), ``valid``; and ``mean``, the new mean."""
    new, _, rmax, index, valid, ess = update(mean, a_clip, returns, kappa)
    return dict(action=new[:, :act_dim].copy(), rmax=rmax, index=index, ess=ess, valid=valid, mean=new)


def sum_chain(n):
    """``L(n)``: the longest sequential add chain of l2a_mppi_update_k's summation order (its header comment): an accumulator's
    ``ceil(n / 128)`` fused multiply-adds, at most 3 more from the tail loop, 2 adds joining the four accumulators, 32 slice adds."""
    return -(-int(n) // 128) + 37


def update_bounds(n, kappa, B, L=None):
    """Derived fp32 error bounds of ``l2a_mppi_update``: ``(mean_bound, ess_relative_bound)`` with
    ``|mu - ref| <= (2 gamma_w + 2 gamma_s) B`` and ``|ess - ref| <= (2 gamma_w + 2 gamma_s) ref``.

    ``gamma_s = (L(n) + 16) 2^-24``: numerator and denominator are sums of non-negative weights times values of magnitude at most
    ``B``; a chain of ``L`` fp32 additions (``sum_chain``) is off by at most ``L 2^-24`` of the sum of the magnitudes, the 16 covers
    the products, the division and second-order terms.  One ``gamma_s`` each for numerator and denominator.

    ``gamma_w = 104 2^-24 + 2 2^-24``, the relative error of one weight: the argument ``kappa * (R - Rmax)`` is rounded to fp32 and
    any weight that is not flushed to zero has ``|kappa d| <= 104`` (``exp(-104) < 2^-149``), so the rounding moves the argument
    by at most ``104 2^-24`` and the weight by that fraction; ``expf`` itself is good to 1 ulp = ``2 2^-24`` relative (the figure HIP's
    math-function accuracy table gives for ``expf``).  The argument in fact takes two roundings (the difference, then the
    product), ``208 2^-24`` at worst; the stated bound still holds, because a relative weight error ``delta_j`` moves the weighted
    mean by ``sum_j delta_j w_j (a_j - mu) / sum w``, at most ``max |delta| B`` (the weighted mean absolute deviation of values in
    ``[-B, B]`` is at most ``B``): ``(208 + 2) 2^-24 B <= 2 gamma_w B``.  A weight in the denormal range (argument below -87.3)
    carries an absolute error of up to ``2^-149`` instead; against ``sum w >= 1`` that is nothing.

    ``kappa`` does not enter: the cap of 104 on the argument holds for every ``kappa``.  ``B``: the largest ``|a|`` of the case."""
    L = sum_chain(n) if L is None else int(L)
    gamma_s = (L + 16) * 2.0 ** -24
    gamma_w = 104 * 2.0 ** -24 + 2 * 2.0 ** -24
    rel = 2.0 * gamma_w + 2.0 * gamma_s
    return rel * float(B), rel
