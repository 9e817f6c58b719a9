"""Plain NumPy restatement of the iCEM planner's noise-as-a-matrix sample (``csrc/l2a_icem.hip``: ``l2a_icem_sample_noise_k``,
``l2a_icem_noise_matrix``; no GPU, no library calls), as ``include/l2a.h`` states it.

The noise sequence of one (candidate, action dimension) is ``nz = M z`` with ``z`` the ``h`` standard normals of that sequence and
``M [h, h]`` any matrix; one fixed order, ``acc = M[t, 0] z_0``, then ``acc = acc + (M[t, s] z_s)`` for ``s = 1 .. h - 1``, and
``a = clip(mu'_t + nz_t sd'_t)``.  Shift, kept rows, the mean row and the layouts are ``icem_reference._sample``'s.
``tests/test_icem_noise_reference.py`` pins every function here before it judges a kernel."""

import numpy as np

import icem_reference as ir


def noise_matrix(h, beta):
    """The power-law matrix ``M [h, h]`` in float64 for a spectral density ``f^-beta``: ``s_k = max(k, 1)^(-beta / 2) h^(beta / 2)``
    for ``k = 0 .. h // 2`` (the DC term gets the lowest frequency's amplitude), mid ``k`` are ``1 .. (h - 1) // 2``,
    ``N = sqrt(s_0^2 + 2 sum_mid s_k^2 + [h even, h > 1] s_(h/2)^2)``; column 0 is ``s_0 / N``, columns ``2k - 1`` and ``2k`` are
    ``sqrt(2) s_k cos(2 pi k t / h) / N`` and ``-sqrt(2) s_k sin(2 pi k t / h) / N``, the last column of an even ``h > 1`` is
    ``s_(h/2) (-1)^t / N``.  (``k t`` is reduced modulo ``h`` in integers: the same angle, below ``2 pi``.)"""
    h, beta = int(h), float(beta)
    half, mid = h // 2, (h - 1) // 2
    nyquist = h % 2 == 0 and h > 1
    s = np.array([float(max(k, 1)) ** (-0.5 * beta) * float(h) ** (0.5 * beta) for k in range(half + 1)])
    total = s[0] * s[0]
    for k in range(1, mid + 1):
        total += 2.0 * (s[k] * s[k])
    if nyquist:
        total += s[half] * s[half]
    N = np.sqrt(total)
    M = np.zeros((h, h))
    for t in range(h):
        M[t, 0] = s[0] / N
        for k in range(1, mid + 1):
            ang = 2.0 * np.pi * float((k * t) % h) / float(h)
            M[t, 2 * k - 1] = np.sqrt(2.0) * s[k] * np.cos(ang) / N
            M[t, 2 * k] = -np.sqrt(2.0) * s[k] * np.sin(ang) / N
        if nyquist:
            M[t, h - 1] = (-s[half] if t % 2 else s[half]) / N
    return M


def mix(M, z, ft):
    """``nz [n, m, h, A]`` from ``z [n, m, h, A]``: ``nz[..., t, :] = sum_s M[t, s] z[..., s, :]`` in the kernel's order, looping over
    ``s`` - in ``ft`` every product and every add is rounded on its own."""
    M = np.asarray(M, dtype=ft)
    h = M.shape[0]
    assert z.dtype == ft and z.shape[2] == h
    nz = np.empty_like(z)
    col = [M[:, s].reshape(1, 1, h, 1) for s in range(h)]
    rows = max(1, 65536 // max(1, z.shape[1] * h * z.shape[3]))        # candidates per block: the arrays of a block stay in cache
    for j0 in range(0, z.shape[0], rows):
        zb = z[j0:j0 + rows]
        acc = col[0] * zb[:, :, 0:1]                                    # every t at once: [rows, m, h, A]
        pr = np.empty_like(acc)
        for s in range(1, h):
            np.multiply(col[s], zb[:, :, s:s + 1], out=pr)
            np.add(acc, pr, out=acc)
        nz[j0:j0 + rows] = acc
    assert nz.dtype == ft and acc.dtype == ft
    return nz


def _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, M, low, high, n, m, h, act_dim, Kk, add_mean, ft):
    D = h * act_dim
    mean_in, std_in = (np.asarray(v, dtype=ft).reshape(m, D) for v in (mean_in, std_in))
    sigma0, low, high = (np.asarray(v, dtype=ft).reshape(act_dim) for v in (sigma0, low, high))
    lowD, highD = np.tile(low, h), np.tile(high, h)
    z = np.asarray(z, dtype=ft).reshape(n, m, h, act_dim)
    mu = np.empty((m, D), dtype=ft)
    sd = np.empty((m, D), dtype=ft)
    for i in range(m):
        s = int(shift[i])
        mu[i] = 0 if s < 0 else ir.shift_rows(mean_in[i], s > 0, h, act_dim)
        sd[i] = np.tile(sigma0, h) if s != 0 else std_in[i]
    mu3, sd3 = mu.reshape(m, h, act_dim), sd.reshape(m, h, act_dim)
    nz = mix(np.asarray(M).reshape(h, h), z, ft)
    sc = nz * sd3[None]
    a = np.minimum(np.maximum(mu3[None] + sc, low), high).reshape(n, m, D)
    for i in range(m):
        kc = ir.kept_count(0 if kc_in is None else kc_in[i], Kk, shift[i])
        for j in range(min(kc, n)):
            a[j, i] = ir.shift_rows(np.asarray(kept_in, dtype=ft).reshape(m, Kk, D)[i, j], int(shift[i]) > 0, h, act_dim)
        if add_mean:
            a[n - 1, i] = np.minimum(np.maximum(mu[i], lowD), highD)
    assert a.dtype == ft and mu.dtype == ft and sd.dtype == ft
    return mu, sd, a, a.reshape(-1)[ir.seq_index(n, m, h, act_dim)]


def sample_noise_f32(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, M, low, high, n, m, h, act_dim, Kk, add_mean):
    """``(mean_out [m, D], std_out [m, D], a_clip [n, m, D], seq [h, m * n, act_dim])`` in fp32 with the kernel's exact operation
    order: the ``h``-term sum over ``s`` (one rounding per product and per add), ``a = mu' + nz * sd'``, ``min(max(a, low), high)``;
    kept rows and the mean row are copies."""
    return _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, M, low, high, n, m, h, act_dim, Kk, add_mean, np.float32)


def sample_noise(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, M, low, high, n, m, h, act_dim, Kk, add_mean):
    """The same in float64 (``M`` as given: pass the fp32 values to restate the kernel's inputs)."""
    return _sample(mean_in, std_in, kept_in, kc_in, shift, z, sigma0, M, low, high, n, m, h, act_dim, Kk, add_mean, np.float64)
