"""``tests/icem_noise_reference.py`` against known answers and independent formulations (CPU only): the power-law matrix's unit row
norms, circulant covariance and white limit, the identity matrix against ``icem_reference.sample_f32`` at ``rho = 0``, the
recurrence written as a matrix against the float64 AR(1) sample, and the rows that are copies."""

import numpy as np
import pytest

import icem_noise_reference as nr
import icem_reference as ir

HS = (1, 2, 3, 4, 7, 30, 33, 128)
BETAS = (0.0, 1.0, 2.0, 4.0)
WIDE = 1e9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------- the power-law matrix
@pytest.mark.parametrize("h", HS)
def test_matrix_rows_have_unit_norm_and_the_covariance_is_circulant(h):
    """Independent unit normals: ``Cov nz = M M^T``.  Unit diagonal = unit variance at every step (what the AR(1) noise has);
    ``(M M^T)[t, u]`` a function of ``(t - u) mod h`` = a stationary process; every column is used; ``|M| <= 1``."""
    for beta in BETAS:
        M = nr.noise_matrix(h, beta)
        assert M.shape == (h, h) and M.dtype == np.float64
        np.testing.assert_allclose((M * M).sum(axis=1), np.ones(h), rtol=0, atol=1e-15)
        C = M @ M.T
        lag = (np.arange(h)[:, None] - np.arange(h)[None, :]) % h
        assert np.max(np.abs(C - C[lag, 0])) <= 1e-14, (h, beta)
        assert np.all(np.abs(M).max(axis=0) > 0), "an unused column"
        assert np.max(np.abs(M)) <= 1.0
        if beta == 0.0:
            np.testing.assert_allclose(M.T @ M, np.eye(h), rtol=0, atol=1e-14)       # orthogonal: white noise
    if h == 2:          # s_0 = s_1 for every beta: white
        for beta in BETAS:
            np.testing.assert_allclose(nr.noise_matrix(2, beta), nr.noise_matrix(2, 0.0), rtol=0, atol=4e-16)


def test_matrix_known_entries_and_lag_one_correlations():
    assert np.array_equal(nr.noise_matrix(1, 3.0), np.ones((1, 1)))
    r = np.sqrt(0.5)
    np.testing.assert_allclose(nr.noise_matrix(2, 1.0), np.array([[r, r], [r, -r]]), rtol=0, atol=4e-16)
    # h = 3, beta = 0: the real Fourier basis (1, sqrt(2) cos, -sqrt(2) sin) / sqrt(3)
    t = np.arange(3)
    want = np.stack([np.ones(3), np.sqrt(2) * np.cos(2 * np.pi * t / 3), -np.sqrt(2) * np.sin(2 * np.pi * t / 3)], axis=1) / np.sqrt(3)
    np.testing.assert_allclose(nr.noise_matrix(3, 0.0), want, rtol=0, atol=1e-15)
    # the spectrum: the squared column norms over frequency fall as k^-beta (DC takes the lowest frequency's amplitude)
    M = nr.noise_matrix(30, 2.0)
    power = (M * M).sum(axis=0)
    assert abs(power[0] / (power[1] + power[2]) - 0.5) < 1e-12
    for k in (2, 5, 14):
        assert abs((power[2 * k - 1] + power[2 * k]) / (power[1] + power[2]) - k ** -2.0) < 1e-12
    assert abs(power[29] / (power[1] + power[2]) - 0.5 * 15 ** -2.0) < 1e-12
    for beta, want in ((1.0, 0.565), (2.0, 0.883), (4.0, 0.979)):
        M = nr.noise_matrix(30, beta)
        assert abs((M @ M.T)[1, 0] - want) < 5e-4, beta


# ------------------------------------------------------------------------------------------------------------------- the sample
def _inputs(rs, n, m, h, ad, Kk):
    D = h * ad
    low, high = np.linspace(-0.8, -0.3, ad).astype(np.float32), np.linspace(0.4, 0.9, ad).astype(np.float32)
    return dict(mean=(0.7 * rs.randn(m, D)).astype(np.float32), std=(0.05 + 0.6 * rs.rand(m, D)).astype(np.float32),
                kept=np.clip((0.5 * rs.randn(m, max(Kk, 1), D)).astype(np.float32), np.tile(low, h), np.tile(high, h))[:, :Kk],
                sigma0=(0.1 + 0.5 * rs.rand(ad)).astype(np.float32), low=low, high=high, z=rs.randn(n, m, D).astype(np.float32))


def test_identity_matrix_is_the_white_ar1_sample_as_values():
    """``M = I``: every sum is ``z_t`` plus signed zeros, so the fp32 sample equals ``icem_reference.sample_f32`` at ``rho = 0`` as
    values - with shifts, kept rows and the mean row in play."""
    rs = np.random.RandomState(31)
    for n, m, h, ad, Kk, shift, kc, add_mean in ((9, 3, 7, 4, 2, [1, 0, -1], [2, 1, 2], 1), (5, 1, 1, 3, 0, [0], None, 0),
                                                  (6, 2, 30, 6, 3, [0, 1], [3, 0], 0)):
        inp = _inputs(rs, n, m, h, ad, Kk)
        shift = np.asarray(shift, dtype=np.int32)
        kept = inp["kept"] if Kk else None
        got = nr.sample_noise_f32(inp["mean"], inp["std"], kept, kc, shift, inp["z"], inp["sigma0"], np.eye(h), inp["low"], inp["high"],
                                  n, m, h, ad, Kk, add_mean)
        want = ir.sample_f32(inp["mean"], inp["std"], kept, kc, shift, inp["z"], inp["sigma0"], 0.0, inp["low"], inp["high"],
                             n, m, h, ad, Kk, add_mean)
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("rho", [0.5, 0.96875])
@pytest.mark.parametrize("h", [1, 2, 9, 30])
def test_recurrence_as_a_matrix_is_the_float64_ar1_sample(rho, h):
    """``M = recurrence_coefficients(rho, h)`` (rounded to fp32, as a caller would upload it) on fresh envs with ``sigma0 = 1`` and
    bounds far away: ``a = 0 + nz * 1`` is ``nz`` itself, the value before the clip.  Against the float64 recurrence
    (``icem_reference.recurrence``) the fp32 sum of row t is off by at most ``(h + 2) 2^-24 max|z| sum_s |M[t, s]|``:
    rounding ``M[t, s]`` to fp32 moves each term by at most ``2^-24 |M[t, s] z_s|``, so does rounding the product, and each of the
    ``h - 1`` adds moves its partial sum - at most ``sum_s |M[t, s] z_s|`` in magnitude - by at most ``2^-24`` of it: together
    ``(h + 1) 2^-24 sum_s |M[t, s]| |z_s|``; the last unit covers the second-order terms and the float64 side's own rounding."""
    rs = np.random.RandomState(32 + h)
    n, m, ad = 6, 2, 3
    z = rs.randn(n, m, h * ad).astype(np.float32)
    C = ir.recurrence_coefficients(rho, h)
    big = np.full(ad, WIDE, dtype=np.float32)
    zero = np.zeros((m, h * ad), dtype=np.float32)
    _, _, a, _ = nr.sample_noise_f32(zero, zero, None, None, -np.ones(m, dtype=np.int32), z, np.ones(ad, dtype=np.float32),
                                     C.astype(np.float32), -big, big, n, m, h, ad, 0, 0)
    want = ir.recurrence(z.reshape(n, m, h, ad), rho)
    bound = (h + 2) * 2.0 ** -24 * float(np.max(np.abs(z))) * np.abs(C).sum(axis=1)
    err = np.abs(a.reshape(n, m, h, ad).astype(np.float64) - want).max(axis=(0, 1, 3))
    assert np.all(err <= bound), (err / bound).max()
    # and the float64 twin is that product up to float64 rounding
    _, _, a64, _ = nr.sample_noise(zero, zero, None, None, -np.ones(m, dtype=np.int32), z, np.ones(ad), C, -big, big, n, m, h, ad, 0, 0)
    assert a64.dtype == np.float64
    np.testing.assert_allclose(a64.reshape(n, m, h, ad), want, rtol=0, atol=1e-13)


def test_fp32_sample_follows_the_float64_twin_on_a_random_matrix():
    rs = np.random.RandomState(33)
    n, m, h, ad, Kk = 7, 2, 11, 5, 2
    inp = _inputs(rs, n, m, h, ad, Kk)
    M = rs.randn(h, h).astype(np.float32)
    args = (inp["mean"], inp["std"], inp["kept"], [2, 1], np.array([0, 1], dtype=np.int32), inp["z"], inp["sigma0"], M, inp["low"],
            inp["high"], n, m, h, ad, Kk, 1)
    a32, a64 = nr.sample_noise_f32(*args)[2], nr.sample_noise(*args)[2]
    scale = (h + 4) * 2.0 ** -24 * (1.0 + float(np.max(np.abs(inp["z"]))) * float(np.abs(M).sum(axis=1).max()))
    assert np.max(np.abs(a32 - a64)) <= scale
    # a transposed matrix is another sample
    aT = nr.sample_noise_f32(*(args[:7] + (M.T.copy(),) + args[8:]))[2]
    assert not np.array_equal(aT, a32)


def test_kept_rows_mean_row_and_shifts_are_copies():
    rs = np.random.RandomState(34)
    n, m, h, ad, Kk = 5, 3, 4, 2, 2
    D = h * ad
    inp = _inputs(rs, n, m, h, ad, Kk)
    M = rs.randn(h, h).astype(np.float32)
    shift = np.array([1, 0, -1], dtype=np.int32)
    kc = [2, 1, 2]
    mu, sd, a, seq = nr.sample_noise_f32(inp["mean"], inp["std"], inp["kept"], kc, shift, inp["z"], inp["sigma0"], M, inp["low"],
                                         inp["high"], n, m, h, ad, Kk, 1)
    lowD, highD = np.tile(inp["low"], h), np.tile(inp["high"], h)
    assert np.array_equal(_bits(mu[0]), _bits(ir.shift_rows(inp["mean"][0], True, h, ad)))
    assert np.array_equal(_bits(mu[1]), _bits(inp["mean"][1])) and np.all(mu[2] == 0)
    assert np.array_equal(_bits(sd[0]), _bits(np.tile(inp["sigma0"], h))) and np.array_equal(_bits(sd[1]), _bits(inp["std"][1]))
    assert np.array_equal(_bits(sd[2]), _bits(np.tile(inp["sigma0"], h)))
    for j in range(2):
        assert np.array_equal(_bits(a[j, 0]), _bits(ir.shift_rows(inp["kept"][0, j], True, h, ad)))
    assert np.array_equal(_bits(a[0, 1]), _bits(inp["kept"][1, 0]))
    assert not np.array_equal(a[1, 1], inp["kept"][1, 1])                # env 1 holds one kept row only
    assert not np.array_equal(a[0, 2], inp["kept"][2, 0])                # a fresh env places none
    for i in range(m):
        assert np.array_equal(_bits(a[n - 1, i]), _bits(np.minimum(np.maximum(mu[i], lowD), highD)))
    assert np.array_equal(_bits(seq), _bits(a.reshape(-1)[ir.seq_index(n, m, h, ad)]))
    # the same state through the AR(1) restatement: mean_out, std_out and the copied rows agree
    mu1, sd1, a1, _ = ir.sample_f32(inp["mean"], inp["std"], inp["kept"], kc, shift, inp["z"], inp["sigma0"], 0.5, inp["low"],
                                    inp["high"], n, m, h, ad, Kk, 1)
    assert np.array_equal(_bits(mu), _bits(mu1)) and np.array_equal(_bits(sd), _bits(sd1))
    assert np.array_equal(_bits(a[:2, 0]), _bits(a1[:2, 0])) and np.array_equal(_bits(a[n - 1]), _bits(a1[n - 1]))
