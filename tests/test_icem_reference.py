"""``tests/icem_reference.py`` against known answers and independent formulations (CPU only): the white-noise case against
``cem_reference``, the recurrence's closed form and its unit variance, shift / kept rows / mean row, elite selection against a
stable argsort, the population formula at its edges, the refit on a hand-computed case and the bound's ingredients."""

import numpy as np
import pytest

import cem_reference as cr
import icem_reference as ir

WIDE = 1e9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- white noise
def test_rho_zero_without_kept_rows_is_cem_fixed_mode_sample_bit_for_bit():
    """``rho = 0``, ``kc = 0``, ``shift = 0``, ``add_mean = 0``: the fp32 sample equals ``cem_reference.sample(reference=False)``
    bit for bit.  The inputs are dyadic (odd multiples of 1/8 times powers of two plus multiples of 1/16), so the float64
    arithmetic of ``cem_reference`` is exact and its result is an fp32 number: equal bits, no tolerance."""
    rs = np.random.RandomState(3)
    n, m, h, ad = 11, 3, 4, 5
    D = h * ad
    z = ((2 * rs.randint(-20, 20, size=(n, m, D)) + 1) / 8.0).astype(np.float32)
    std = (2.0 ** rs.randint(-3, 2, size=(m, D))).astype(np.float32)
    mean = (rs.randint(-16, 16, size=(m, D)) / 16.0).astype(np.float32)
    low, high = np.linspace(-1.5, -0.5, ad).astype(np.float32), np.linspace(0.5, 1.25, ad).astype(np.float32)
    _, want_a, want_seq = cr.sample(mean, std, z, low, high, n, m, h, ad, False, 0, n)
    shift = np.zeros(m, dtype=np.int32)
    for Kk, kept, kc in ((0, None, None), (2, np.full((m, 2, D), 7.0, dtype=np.float32), np.zeros(m, dtype=np.int32))):
        mu, sd, a, seq = ir.sample_f32(mean, std, kept, kc, shift, z, np.ones(ad, dtype=np.float32), 0.0, low, high, n, m, h, ad, Kk, 0)
        assert a.dtype == np.float32
        assert np.array_equal(_bits(a), _bits(want_a)) and np.array_equal(a.astype(np.float64), want_a)
        assert np.array_equal(_bits(seq), _bits(want_seq))
        assert np.array_equal(_bits(mu), _bits(mean)) and np.array_equal(_bits(sd), _bits(std))
    assert (want_a == np.tile(low, h)).any() and (want_a == np.tile(high, h)).any()


# -------------------------------------------------------------------------------------------------------------------- recurrence
@pytest.mark.parametrize("rho", [0.0, 0.5, 0.96875])
def test_recurrence_matches_its_closed_form_and_has_unit_variance(rho):
    rs = np.random.RandomState(4)
    n, m, h, ad = 5, 2, 9, 3
    z = rs.randn(n, m, h, ad)
    C = ir.recurrence_coefficients(rho, h)
    want = np.einsum("ts,nmsa->nmta", C, z)
    np.testing.assert_allclose(ir.recurrence(z, rho), want, rtol=1e-12, atol=1e-13)
    # unit variance analytically: independent unit normals, so Var nz_t = sum_s C[t, s]^2
    np.testing.assert_allclose((C * C).sum(axis=1), np.ones(h), rtol=0, atol=4e-16 * h)
    assert np.all(np.triu(C, 1) == 0)
    # the sample restatement (fp32 constants, float64 arithmetic) is that recurrence scaled by sd' around mu'
    z32 = z.astype(np.float32)
    mean = rs.randn(m, h * ad).astype(np.float32)
    std = (0.1 + rs.rand(m, h * ad)).astype(np.float32)
    big = np.full(ad, WIDE, dtype=np.float32)
    _, _, a, _ = ir.sample(mean, std, None, None, np.zeros(m, dtype=np.int32), z32, np.ones(ad), rho, -big, big, n, m, h, ad, 0, 0)
    want_a = mean.astype(np.float64)[None] + ir.recurrence(z32.astype(np.float64), rho).reshape(n, m, -1) * std.astype(np.float64)[None]
    np.testing.assert_allclose(a, want_a, rtol=1e-6, atol=1e-6)
    a32 = ir.sample_f32(mean, std, None, None, np.zeros(m, dtype=np.int32), z32, np.ones(ad), rho, -big, big, n, m, h, ad, 0, 0)[2]
    assert a32.dtype == np.float32
    # fp32 against float64: each step adds at most 4 roundings on magnitudes bounded by |mu| + |nz| sd
    scale = np.abs(mean).max() + np.abs(ir.recurrence(z32, rho)).max() * std.max()
    assert np.max(np.abs(a32 - a)) <= 4 * h * 2.0 ** -24 * scale


def test_noise_constants_are_fp32_and_exact_where_they_can_be():
    r, c = ir.noise_constants(0.0)
    assert r == 0 and c == 1 and c.dtype == np.float32
    r, c = ir.noise_constants(0.6)
    assert r == np.float32(0.6) and abs(float(c) - 0.8) < 2.0 ** -23
    assert ir.noise_constants(0.5)[1] == np.float32(np.sqrt(np.float32(0.75)))


# ------------------------------------------------------------------------------------------------- shift, kept rows, mean row
def test_shift_kept_rows_and_mean_row():
    rs = np.random.RandomState(5)
    n, m, h, ad, Kk = 4, 3, 3, 2, 2
    D = h * ad
    mean = rs.randn(m, D).astype(np.float32)
    std = (0.5 + rs.rand(m, D)).astype(np.float32)
    kept = (0.1 * rs.randn(m, Kk, D)).astype(np.float32)
    kc = np.array([2, 2, 1], dtype=np.int32)
    sigma0 = np.array([0.25, 0.5], dtype=np.float32)
    z = rs.randn(n, m, D).astype(np.float32)
    low, high = np.full(ad, -0.3, dtype=np.float32), np.full(ad, 0.3, dtype=np.float32)
    shift = np.array([-1, 1, 0], dtype=np.int32)
    mu, sd, a, seq = ir.sample_f32(mean, std, kept, kc, shift, z, sigma0, 0.5, low, high, n, m, h, ad, Kk, 1)
    moved = lambda x: np.concatenate([x[ad:], x[-ad:]])      # noqa: E731
    assert np.all(mu[0] == 0) and np.array_equal(mu[1], moved(mean[1])) and np.array_equal(mu[2], mean[2])
    assert np.array_equal(sd[0], np.tile(sigma0, h)) and np.array_equal(sd[1], np.tile(sigma0, h)) and np.array_equal(sd[2], std[2])
    # env 0 is fresh: no kept row; env 1: two kept rows, shifted; env 2: one kept row, as stored
    assert np.array_equal(a[0, 1], moved(kept[1, 0])) and np.array_equal(a[1, 1], moved(kept[1, 1]))
    assert np.array_equal(a[0, 2], kept[2, 0])
    first = np.clip(mu[2, :ad] + z[1, 2, :ad] * sd[2, :ad], low, high)
    assert np.array_equal(a[1, 2, :ad], first) and np.array_equal(a[0, 0, :ad], np.clip(z[0, 0, :ad] * sigma0, low, high))
    for i in range(m):
        assert np.array_equal(a[n - 1, i], np.clip(mu[i], np.tile(low, h), np.tile(high, h)))
    assert np.array_equal(seq, a.reshape(-1)[ir.seq_index(n, m, h, ad)])
    # the mean row wins over a kept row: n = 1, kc = 1
    a1 = ir.sample_f32(mean, std, kept, kc, np.zeros(m, dtype=np.int32), z[:1], sigma0, 0.5, low, high, 1, m, h, ad, Kk, 1)[2]
    assert np.array_equal(a1[0], np.clip(mean, np.tile(low, h), np.tile(high, h)))
    a0 = ir.sample_f32(mean, std, kept, kc, np.zeros(m, dtype=np.int32), z[:1], sigma0, 0.5, low, high, 1, m, h, ad, Kk, 0)[2]
    assert np.array_equal(a0[0], kept[:, 0])
    # a count beyond Kk is held to Kk, one beyond n fills every row
    a2 = ir.sample_f32(mean, std, kept, np.array([9, 9, 9]), np.zeros(m, dtype=np.int32), z[:1], sigma0, 0.5, low, high, 1, m, h, ad, Kk, 0)[2]
    assert np.array_equal(a2, a0)


# ---------------------------------------------------------------------------------------------------------------------- elites
@pytest.mark.parametrize("K", [1, 2, 5, 40])
def test_elites_are_the_stable_argsort_restricted_to_the_valid_candidates(K):
    rs = np.random.RandomState(6)
    n = 37
    rows = [rs.randn(n), rs.choice([-1.5, 0.25, 7.0], size=n), np.full(n, 1.5), np.full(n, np.nan), np.full(n, -np.inf),
            np.full(n, np.inf), rs.choice([np.inf, -np.inf], size=n), np.where(np.arange(n) % 2 == 0, 0.0, -0.0)]
    mixed = rs.randn(n)
    mixed[::5], mixed[1::7], mixed[2::11] = np.nan, -np.inf, np.inf
    one = np.full(n, np.nan)
    one[12] = 0.75
    r = np.array(rows + [mixed, one], dtype=np.float32)
    el, valid = ir.elites(r, K)
    for i in range(len(r)):
        ok = ~np.isnan(r[i]) & (r[i] != -np.inf)
        order = np.argsort(-r[i].astype(np.float64), kind="stable")
        order = order[ok[order]]
        assert valid[i] == ok.sum()
        assert np.array_equal(el[i], order[:min(K, ok.sum())])


def test_population_formula_at_its_edges():
    assert ir.sizes(100, 0.1, 0.3, 1.25, 4) == (10, 3, [100, 80, 64, 51])
    assert ir.sizes(100, 0.1, 0.3, 1.0, 3) == (10, 3, [100, 100, 100])                  # decay = 1: no shrinking
    assert ir.sizes(10, 0.6, 0.5, 2.0, 3) == (6, 3, [10, 10, 10])                       # 2 K > n: n caps the floor
    assert ir.sizes(96, 0.1, 0.3, 4.0, 3) == (9, 2, [96, 24, 18])                       # the floor 2 K
    assert ir.sizes(5, 0.1, 0.3, 1.25, 2) == (1, 0, [5, 4])                             # K at least 1, Kk may be 0
    assert ir.population(1000, 100, 1.25, 40) == 200


# ----------------------------------------------------------------------------------------------------------------------- refit
def test_refit_on_a_hand_computed_case():
    low, high = np.array([-1.0], dtype=np.float32), np.array([1.0], dtype=np.float32)
    a = np.array([[[0.5, 0.0]], [[-0.5, 1.0]], [[0.25, 0.5]], [[0.75, -1.0]]], dtype=np.float32)     # [n = 4, m = 1, D = 2]
    r = np.array([[1.0, np.nan, 3.0, 1.0]], dtype=np.float32)
    mean, std = np.array([[2.0, 4.0]], dtype=np.float32), np.array([[1.0, 1.0]], dtype=np.float32)
    out = ir.refit(mean, std, a, r, 2, 1, 0.5, low, high, 1)
    assert [list(e) for e in out["elites"]] == [[2, 0]] and out["valid"][0] == 3 and out["Ke"][0] == 2
    np.testing.assert_allclose(out["mean"], [[0.5 * 2.0 + 0.5 * 0.375, 0.5 * 4.0 + 0.5 * 0.25]])
    np.testing.assert_allclose(out["std"], [[0.5 + 0.5 * 0.125, 0.5 + 0.5 * 0.25]])
    assert out["kc"][0] == 1 and np.array_equal(out["kept"][0], a[2:3, 0])
    assert out["index"][0] == 2 and out["best_return"][0] == 3.0 and out["action"][0, 0] == 0.25
    none = ir.refit(mean, std, a, np.full((1, 4), np.nan), 2, 1, 0.5, low, high, 1)
    assert np.array_equal(none["mean"], mean) and np.array_equal(none["std"], std) and none["kc"][0] == 0
    assert none["index"][0] == -1 and np.isnan(none["best_return"][0]) and none["action"][0, 0] == 1.0 and none["Ke"][0] == 0


def test_bound_ingredients():
    assert [ir.sum_chain(k) for k in (1, 128, 129, 8192)] == [35, 35, 36, 98]
    mb, sb = ir.refit_bounds(100, 2.0)
    assert mb == (ir.sum_chain(100) + 8) * 2.0 ** -24 * 2.0 and sb == 2 * mb
    assert ir.REFIT_STATIC_LDS == 32 * 33 * 4 + 16 * 4
