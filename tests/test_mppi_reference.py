"""``tests/mppi_reference.py`` against known answers and independent formulations (CPU only): the filter's closed form, the shift,
the weights in every non-finite case, the effective sample size, the rollout tensor's permutation and the bound's ingredients."""

import inspect

import numpy as np
import pytest

import mppi_reference as mr

WIDE = 1e9


def _case(rs, n, m, h, ad):
    D = h * ad
    return dict(mean=(0.3 * rs.randn(m, D)).astype(np.float32), z=rs.randn(n, m, D).astype(np.float32),
                sigma=(0.1 + rs.rand(ad)).astype(np.float32), low=np.full(ad, -WIDE, dtype=np.float32),
                high=np.full(ad, WIDE, dtype=np.float32))


# ----------------------------------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("beta", [1.0, 0.6, 2.0 ** -10])
def test_filter_matches_its_closed_form(beta):
    rs = np.random.RandomState(1)
    n, m, h, ad = 5, 2, 7, 3
    c = _case(rs, n, m, h, ad)
    _, a, _ = mr.sample(np.zeros((m, h * ad)), np.zeros(m, dtype=np.int32), c["z"], c["sigma"], beta, c["low"], c["high"], n, m, h, ad)
    u = c["z"].astype(np.float64).reshape(n, m, h, ad) * c["sigma"].astype(np.float64)
    want = mr.filter_closed_form(u, float(np.float32(beta)))
    np.testing.assert_allclose(a.reshape(n, m, h, ad), want, rtol=1e-6, atol=1e-12)
    if beta == 1.0:
        assert np.array_equal(a.reshape(n, m, h, ad), u)            # beta = 1 reproduces u exactly


def test_f32_restatement_follows_the_float64_one_and_rounds_every_operation():
    rs = np.random.RandomState(2)
    n, m, h, ad = 9, 3, 5, 4
    c = _case(rs, n, m, h, ad)
    shift = np.array([1, 0, -1], dtype=np.int32)
    low, high = np.full(ad, -0.4, dtype=np.float32), np.full(ad, 0.5, dtype=np.float32)
    m32, a32, s32 = mr.sample_f32(c["mean"], shift, c["z"], c["sigma"], 0.6, low, high, n, m, h, ad)
    m64, a64, s64 = mr.sample(c["mean"], shift, c["z"], c["sigma"], 0.6, low, high, n, m, h, ad)
    assert m32.dtype == a32.dtype == s32.dtype == np.float32 and a64.dtype == np.float64
    assert np.array_equal(m32.astype(np.float64), m64)              # the shift moves values, it computes nothing
    assert np.max(np.abs(a32 - a64)) < 1e-5 and np.max(np.abs(a32 - a64)) > 0
    assert (a32 == low[0]).any() and (a32 == high[0]).any() and a32.min() >= low[0] and a32.max() <= high[0]
    # one step by hand, scalar np.float32 arithmetic
    z0, z1 = c["z"][4, 1, 2], c["z"][4, 1, ad + 2]
    sg, be = c["sigma"][2], np.float32(0.6)
    n0 = be * (z0 * sg) + (np.float32(1) - be) * np.float32(0)
    n1 = be * (z1 * sg) + (np.float32(1) - be) * n0
    want = np.minimum(np.maximum(c["mean"][1, ad + 2] + n1, low[2]), high[2])
    assert a32[4, 1, ad + 2] == want


# ------------------------------------------------------------------------------------------------------------------------ shift
def test_shift_clamps_zeroes_and_keeps():
    h, ad = 4, 2
    mean = np.arange(3 * h * ad, dtype=np.float32).reshape(3, h * ad) + 1
    out = mr.shift_mean(mean, [1, -1, 0], h, ad).reshape(3, h, ad)
    src = mean.reshape(3, h, ad)
    assert np.array_equal(out[0, :h - 1], src[0, 1:]) and np.array_equal(out[0, h - 1], src[0, h - 1])     # clamps at h - 1
    assert np.all(out[1] == 0)
    assert np.array_equal(out[2], src[2])
    one = mr.shift_mean(mean[:, :ad], [1, 1, 1], 1, ad)             # h = 1: the shift is the identity
    assert np.array_equal(one, mean[:, :ad])


# ---------------------------------------------------------------------------------------------------------------------- weights
def test_weights_are_non_negative_and_sum_to_at_least_one():
    rs = np.random.RandomState(3)
    r = (rs.randn(4, 50) * 10).astype(np.float32)
    r[1, 7] = np.nan
    r[2, :] = -np.inf
    for kappa in (2.0 ** -10, 1.0, 1e3):
        w, rmax, index, valid = mr.weights(r, kappa)
        assert np.all(w >= 0) and np.all(w <= 1)
        assert np.all(w.sum(axis=1)[valid > 0] >= 1.0)
        assert w[1, 7] == 0 and np.all(w[2] == 0) and valid[2] == 0 and index[2] == -1 and np.isnan(rmax[2])
        assert valid[1] == 49 and valid[0] == 50
        for i in (0, 1, 3):
            assert w[i, index[i]] == 1.0 and rmax[i] == np.nanmax(r[i])


def test_large_kappa_concentrates_on_the_arg_max_and_tiny_kappa_is_the_plain_mean():
    rs = np.random.RandomState(4)
    n, m, D = 30, 2, 6
    a = rs.uniform(-1, 1, size=(n, m, D)).astype(np.float32)
    r = np.stack([rs.permutation(n) * 1.0 for _ in range(m)]).astype(np.float32)        # separated by 1
    mean0 = np.zeros((m, D))
    new = mr.update(mean0, a, r, 1e3)[0]
    best = np.argmax(r, axis=1)
    np.testing.assert_allclose(new, a[best, np.arange(m)].astype(np.float64), atol=1e-300)
    new = mr.update(mean0, a, r, 1e-9)[0]
    np.testing.assert_allclose(new, a.astype(np.float64).mean(axis=0), atol=1e-7)


def test_every_non_finite_case():
    inf, nan = np.inf, np.nan
    # NaN and -inf weigh 0; the maximum is taken over the valid ones
    w, rmax, index, valid = mr.weights(np.float32([[nan, 1.0, -inf, 2.0, nan]]), 1.0)
    np.testing.assert_allclose(w[0], [0, np.exp(-1.0), 0, 1.0, 0])
    assert rmax[0] == 2.0 and index[0] == 3 and valid[0] == 2
    # Rmax = +inf: 1 for the +inf returns, 0 otherwise (no inf - inf)
    w, rmax, index, valid = mr.weights(np.float32([[1.0, inf, -inf, inf, nan, 5.0]]), 2.0)
    assert np.array_equal(w[0], [0, 1, 0, 1, 0, 0]) and rmax[0] == inf and index[0] == 1 and valid[0] == 4
    # all invalid: degenerate
    for row in ([nan, nan], [-inf, -inf], [nan, -inf]):
        w, rmax, index, valid = mr.weights(np.float32([row]), 1.0)
        assert np.all(w == 0) and np.isnan(rmax[0]) and index[0] == -1 and valid[0] == 0
    # a difference that overflows fp32 gives 0, whatever kappa
    w, rmax, index, valid = mr.weights(np.float32([[3e38, -3e38, 3e38]]), 2.0 ** -100)
    assert np.array_equal(w[0], [1, 0, 1]) and index[0] == 0 and valid[0] == 3
    # ties: the first maximum; -0.0 and +0.0 tie
    w, rmax, index, valid = mr.weights(np.float32([[-0.0, 0.0, -1.0]]), 1.0)
    assert index[0] == 0 and np.signbit(rmax[0]) and w[0, 0] == w[0, 1] == 1.0
    # a degenerate env keeps its mean; the others move
    a = np.ones((2, 2, 3), dtype=np.float32)
    mean0 = np.full((2, 3), 7.0)
    res = mr.result_row(mean0, a, np.float32([[nan, -inf], [0.0, nan]]), 1.0, 3)
    assert np.all(res["mean"][0] == 7.0) and np.all(res["mean"][1] == 1.0)
    assert res["ess"][0] == 0 and res["ess"][1] == 1 and list(res["valid"]) == [0, 1] and list(res["index"]) == [-1, 0]
    assert np.isnan(res["rmax"][0]) and res["rmax"][1] == 0.0 and np.all(res["action"][0] == 7.0)


def test_effective_sample_size():
    n = 17
    a = np.zeros((n, 1, 2), dtype=np.float32)
    r = np.full((1, n), 1.5, dtype=np.float32)
    r[0, 3] = np.nan
    assert mr.update(np.zeros((1, 2)), a, r, 1.0)[5][0] == pytest.approx(n - 1)       # equal returns: the number of valid candidates
    r = np.zeros((1, n), dtype=np.float32)
    r[0, 5] = 1000.0
    assert mr.update(np.zeros((1, 2)), a, r, 1.0)[5][0] == pytest.approx(1.0)         # a single dominant one


# -------------------------------------------------------------------------------------------------------------------------- seq
def test_seq_is_the_stated_permutation_of_a_clip():
    rs = np.random.RandomState(5)
    n, m, h, ad = 4, 3, 5, 2
    c = _case(rs, n, m, h, ad)
    _, a, seq = mr.sample_f32(c["mean"], np.zeros(m, dtype=np.int32), c["z"], c["sigma"], 0.6, c["low"], c["high"], n, m, h, ad)
    assert seq.shape == (h, m * n, ad)
    a5 = a.reshape(n, m, h, ad)
    for j in range(n):
        for i in range(m):
            for t in range(h):
                assert np.array_equal(seq[t, i * n + j], a5[j, i, t])
    idx = mr.seq_index(n, m, h, ad)
    assert sorted(idx.reshape(-1)) == list(range(n * m * h * ad))


# ----------------------------------------------------------------------------------------------------------------------- bounds
def test_bound_ingredients():
    assert mr.sum_chain(1) == 38 and mr.sum_chain(128) == 38 and mr.sum_chain(129) == 39 and mr.sum_chain(4097) == 33 + 37
    b, rel = mr.update_bounds(64, 1.0, 2.0)
    gamma_s = (mr.sum_chain(64) + 16) * 2.0 ** -24
    gamma_w = 106 * 2.0 ** -24
    assert rel == 2 * gamma_w + 2 * gamma_s and b == rel * 2.0
    assert mr.update_bounds(64, 1e3, 2.0) == (b, rel)
    assert mr.update_bounds(64, 1.0, 2.0, L=100)[1] == 2 * gamma_w + 2 * 116 * 2.0 ** -24
    assert "L" in inspect.signature(mr.update_bounds).parameters


def test_philox_stream_is_cems():
    import cem_reference as cr
    assert mr.philox_normal is cr.philox_normal and mr.philox_indices is cr.philox_indices
