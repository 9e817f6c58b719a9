"""Pins ``tests/cem_reference.py`` - the float64 restatement the CEM kernels are judged by (``tests/test_cem_kernels_gpu.py``) -
against known answers and independent formulations, without a GPU."""

import numpy as np
import pytest

import cem_reference as cr
import cem_ties
from test_cem_refit_sample import _returns


# Random123's kat_vectors, philox4x32 with 10 rounds: (counter, key, output)
_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF),
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in _KAT:
        got = cr.philox4x32_10(ctr, key)
        assert [int(w[0]) for w in got] == list(want)
    # vectorised: the three vectors at once
    got = cr.philox4x32_10([np.array([v[0][w] for v in _KAT], dtype=np.uint64) for w in range(4)],
                           [np.array([v[1][w] for v in _KAT], dtype=np.uint64) for w in range(2)])
    assert np.array_equal(np.stack(got, axis=1), np.array([v[2] for v in _KAT], dtype=np.uint64))


def test_philox_normal_matches_the_scalar_restatement():
    from test_gpu_parity import _philox_normal_ref
    rs = np.random.RandomState(0)
    idx = [0, 1, 2, 63, 64, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 12345, 1 << 63, (1 << 64) - 1]
    idx += [int(x) for x in rs.randint(0, 1 << 31, 489)]
    idx += [(int(a) << 32) | int(b) for a, b in zip(rs.randint(1, 1 << 31, 500) * 2 + 1, rs.randint(0, 1 << 31, 500) * 2 + 1)]
    assert len(idx) == 1000 and sum(1 for x in idx if x >= 1 << 32) > 500
    for seed in (0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x1234567887654321):
        got = cr.philox_normal(seed, np.array(idx, dtype=np.uint64))
        want = np.array([_philox_normal_ref(seed, x) for x in idx])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    assert np.array_equal(cr.philox_indices((1 << 64) - 2, 4), np.array([(1 << 64) - 2, (1 << 64) - 1, 0, 1], dtype=np.uint64))
    u1, u2 = cr.philox_uniforms(7, cr.philox_indices(0, 4096))
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)


def test_reference_refit_matches_the_mask_formulation_on_tie_free_returns():
    rs = np.random.RandomState(1)
    for n, m, D, k, alpha in ((50, 1, 3, 5, 0.1), (333, 3, 20, 33, 0.1), (64, 2, 7, 64, 0.0), (17, 4, 2, 1, 1.0)):
        returns = rs.permutation(m * n).reshape(m, n).astype(np.float64) * 0.37 - 3.0
        a = rs.randn(n, m, D)
        mean = rs.randn(m, D)
        got_mean, got_std, _ = cr.refit(mean, a, returns, k, alpha, True)
        want_mean, want_std = cem_ties.reference_refit(mean, a, returns, k, np.float64(np.float32(alpha)))
        np.testing.assert_allclose(got_mean, want_mean, rtol=1e-12)
        np.testing.assert_allclose(got_std, np.broadcast_to(want_std, (m, D)), rtol=1e-12)


def test_fixed_refit_is_the_top_k_per_env():
    rs = np.random.RandomState(2)
    n, m, D, k = 40, 3, 4, 6
    returns = rs.permutation(m * n).reshape(m, n).astype(np.float64)
    a, mean = rs.randn(n, m, D), rs.randn(m, D)
    got_mean, got_std, rows = cr.refit(mean, a, returns, k, 0.25, False)
    for i in range(m):
        top = np.argsort(-returns[i])[:k]
        assert np.array_equal(rows[i], top * m + i)
        np.testing.assert_allclose(got_mean[i], mean[i] * 0.25 + 0.75 * a[top, i].mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(got_std[i], a[top, i].std(axis=0), rtol=1e-12)


def _sorts_before(r, c, j):
    """Does candidate c sort before candidate j (descending, NaN as -inf, ties to the lower index)?"""
    w = -np.inf if np.isnan(r[c]) else r[c]
    v = -np.inf if np.isnan(r[j]) else r[j]
    return w > v or (w == v and c < j)


@pytest.mark.parametrize("kind", ["mixed", "equal", "nan"])
def test_elite_rows_match_a_brute_force_count(kind):
    rs = np.random.RandomState(3)
    n, m = 41, 3
    returns = _returns(rs, m, n, kind)
    if kind == "mixed":
        returns[1, :7] = [np.inf, -np.inf, np.nan, np.inf, -np.inf, 0.0, -0.0]
    brute = np.array([[sum(_sorts_before(returns[i], c, j) for c in range(n)) for j in range(n)] for i in range(m)])
    order, ranks = cr.stable_rank(returns)
    assert np.array_equal(ranks, brute)
    for i in range(m):
        assert sorted(ranks[i]) == list(range(n)) and np.array_equal(ranks[i, order[i]], np.arange(n))
    for k in (1, 4, n):
        fixed = cr.elite_rows(returns, k, False)
        want = np.array([[j * m + i for p in range(k) for j in range(n) if brute[i, j] == p] for i in range(m)])
        assert np.array_equal(fixed, want)
        ref = cr.elite_rows(returns, k, True)
        assert np.array_equal(ref, np.array([[brute[i, j] * m + i for j in range(k)] for i in range(m)]))
        # the reference's own mask (:101) selects the same positions
        mask = (order < k).T
        for i in range(m):
            assert np.array_equal(np.sort(ref[i]), np.nonzero(mask[:, i])[0] * m + i)


@pytest.mark.parametrize("reference", [True, False])
def test_sample_matches_the_transposes(reference):
    rs = np.random.RandomState(4)
    n, m, h, ad = 13, 3, 5, 4
    D = h * ad
    z, mean, std = rs.randn(n, m, D), 0.3 * rs.randn(m, D), 0.5 + rs.rand(m, D)
    low, high = np.linspace(-0.8, -0.3, ad), np.linspace(0.4, 0.9, ad)
    a_want = mean[None] + z * std[None]
    c_want = np.clip(a_want, np.tile(low, h), np.tile(high, h))
    assert (c_want != a_want).any() and (c_want == a_want).any()
    if reference:       # the reference reads its candidate-major rows as [m, n, D] (:92-96), unclipped
        full = np.transpose(a_want.reshape(n * m, h, ad), (1, 0, 2)).reshape(h, m, n, ad)
    else:
        full = np.transpose(c_want.transpose(1, 0, 2).reshape(m * n, h, ad), (1, 0, 2)).reshape(h, m, n, ad)
    for lo, hi in ((0, n), (0, 1), (n - 1, n), (n // 3, 2 * n // 3), (n // 2, n // 2)):
        a_raw, a_clip, seq = cr.sample(mean, std, z, low, high, n, m, h, ad, reference, lo, hi)
        assert np.array_equal(a_raw, a_want) and np.array_equal(a_clip, c_want)
        assert seq.shape == (h, m * (hi - lo), ad)
        assert np.array_equal(seq, full[:, :, lo:hi, :].reshape(h, m * (hi - lo), ad))
    idx = cr.seq_index(n, m, h, ad, reference, 0, n)
    assert sorted(idx.reshape(-1)) == list(range(n * m * D))       # a permutation of the sample elements


def test_pick_is_numpy_argmax_in_both_readings():
    n, m, D, ad = 9, 2, 6, 3
    cand = np.arange(n * m * D, dtype=np.float32).reshape(n, m, D)
    returns = np.array([[1, 5, 5, 0, 2, 3, 4, 1, 5], [0, np.nan, 9, np.nan, 1, 2, 3, 4, 5]], dtype=np.float32)
    idx, ret, act = cr.pick(returns, cand, n, m, D, ad, True)
    assert list(idx) == [1, 1] and ret[0] == 5 and np.isnan(ret[1])
    assert np.array_equal(act, cand.reshape(m, n, D)[[0, 1], [1, 1], :ad])
    idx, ret, act = cr.pick(returns, cand, n, m, D, ad, False)
    assert np.array_equal(act, cand[[1, 1], [0, 1], :ad])
    idx, _, _ = cr.pick(np.full((m, n), -np.inf), cand, n, m, D, ad, False)
    assert list(idx) == [0, 0]


def test_stats_bounds_are_the_derived_ones():
    a, mean = np.array([0.5, -2.0]), np.array([1.0])
    mb, sb = cr.stats_bounds(1, a, mean)
    assert mb == 17 * 2.0 ** -24 * 2.0 and sb == 2 * mb
    assert cr.stats_bounds(33, a, mean)[0] == 18 * 2.0 ** -24 * 2.0
    assert cr.stats_bounds(8192, a, mean * 4)[0] == (256 + 16) * 2.0 ** -24 * 4.0
