"""Self-checks of the diverged-rollout fixtures (nonfinite_cases.py), CPU only: every fixture gives its intended class
pattern in the oracle, in fp32 and in float64 end to end, and its finite candidates stay far below the fp32 range - so the
GPU comparisons in test_gpu_nonfinite.py test the kernels, not the rounding of a borderline candidate."""

import numpy as np
import pytest

import nonfinite_cases as nc


@pytest.mark.parametrize("kind,kw", nc.MLP_CASES, ids=[nc.case_id(k, kw) for k, kw in nc.MLP_CASES])
def test_fixture_classes_and_margins(kind, kw):
    case = nc.mlp_case(kind, **kw)
    pat = case["pattern"]
    states = []
    ret = nc.oracle_returns(case, track=states)
    np.testing.assert_array_equal(nc.classify(ret), pat)
    np.testing.assert_array_equal(nc.classify(nc.oracle_returns(case, mlp_dtype=np.float64)), pat)
    fin = pat == nc.FINITE
    assert fin.sum() > case["n"] // 2
    for s in states:
        assert np.all(np.abs(s.reshape(case["m"], case["n"], -1)[fin]) <= nc.MARGIN)
    assert np.all(np.abs(ret[fin]) <= nc.MARGIN)
    want = {"mixed": nc.NAN, "inf": nc.POS_INF, "hidden_nan": nc.NAN, "out_nan": nc.NAN, "onesign": nc.POS_INF,
            "vel": nc.NAN}[kind]
    for i in range(case["m"]):
        best = int(np.argmax(ret[i]))
        assert pat[i, best] == want and best == int(np.argmax(pat[i] == want))
        if want == nc.NAN:
            assert best >= 16          # the first NaN is past the first 16-candidate tile
    if kind == "mixed":
        assert set(np.unique(pat)) == {nc.FINITE, nc.POS_INF, nc.NEG_INF, nc.NAN}
    if kind == "inf":
        assert set(np.unique(pat)) == {nc.FINITE, nc.POS_INF, nc.NEG_INF}
    if kind == "onesign":
        assert case["obs_dim"] % 16 != 0 and set(np.unique(pat)) == {nc.FINITE, nc.POS_INF}
    if kind == "vel":
        assert case["spec"].w_vel != 0.0 and case["h"] >= 2 and set(np.unique(pat)) == {nc.FINITE, nc.NAN}


def test_classify():
    x = np.array([0.0, -0.0, 1e38, np.inf, -np.inf, np.nan, -1.0])
    np.testing.assert_array_equal(nc.classify(x), [0, 0, 0, 1, 2, 3, 0])


@pytest.mark.parametrize("cell,sizes,act", nc.RNN_CASES)
def test_rnn_fixture_classes(cell, sizes, act):
    case = nc.rnn_case(cell, sizes, act)
    np.testing.assert_array_equal(nc.classify(nc.rnn_oracle_returns(case)), case["pattern"])
    np.testing.assert_array_equal(nc.classify(nc.rnn_oracle_returns(case, np.float64)), case["pattern"])
    ret = nc.rnn_oracle_returns(case)
    assert np.all(np.abs(ret[case["pattern"] == nc.FINITE]) <= nc.MARGIN)
