"""The env-layout table of ``tests/env_layout_cases.py`` judged on the CPU, before ``tests/test_env_layout_gpu.py`` runs it on
the kernels: the vectorised ``key_pack`` is the library's host ``l2a_key_encode``; the restatements of the two per-env key
reductions equal the plain arg-max on every ``(W, n, tail)``; each one-line mutant is rejected by the table; the mutants that touch
wave 1 only (V1, V3, S2) are rejected by NO layout below 128 rows per workgroup, and V1 / V3 by none of the shapes the suite had
before at the 16 rows per workgroup those shapes ran with - the gap this table closes; and the table's structural claims hold at
32, 64, 256 and 304 compute units."""

import ctypes
import functools

import numpy as np
import pytest

import env_layout_cases as elc
from learning_to_adapt_amd import _lib

WN = [(W, n) for W in elc.WS for n in elc.N_LAYOUT]
WN_IDS = ["W%d_n%d" % wn for wn in WN]


def _encode(ret, index):
    return int(_lib.load().l2a_key_encode(ctypes.c_float(ret), int(index)))


# ------------------------------------------------------------------------------------------
# 1. key_pack
# ------------------------------------------------------------------------------------------
def test_key_pack_is_the_librarys_key_encode():
    f32 = np.float32
    tiny, big = np.finfo(f32).tiny, np.finfo(f32).max
    denormal = np.array([1, 0x007FFFFF, 0x80000001, 0x807FFFFF], dtype=np.uint32).view(f32)
    values = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, big, -big, tiny, -tiny, 1.0, -1.0], dtype=f32),
                             denormal])
    rs = np.random.RandomState(1)
    words = rs.randint(0, 2 ** 32, size=4000, dtype=np.uint64).astype(np.uint32).view(f32)
    widx = rs.randint(0, 2 ** 31, size=4000, dtype=np.int64)
    vals = np.concatenate([np.repeat(values, 4), words])
    idx = np.concatenate([np.tile(np.array([0, 1, 1000, 2 ** 31 - 1], dtype=np.int64), len(values)), widx])
    got = elc.key_pack(vals, idx)
    assert got.dtype == np.uint64 and got.shape == vals.shape
    for v, i, k in zip(vals, idx, got):
        assert int(k) == _encode(v, i), (v, i)
    # the order the kernels rely on
    k = lambda v, i=0: int(elc.key_pack(f32(v), i))                         # noqa: E731
    assert k(-np.inf) < k(-big) < k(-1.0) < k(-tiny) < k(denormal[2]) < k(0.0) < k(denormal[0]) < k(tiny) < k(big) < k(np.inf) < k(np.nan)
    assert k(0.0) == k(-0.0) and k(1.0, 5) > k(1.0, 6) and k(-np.inf, 2 ** 31 - 1) > 0
    assert k(-np.inf) == (0x007FFFFF << 31) | 0x7FFFFFFF


def test_want_keys_is_the_ctypes_arg_max_of_the_older_tests():
    rs = np.random.RandomState(2)
    r = rs.randn(40, 7).astype(np.float32)
    r[3, 2] = r[3, 5] = 9.0
    r[4] = -np.inf
    r[5, 4] = np.nan
    r[6] = np.nan
    r[7, 1], r[7, 3] = 0.0, -0.0
    r[7, [0, 2, 4, 5, 6]] = -1.0
    for off in (0, 1000, 2 ** 31 - 1 - 7):
        want = [_encode(row[int(np.argmax(row))], off + int(np.argmax(row))) for row in r]
        assert [int(x) for x in elc.want_keys(r, off)] == want
        assert np.array_equal(elc.row_keys(r, off).reshape(40, 7).max(axis=1), elc.want_keys(r, off))


# ------------------------------------------------------------------------------------------
# 2. the layouts
# ------------------------------------------------------------------------------------------
def test_layout_gives_the_class_it_is_asked_for_or_says_it_cannot():
    """Which classes each n covers, written out: W is a power of two, so ``rows mod W`` walks the multiples of gcd(n, W)."""
    impossible = {(W, n, tail) for W in elc.WS for n in elc.N_LAYOUT for tail in elc.TAILS if elc.layout(W, n, 100, tail) is None}
    want = set()
    for W in elc.WS:
        want |= {(W, n, elc.ONE) for n in (2, 16, 32, 64)}                                  # an even n never leaves one row
        want |= {(W, n, elc.SHORT) for n in (16, 32, 64) if n % min(W, 64) == 0}            # W | n: whole workgroups only (at 128: 0 or 64 rows)
        want |= {(W, n, elc.LONG) for n in elc.N_LAYOUT if W != 128 or n == 64}             # wave 1 exists at W = 128 alone
        want |= {(W, n, elc.CUT) for n in (1, 2, 16, 32, 64) if W % n == 0 or n % W == 0}   # n | W: no env crosses a workgroup boundary; W | n: whole workgroups
    assert impossible == want
    for W, n in WN:
        got = elc.layouts(W, n, elc.min_rows_small(W))
        plain = (W, n) in ((16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64), (128, 64))
        assert ([t for t, _, _ in got] == [elc.PLAIN]) == plain, (W, n)
        for tail, m, rows in got:
            assert rows == m * n and elc.min_rows_small(W) <= rows < elc.min_rows_small(W) + W * n
            assert tail == elc.PLAIN or elc.tail_ok(W, n, rows % W, tail)
    # the (W, n) without a class stay in the table: whole workgroups where W | n, a wave-0-only last workgroup at (128, 64)
    assert elc.layouts(128, 64, 421) == [(elc.PLAIN, 7, 448)] and elc.layouts(64, 64, 229) == [(elc.PLAIN, 4, 256)]
    assert [t for t, _, _ in elc.layouts(128, 16, 421)] == [elc.SHORT, elc.LONG] and elc.layout(128, 32, 421, elc.LONG) == (15, 480)


@functools.lru_cache(maxsize=None)
def _case(W, n, tail, m, seed=0):
    """Returns with the planted patterns, their keys at a cand_offset that cycles with the layout, and the wanted keys."""
    off = elc.cand_offset_of(elc.CAND_OFFSETS[(elc.N_LAYOUT.index(n) + elc.WS.index(W) + (elc.TAILS + (elc.PLAIN,)).index(tail)) % 3], n)
    returns = elc.base_returns(seed + 7 * n + W, m, n)
    planted = elc.plant(returns, W)
    return returns, planted, off, elc.row_keys(returns, off), elc.want_keys(returns, off)


def _all_layouts(W, n):
    return elc.layouts(W, n, elc.min_rows_small(W))


@pytest.mark.parametrize("W,n", WN, ids=WN_IDS)
def test_restatements_equal_the_arg_max_and_mutants_show_where_they_can(W, n):
    for tail, m, rows in _all_layouts(W, n):
        returns, planted, off, keys, want = _case(W, n, tail, m)
        assert np.array_equal(elc.value_reduce(keys, n, W), want), (tail, "value")
        assert np.array_equal(elc.scorer_reduce(keys, n, W), want), (tail, "scorer")
        elc.check_plants(returns, want, planted, off)
        if W < 128:         # the gap: below 128 rows per workgroup nothing sits in wave 1 - these three ARE the kernel
            for mutant in ("V1", "V3"):
                assert np.array_equal(elc.value_reduce(keys, n, W, mutant), want), (tail, mutant)
            assert np.array_equal(elc.scorer_reduce(keys, n, W, "S2"), want), (tail, "S2")
        assert np.array_equal(elc.gather_env(rows, n), np.repeat(np.arange(m), n))


def _rejecting(mutant, W):
    """The (n, tail) of the table at W whose planted returns tell ``mutant`` from the kernel."""
    out = []
    for n in elc.N_LAYOUT:
        for tail, m, rows in _all_layouts(W, n):
            returns, planted, off, keys, want = _case(W, n, tail, m)
            if mutant == "G":
                differs = not np.array_equal(elc.gather_env(rows, n, "G"), elc.gather_env(rows, n))
            elif mutant in elc.VALUE_MUTANTS:
                differs = not np.array_equal(elc.value_reduce(keys, n, W, mutant), want)
            else:
                differs = not np.array_equal(elc.scorer_reduce(keys, n, W, mutant), want)
            if differs:
                out.append((n, tail))
    return out


def test_every_mutant_is_rejected_and_wave_1_mutants_only_at_128_rows():
    total = {W: sum(len(_all_layouts(W, n)) for n in elc.N_LAYOUT) for W in elc.WS}
    for mutant in ("V1", "V3", "S2"):
        for W in (16, 32, 64):
            assert _rejecting(mutant, W) == [], (mutant, W)
        hit = _rejecting(mutant, 128)
        print("%s: rejected by %d of %d layouts at W = 128: n in %s" % (mutant, len(hit), total[128], sorted({n for n, _ in hit})))
        # V1, V3: every n has an env whose winner can sit in wave 1.  S2: an env run crosses rows 63 | 64 unless n divides 64
        assert {n for n, _ in hit} == {n for n in elc.N_LAYOUT if mutant != "S2" or 64 % n}, mutant
    for mutant in ("V2", "S1", "G"):
        for W in elc.WS:
            hit = _rejecting(mutant, W)
            print("%s: rejected by %d of %d layouts at W = %d" % (mutant, len(hit), total[W], W))
            ns = {n for n, _ in hit}
            if mutant == "V2":      # a wave's rows (the workgroup's below 64) touch a second env unless they are whole envs' rows
                assert ns == {n for n in elc.N_LAYOUT if n % min(W, 64)}, (W, ns)
            elif mutant == "S1":    # an env starts off a multiple of 16 unless 16 | n
                assert ns == {n for n in elc.N_LAYOUT if n % 16}, (W, ns)
            else:                   # a 16-row tile holds two envs unless 16 | n
                assert ns == {n for n in elc.N_LAYOUT if n % 16}, (W, ns)


def test_the_shapes_the_suite_had_before_do_not_see_wave_1():
    """``l2a_value_terminal`` ran at m * n <= 260 rows only: RT = 1 on any device of 17 CUs or more, 16 rows per workgroup."""
    for m, n in elc.OLD_VALUE_SHAPES:
        for cus in elc.CUS:
            assert elc.value_rt(m * n, cus) == 1
            assert _lib.value_model_geometry(elc.VALUE_OBS, elc.VALUE_HIDDEN, m * n, cus=cus)["RT"] == 1
        returns = (3.0 * np.random.RandomState(200 + n).randn(m, n)).astype(np.float32)     # tests/test_value_model_gpu.py: _setup
        keys, want = elc.row_keys(returns, 0), elc.want_keys(returns, 0)
        assert np.array_equal(elc.value_reduce(keys, n, 16), want)
        for mutant in ("V1", "V3"):
            assert np.array_equal(elc.value_reduce(keys, n, 16, mutant), want), (mutant, m, n)
    # V2 drops the rows behind an env boundary inside a workgroup: 14 rows of (3, 70) and of (2, 130), none of the other two -
    # it shows there only when an env's winner happens to be one of them
    assert [int(elc.v2_lost_rows(16, n, m * n).sum()) for m, n in elc.OLD_VALUE_SHAPES] == [0, 0, 14, 14]
    for m, n in elc.OLD_SHAPES:                 # the scorers' 64 rows per workgroup: S2 is the kernel; two envs per tile at most
        returns = (3.0 * np.random.RandomState(n).randn(m, n)).astype(np.float32)
        keys, want = elc.row_keys(returns, 0), elc.want_keys(returns, 0)
        assert np.array_equal(elc.scorer_reduce(keys, n, 64, "S2"), want)
        f = elc.facts(64, n, m * n)
        assert f["interior_envs"] == 0 and not f["run1_last"]
        env = elc.gather_env(m * n, n)
        assert max(len(set(env[lo:lo + 16])) for lo in range(0, m * n, 16)) <= 2


# ------------------------------------------------------------------------------------------
# 3. what the tables contain, at every device size
# ------------------------------------------------------------------------------------------
def _claims(W, table):
    """``table``: (n, rows) pairs at one W."""
    fs = [elc.facts(W, n, rows) for n, rows in table]
    assert max(f["interior_envs"] for f in fs) >= 3, "a workgroup with three whole envs in its interior"
    assert any(f["run1_first"] for f in fs) and any(f["run1_last"] for f in fs), "an env run of length 1 on a first / last row"
    # an env spanning three workgroups has at least W + 2 rows: 129 is the largest n of the table, so 64 rows per workgroup
    # (the trajectory scorers' only size) is the largest W with one
    assert any(f["three_wgs"] for f in fs) == (W <= 64), "an env spanning three workgroups"
    if W == 128:
        assert any(f["in_wave1"] for f in fs), "an env wholly inside wave 1"
        assert any(f["across_waves"] for f in fs), "an env across rows 63 | 64"
        assert any(65 <= f["last_rows"] <= 127 for f in fs) and any(f["last_rows"] <= 64 for f in fs)


@pytest.mark.parametrize("cus", elc.CUS)
def test_structural_claims_of_the_value_table(cus):
    table = elc.value_table(cus)
    kept = {}
    for rt, n, tail, m, rows in table:
        got = _lib.value_model_geometry(elc.VALUE_OBS, elc.VALUE_HIDDEN, rows, cus=cus)["RT"]
        assert got == elc.value_rt(rows, cus)
        assert _lib.value_model_geometry(elc.VALUE_OBS, elc.VALUE_WIDE, rows, cus=cus)["RT"] == got      # the wide network: the same caps
        if got == rt:
            kept.setdefault((rt, n), []).append((tail, rows))
    # a layout whose search for its tail class overshoots the RT's window of row counts runs under the next RT: the GPU test
    # drops it by the geometry it asserts.  None is lost at 256 and 304 CUs, and every (RT, n) keeps a layout at 32 and 64.
    lost = len(table) - sum(len(v) for v in kept.values())
    assert set(kept) == {(rt, n) for rt in elc.RTS for n in elc.N_LAYOUT if elc.layouts(16 * rt, n, 1)}
    assert lost == 0 or cus < 256, lost
    for rt in elc.RTS:
        _claims(16 * rt, [(n, rows) for (r, n), v in kept.items() if r == rt for _, rows in v])


@pytest.mark.parametrize("cus", elc.CUS)
def test_reward_model_cases_take_their_geometry(cus):
    for geo, a, h in elc.MODEL_GEOMETRIES:
        for n in elc.MODEL_NS:
            rows = elc.model_envs(a, cus, n) * n
            g = _lib.reward_model_geometry(elc.MODEL_OBS, elc.MODEL_ACT, elc.MODEL_HIDDEN, rows, h, cus=cus)
            assert (g["RT"], g["CT"], g["S"]) == geo, (geo, n, cus, g)
    assert {16 * g[1] for g, _, _ in elc.MODEL_GEOMETRIES} == set(elc.WS)          # every workgroup size of the table


def test_structural_claims_of_the_scorer_tables():
    for W in elc.WS:                            # 64: l2a_score_traj_k, l2a_score_term_k; 16 CT: l2a_score_mlp_k
        _claims(W, [(n, rows) for n, _, _, rows in elc.scorer_table(W)])


def test_every_pattern_is_planted_at_every_workgroup_size():
    for W in elc.WS:
        count = {p: 0 for p in elc.PLANTS}
        for n in elc.N_LAYOUT:
            for tail, m, rows in _all_layouts(W, n):
                planted = _case(W, n, tail, m)[1]
                for p in planted:
                    count[p] += 1
                if m >= 7:      # enough envs for all of them; twins across a workgroup boundary wherever n does not divide W
                    assert set(planted) >= {"win_first", "win_last", "all_ninf", "one_nan", "all_nan"}, (W, n, tail)
                    assert ("twins_wg" in planted) == (n >= 2 and W % n != 0), (W, n, tail)
        print("W = %d: planted %s" % (W, count))
        assert all(count[p] >= 10 for p in elc.PLANTS if p != "twins_wave")
        assert (count["twins_wave"] >= 10) == (W == 128)


# ------------------------------------------------------------------------------------------
# 4. the plan cases
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,m,n", [(model, m, n) for model in elc.PLAN_MODELS for m, n in elc.PLAN_SHAPES])
def test_plan_cases_meet_their_input_conditions(model, m, n):
    """Checked on the oracle alone, as tests/test_termination.py checks its own: few ambiguous rows, enough rows that terminate
    early - at step 0 and at a middle step - and enough that survive."""
    import termination_cases as tc
    p = elc.plan_case(model, m, n)
    want, steps, ambiguous, alive = tc.plan_want(p, p["reward_fn"], terminal_reward=-3.5)
    h = elc.PLAN_H
    print("%s m %d n %d: guard %s, %.1f %% ambiguous, %.1f %% terminate before h, %.1f %% survive"
          % (model, m, n, p["guards"], 100 * ambiguous.mean(), 100 * (steps < h).mean(), 100 * alive.mean()))
    assert ambiguous.mean() <= 0.01 and (steps < h).mean() >= 0.20 and alive.mean() >= 0.20
    assert (steps == 1).any() and ((steps > 1) & (steps < h)).any() and np.isfinite(want).all()
    assert np.all(p["obs0"][1:] != p["obs0"][:-1])
