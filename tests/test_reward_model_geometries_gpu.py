"""The reward-model scorer (``l2a_score_mlp_k``) under every launch geometry ``(RT, CT, S)`` its launcher can pick, at the
multi-pass horizons and ``CT > 1`` row counts the products run (tests/reward_model_geometries.py).

Per row of the table, with the device's own CU count and LDS size: (1) the launcher's decision (``l2a_reward_model_geometry``)
is the geometry the row is there for; (2) the returns against the float64 restatement, bar 1e-4; (3) the returns are bit for
bit the fp32 sum of ``predict``'s per-step rewards taken in chunks that run ``CT = 1`` in one pass, and - on ``CT > 1`` rows -
those of two shards that take another geometry; (4) guard floats, keys at two candidate offsets, the keys-only call.  Two more
tests put a non-finite input and an exact twin of the best candidate into later passes and later candidate tiles.

Measured on one MI355X: the maximum over all rows of ``|got - want| / max(1, |want|)`` is printed per row and recorded in
DESIGN section 4.9."""

import numpy as np
import pytest
import torch

import reward_model_cases as rmc
import reward_model_geometries as rmg
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
from test_reward_model_gpu import RTOL, _accumulate_f32, _dev, _want_keys, rel_err

pytestmark = pytest.mark.gpu

DISCOUNTS = (1.0, 0.9)
GUARD = 8
FILL = -123.5
SCORED = [r for r in rmg.ROWS if r.id not in rmg.PREDICT]
MULTI_PASS_CT1, MULTI_PASS_CT4 = "g818_h13_m3", "g842_h9"


def _device():
    info = _lib.Context.get(0).info()
    return int(info["compute_units"]), int(info["lds_per_block"])


def _geometry(row, rows, h):
    cus, lds = _device()
    g = _lib.reward_model_geometry(row.obs, row.act, row.hidden, rows, h, cus=cus, lds_per_block=lds)
    return (g["RT"], g["CT"], g["S"]), g


_SETUPS = {}


def _setup(row):
    """Model, inputs (host and device) and the float64 returns of a row: built once, never modified."""
    if row.id not in _SETUPS:
        cus, _ = _device()
        n = rmg.plan_n(row, cus)
        params = rmc.reward_weights(row.obs, row.act, row.hidden)
        norm = rmc.reward_norm(row.obs, row.act)
        native = NativeRewardModel(row.obs, row.act, row.hidden, row.activation)
        native.set_weights(params)
        native.set_norm(norm)
        obs0, traj, actions = rmc.inputs(300 + rmg.ROWS.index(row), row.m, n, row.obs, row.act, row.h, norm)
        fn = rmc.reward_fn(params, norm, row.activation)
        want = {d: rmc.returns_f64(fn, obs0, traj, actions, n, d) for d in DISCOUNTS}
        _SETUPS[row.id] = dict(native=native, n=n, obs0=obs0, traj=traj, actions=actions, want=want, cus=cus,
                               dev=(_dev(obs0), _dev(traj), _dev(actions)), scored={}, step=None)
    return _SETUPS[row.id]


def _score_arrays(row, native, obs0_d, traj_d, act_d, n, discount, cand_offset, returns=True):
    """One scoring call on device tensors: the returns between their guard floats (or None) and the keys."""
    m, h = row.m, row.h
    rets = torch.full((GUARD + m * n + GUARD,), FILL, dtype=torch.float32, device="cuda:0") if returns else None
    best = torch.full((m,), -1, dtype=torch.int64, device="cuda:0")
    native.score_trajectory(obs0_d, traj_d, act_d, m, n, h, discount, cand_offset=cand_offset,
                            returns_out=rets[GUARD:GUARD + m * n] if returns else None, best_key=best)
    torch.cuda.synchronize()
    return (rets.cpu().numpy() if returns else None), best.cpu().numpy().view(np.uint64)


def _predict_guarded(s):
    """The predict twin: every row in ONE call (the row's geometry), rewards between guard floats."""
    n = s["n"]
    out = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.float32, device="cuda:0")
    s["native"].predict(_dev(np.repeat(s["obs0"], n, axis=0)), s["dev"][2][0].contiguous(), s["dev"][1][0].contiguous(),
                        out=out[GUARD:GUARD + n])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _scored(row, discount, cand_offset=0):
    """The row's own scoring call (guards included), cached: the clean run the other checks compare with."""
    s = _setup(row)
    key = (discount, cand_offset)
    if key not in s["scored"]:
        if row.id in rmg.PREDICT:
            s["scored"][key] = (_predict_guarded(s), None)
        else:
            s["scored"][key] = _score_arrays(row, s["native"], *s["dev"], s["n"], discount, cand_offset)
    return s["scored"][key]


def _unguarded(rets):
    assert np.all(rets[:GUARD] == FILL) and np.all(rets[-GUARD:] == FILL)      # guard floats untouched
    return rets[GUARD:-GUARD]


def _step_rewards(row):
    """``l2a_reward_model_predict`` step by step in chunks of at most ``16 * cus`` rows - every chunk is asserted to run
    ``CT = 1`` in one pass - fp32 ``[h, rows]``."""
    s = _setup(row)
    if s["step"] is None:
        native, n, cus = s["native"], s["n"], s["cus"]
        rows, chunk = row.m * n, 16 * cus
        for lo in range(0, rows, chunk):
            geo, g = _geometry(row, min(chunk, rows - lo), 1)
            assert geo[1:] == (1, 1) and g["passes"] == 1, geo
        state = _dev(np.repeat(s["obs0"], n, axis=0))
        out = np.empty((row.h, rows), dtype=np.float32)
        for t in range(row.h):
            nxt, act = s["dev"][1][t], s["dev"][2][t]
            for lo in range(0, rows, chunk):
                hi = min(rows, lo + chunk)
                out[t, lo:hi] = native.predict(state[lo:hi].contiguous(), act[lo:hi].contiguous(), nxt[lo:hi].contiguous()).cpu().numpy()
            state = nxt
        s["step"] = out
    return s["step"]


# ------------------------------------------------------------------------------------------
# 1. the launcher's decision on this device
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rmg.ROWS, ids=lambda r: r.id)
def test_row_takes_its_geometry_on_this_device(row):
    cus, _ = _device()
    n = rmg.plan_n(row, cus)
    geo, g = _geometry(row, row.m * n, row.h)
    assert geo == row.expect, "%s: %d CUs pick %s for %d x %d x %d" % (row.id, cus, geo, row.m, n, row.h)
    assert g["workgroups"] == -(-row.m * n // (16 * geo[1])) and g["passes"] == -(-row.h // geo[2])


# ------------------------------------------------------------------------------------------
# 2. against the float64 restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("discount", DISCOUNTS)
@pytest.mark.parametrize("row", rmg.ROWS, ids=lambda r: r.id)
def test_returns_match_the_float64_restatement(row, discount):
    s = _setup(row)
    assert _geometry(row, row.m * s["n"], row.h)[0] == row.expect
    rets = _unguarded(_scored(row, discount)[0])
    want = s["want"][discount]
    assert np.isfinite(want).all() and np.std(want) > 0.01
    err = rel_err(rets, want)
    print("geometry %s %s %d x %d x %d discount %.1f vs float64 restatement: %.2e"
          % (row.id, row.expect, row.m, s["n"], row.h, discount, err))
    assert err < RTOL


# ------------------------------------------------------------------------------------------
# 3. bits across geometries
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rmg.ROWS, ids=lambda r: r.id)
def test_returns_are_the_fp32_sum_of_one_pass_ct1_predict(row):
    s = _setup(row)
    assert _geometry(row, row.m * s["n"], row.h)[0] == row.expect
    step = _step_rewards(row)
    for discount in DISCOUNTS:
        rets = _unguarded(_scored(row, discount)[0])
        assert np.array_equal(rets.view(np.uint32), _accumulate_f32(step, discount).view(np.uint32)), discount


@pytest.mark.parametrize("row", [r for r in SCORED if r.expect[1] > 1], ids=lambda r: r.id)
def test_two_shards_of_another_geometry_give_the_same_bits(row):
    s = _setup(row)
    m, n, h, od, ad, cus = row.m, s["n"], row.h, row.obs, row.act, s["cus"]
    most = 16 * cus // m                        # candidates per env of a shard of at most 16 * cus rows
    cut = (n // 2) | 1
    if max(cut, n - cut) > most:                # the plan is longer than two such shards: its first 2 * most candidates or so
        cut = most - 1 + most % 2
    hi = min(n, cut + most)
    assert cut % 2 == 1 and 0 < cut < hi
    t4, a4 = s["traj"].reshape(h, m, n, od), s["actions"].reshape(h, m, n, ad)
    for discount in DISCOUNTS:
        full, keys = _scored(row, discount, 1000)
        full = _unguarded(full).reshape(m, n)
        parts, pkeys = [], []
        for lo, up in ((0, cut), (cut, hi)):
            geo, _ = _geometry(row, m * (up - lo), h)
            assert geo != row.expect and geo[1] < row.expect[1], geo
            r, k = _score_arrays(row, s["native"], s["dev"][0], _dev(t4[:, :, lo:up].reshape(h, -1, od)),
                                 _dev(a4[:, :, lo:up].reshape(h, -1, ad)), up - lo, discount, 1000 + lo)
            parts.append(_unguarded(r).reshape(m, up - lo))
            pkeys.append(k)
        both = np.concatenate(parts, axis=1)
        assert np.array_equal(both.view(np.uint32), full[:, :hi].view(np.uint32))
        assert np.array_equal(np.maximum(pkeys[0], pkeys[1]), _want_keys(full[:, :hi], 1000))
        if hi == n:
            assert np.array_equal(np.maximum(pkeys[0], pkeys[1]), keys)


# ------------------------------------------------------------------------------------------
# 4. keys and guards
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cand_offset", [0, 1000])
@pytest.mark.parametrize("row", SCORED, ids=lambda r: r.id)
def test_keys_and_guards(row, cand_offset):
    s = _setup(row)
    m, n = row.m, s["n"]
    assert _geometry(row, m * n, row.h)[0] == row.expect
    for discount in DISCOUNTS:
        rets, keys = _scored(row, discount, cand_offset)
        rets = _unguarded(rets).reshape(m, n)
        assert np.array_equal(keys, _want_keys(rets, cand_offset))
        none, only = _score_arrays(row, s["native"], *s["dev"], n, discount, cand_offset, returns=False)
        assert none is None and np.array_equal(only, keys)
        base = _unguarded(_scored(row, discount, 0)[0])
        assert np.array_equal(rets.reshape(-1).view(np.uint32), base.view(np.uint32))      # cand_offset moves no bit


# ------------------------------------------------------------------------------------------
# 5. non-finite inputs and exact ties in later passes and later candidate tiles
# ------------------------------------------------------------------------------------------
def _edited(row, s, edit):
    """The row's plan with ``edit(traj4, act4)`` applied to copies ``[h, m, n, *]``, scored at discount 0.9, offset 5."""
    m, n, h = row.m, s["n"], row.h
    t4, a4 = s["traj"].reshape(h, m, n, row.obs).copy(), s["actions"].reshape(h, m, n, row.act).copy()
    edit(t4, a4)
    rets, keys = _score_arrays(row, s["native"], s["dev"][0], _dev(t4.reshape(h, m * n, row.obs)),
                               _dev(a4.reshape(h, m * n, row.act)), n, 0.9, 5)
    return _unguarded(rets).reshape(m, n), keys


@pytest.mark.parametrize("rid", [MULTI_PASS_CT1, MULTI_PASS_CT4])
def test_a_non_finite_input_in_a_later_pass_and_tile(rid):
    row = rmg.by_id(rid)
    s = _setup(row)
    m, n, h = row.m, s["n"], row.h
    (RT, CT, S), g = _geometry(row, m * n, h)
    assert (RT, CT, S) == row.expect and g["passes"] >= 2 and h % S != 0           # a second pass and a ragged last one
    base = _unguarded(_scored(row, 0.9, 5)[0]).reshape(m, n)
    # the victim: second workgroup, its LAST candidate tile (at CT = 1: its only one), sixth candidate of the tile
    r = 16 * CT + 16 * (CT - 1) + 5
    assert r < m * n and (r % (16 * CT)) // 16 == CT - 1
    env, c = r // n, r % n

    def nan_state(t4, a4):
        t4[S, env, c, row.obs - 1] = np.nan             # next observation of step S: the first step of the second pass

    def inf_action(t4, a4):
        a4[h - 1, env, c, 0] = np.inf                   # the last step of the ragged last pass

    for edit in (nan_state, inf_action):
        rets, keys = _edited(row, s, edit)
        assert np.isnan(rets[env, c]) and np.isnan(rets).sum() == 1
        mask = np.ones((m, n), dtype=bool)
        mask[env, c] = False
        assert np.array_equal(rets[mask].view(np.uint32), base[mask].view(np.uint32))
        assert _lib.key_decode(keys[env])[1] == 5 + c and np.array_equal(keys, _want_keys(rets, 5))


@pytest.mark.parametrize("rid", [MULTI_PASS_CT1, MULTI_PASS_CT4])
def test_an_exact_twin_in_another_candidate_tile(rid):
    row = rmg.by_id(rid)
    s = _setup(row)
    m, n, h = row.m, s["n"], row.h
    (RT, CT, S), g = _geometry(row, m * n, h)
    assert (RT, CT, S) == row.expect and g["passes"] >= 2
    base = _unguarded(_scored(row, 0.9, 5)[0]).reshape(m, n)
    env = m // 2
    top = int(np.argmax(base[env]))
    r_top = env * n + top
    # the twin: a row of the same env in ANOTHER 16-candidate tile - of the same workgroup where a workgroup has several
    rows = np.arange(env * n, (env + 1) * n)
    other = rows[rows // 16 != r_top // 16]
    if CT > 1:
        other = other[other // (16 * CT) == r_top // (16 * CT)]
    assert other.size > 0
    twin = int(other[other.size // 2]) - env * n

    def copy(t4, a4):
        t4[:, env, twin], a4[:, env, twin] = t4[:, env, top], a4[:, env, top]

    rets, keys = _edited(row, s, copy)
    assert rets[env, twin].view(np.uint32) == rets[env, top].view(np.uint32) == base[env, top].view(np.uint32)
    assert _lib.key_decode(keys[env])[1] == 5 + min(top, twin)
    assert np.array_equal(keys, _want_keys(rets, 5))
    keep = np.ones((m, n), dtype=bool)
    keep[env, twin] = False
    assert np.array_equal(rets[keep].view(np.uint32), base[keep].view(np.uint32))
