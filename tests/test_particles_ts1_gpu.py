"""TS1 particle plans on the GPU (``csrc/l2a_particles.hip``: ``l2a_particle_shuffle_k``; ``l2a_plan_rs_particles_ts1``;
``MPCController(particle_sampling="ts1")``) against ``tests/particle_ts1_reference.py``.

Bounds (derived, none measured and then set).  The shuffle only copies, so it is held to the index restatement BIT FOR BIT, NaN
payloads included, and its Philox permutations to ``l2a_particle_perm`` (which ``test_particles_ts1.py`` holds to the NumPy
restatement, exactly).  The plan entry with identity permutations, and at ``h = 1``, is bit-equal to ``l2a_plan_rs_particles`` - the
chunk chain's documented bit-identity.  Under Philox permutations every particle return lies within the project's bar, 1e-4 of
max |R|, of the float64 restatement under the SAME permutations (a permutation only moves rows: the error of a particle's return
is the rollout's own, as for TS-infinity), and scores, spread and keys equal ``l2a_particle_score`` of the exposed returns bit for
bit.  Every test prints the maxima it measured (``-s``).

Seen on an MI355X: the worst particle return of the whole Philox grid is 4.0e-07 of max |R| off the restatement (the bar is 1e-4)."""

import ctypes

import numpy as np
import pytest

import particle_reference as pr
import particle_ts1_reference as t1
import test_particles_gpu as tp
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.utils import synthetic

pytestmark = pytest.mark.gpu

OD, AD = tp.OD, tp.AD
BAR = 1e-4
GUARD = 64
FILL, FENCE = 0x5EA7BEEF, 0x0BADC0DE
SEEDS = (0x0123456789ABCDEF, 7)
TOP = (1 << 31) - 1
LIMIT = 1 << 33
H = 7


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from learning_to_adapt_amd.dynamics.native_model import _stream_ptr
    return _stream_ptr(_torch().device("cuda:0"))


class _Words:
    """A device output of 32-bit words between two runs of guard words, pre-filled with a sentinel."""

    def __init__(self, shape):
        torch = _torch()
        self.shape = tuple(shape)
        self.size = int(np.prod(shape))
        self.flat = torch.full((self.size + 2 * GUARD,), FENCE, dtype=torch.int32, device="cuda:0")
        self.view = self.flat[GUARD:GUARD + self.size]
        self.view.fill_(FILL)

    def host(self, what):
        h = self.flat.cpu().numpy().view(np.uint32)
        assert np.all(h[:GUARD] == FENCE) and np.all(h[GUARD + self.size:] == FENCE), "guard words overwritten: " + what
        return h[GUARD:GUARD + self.size].reshape(self.shape).copy()

    def untouched(self, what):
        return bool(np.all(self.host(what) == FILL))


def bit_patterns(m, E, n, O, salt):
    """State ``[m, E, n, O]`` and return ``[m, E, n]`` words, all distinct (an odd multiplier is a bijection of the 32-bit words) -
    NaNs with payloads among them as they fall - with a quiet and a signalling NaN, both infinities and -0 planted."""
    count = m * E * n * (O + 1)
    words = ((np.arange(count, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    special = np.array([0x7FC00123, 0xFFA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x7F800001], dtype=np.uint32)
    k = min(len(special), count)
    words[np.linspace(0, count - 1, k).astype(np.int64)] = special[:k]
    return words[:m * E * n * O].reshape(m, E, n, O), words[m * E * n * O:].reshape(m, E, n)


def run_shuffle(S, R, table=None, seed=0, offset=0, t=0, cand_offset=0, expect_rc=_lib.L2A_OK, args=None, null=None, alias=None,
                S_d=None, R_d=None):
    """One ``l2a_particle_shuffle`` on word arrays; returns the two outputs (guards checked, inputs checked unchanged).  ``args``
    overrides the integer arguments of a call that is to be refused, ``null`` names a buffer passed as NULL, ``alias`` an output
    passed as its input."""
    torch = _torch()
    ctx = _lib.Context.get(0)
    m, E, n, O = S.shape
    S_d = _dev(S.view(np.int32)) if S_d is None else S_d
    R_d = _dev(R.view(np.int32)) if R_d is None else R_d
    So, Ro = _Words(S.shape), _Words(R.shape)
    tab_d = None if table is None else _dev(np.asarray(table, dtype=np.uint8))
    a = dict(t=t, m=m, E=E, n=n, obs_dim=O, cand_offset=cand_offset)
    a.update(args or {})
    ptrs = dict(state_in=_ptr(S_d), ret_in=_ptr(R_d), state_out=_ptr(So.view), ret_out=_ptr(Ro.view))
    if null:
        ptrs[null] = None
    if alias:
        ptrs[alias] = ptrs[alias.replace("_out", "_in")]
    rc = ctx.lib.l2a_particle_shuffle(ctx.handle, ptrs["state_in"], ptrs["ret_in"], ptrs["state_out"], ptrs["ret_out"], _ptr(tab_d),
                                      seed, offset, a["t"], a["m"], a["E"], a["n"], a["obs_dim"], a["cand_offset"], _stream())
    torch.cuda.synchronize()
    what = "shuffle m=%d E=%d n=%d O=%d offset=%d t=%d cand_offset=%d %s" % (m, E, n, O, offset, t, cand_offset, args or "")
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    assert np.array_equal(S_d.cpu().numpy().view(np.uint32), S) and np.array_equal(R_d.cpu().numpy().view(np.uint32), R), "input changed: " + what
    if expect_rc != _lib.L2A_OK:
        assert So.untouched(what) and Ro.untouched(what), "output written by a refused call: " + what
        return None
    return So.host(what), Ro.host(what)


def lib_perm_table(seed, offset, t, m, n, E, cand_offset=0):
    out = np.full((m, n, E), 255, dtype=np.uint8)
    rc = _lib.load().l2a_particle_perm(seed, offset, t, m, 0, m, cand_offset, n, E, out.ctypes.data)
    assert rc == _lib.L2A_OK
    return out


def injected_table(rs, m, n, E):
    """Row by row in turn: the identity, the reversal, a random permutation, a random permutation with one entry >= E (the
    restatement clamps it to E - 1 as the library documents)."""
    tab = np.empty((m, n, E), dtype=np.uint8)
    for c in range(m * n):
        kind = c % 4
        row = np.arange(E) if kind == 0 else np.arange(E)[::-1] if kind == 1 else rs.permutation(E)
        row = row.astype(np.uint8)
        if kind == 3:
            row[rs.randint(E)] = (E, 16, 200, 255)[(c // 4) % 4]
        tab[c // n, c % n] = row
    return tab


# ------------------------------------------------------------------------------------------------------- 1. the shuffle alone
@pytest.mark.parametrize("E", [1, 2, 3, 5, 8, 16])
def test_shuffle_is_bit_equal_to_the_index_restatement(E):
    rs = np.random.RandomState(40 + E)
    launches = 0
    for n in (1, 2, 63, 64, 65, 257):
        for m in (1, 3):
            for O in (1, 17, 20, 49):
                S, R = bit_patterns(m, E, n, O, salt=n * 1000 + m * 100 + O)
                S_d, R_d = _dev(S.view(np.int32)), _dev(R.view(np.int32))
                what = "E=%d n=%d m=%d O=%d" % (E, n, m, O)
                # injected tables
                tab = injected_table(rs, m, n, E)
                s, r = run_shuffle(S, R, tab, S_d=S_d, R_d=R_d)
                ws, wr = t1.shuffle(S, R, tab)
                assert np.array_equal(s, ws) and np.array_equal(r, wr), "injected: " + what
                again = run_shuffle(S, R, tab, S_d=S_d, R_d=R_d)
                assert np.array_equal(again[0], s) and np.array_equal(again[1], r), "run to run: " + what
                launches += 2
                # Philox: both ends of the offset range, two seeds, both ends of the candidate range
                for offset in (0, LIMIT - H * m):
                    for seed in SEEDS:
                        for co in (0, TOP - n):
                            s, r = run_shuffle(S, R, None, seed, offset, H - 1, co, S_d=S_d, R_d=R_d)
                            ws, wr = t1.shuffle(S, R, lib_perm_table(seed, offset, H - 1, m, n, E, co))
                            assert np.array_equal(s, ws) and np.array_equal(r, wr), "philox offset=%d seed=%d co=%d: %s" % (offset, seed, co, what)
                            launches += 1
                # two shards cut at an odd candidate equal the unsharded call
                if n >= 2:
                    cut = (n // 2) | 1 if (n // 2) | 1 < n else 1
                    whole = run_shuffle(S, R, None, SEEDS[0], 5, 2, 0, S_d=S_d, R_d=R_d)
                    parts = [run_shuffle(np.ascontiguousarray(S[:, :, lo:hi]), np.ascontiguousarray(R[:, :, lo:hi]), None, SEEDS[0], 5, 2, lo)
                             for lo, hi in ((0, cut), (cut, n))]
                    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=2), whole[0]), "shards: " + what
                    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=2), whole[1]), "shards: " + what
                    launches += 3
    print("[ts1] E=%d: %d shuffle launches, all bit-equal" % (E, launches))


def test_shuffle_refusals_write_nothing():
    S, R = bit_patterns(2, 3, 10, 4, salt=1)
    E = _lib.L2A_EINVAL
    for buf in ("state_in", "ret_in", "state_out", "ret_out"):
        run_shuffle(S, R, expect_rc=E, null=buf)
    run_shuffle(S, R, expect_rc=E, alias="state_out")
    run_shuffle(S, R, expect_rc=E, alias="ret_out")
    for bad in (dict(m=0), dict(E=0), dict(n=0), dict(obs_dim=0), dict(E=17), dict(t=-1), dict(cand_offset=-1),
                dict(cand_offset=TOP - 9), dict(n=1 << 29), dict(m=-1)):
        run_shuffle(S, R, expect_rc=E, args=bad)
    run_shuffle(S, R, offset=LIMIT - 1, expect_rc=E)            # env 1's slot would be 2^33
    run_shuffle(S, R, offset=LIMIT - 2 * H, t=H, expect_rc=E)
    run_shuffle(S, R, offset=(1 << 64) - 1, expect_rc=E)
    run_shuffle(S, R, offset=LIMIT - 2 * H, t=H - 1)            # the last legal slot
    run_shuffle(S, R, cand_offset=TOP - 10)


# ------------------------------------------------------------------------------------------------------------ 2. the plan entry
def run_ts1(model, obs, actions, n, h, m, lam, reward, seed=0, offset=0, table=None, cand_offset=0, discount=1.0,
            expect_rc=_lib.L2A_OK, E=None):
    """One ``l2a_plan_rs_particles_ts1``; host copies of the four outputs (guards checked), as ``test_particles_gpu.run_plan``."""
    torch = _torch()
    E = model.n_sets if E is None else E
    out = dict(score=tp._Out((m, n)), spread=tp._Out((m, n)), members=tp._Out((m, E, n)), keys=tp._Out((m,), keys=True))
    obs_d, act_d = tp._up(np.asarray(obs, dtype=np.float32)), tp._up(np.asarray(actions, dtype=np.float32))
    tab_d = None if table is None else _dev(np.asarray(table, dtype=np.uint8))
    rc = model.lib.l2a_plan_rs_particles_ts1(model.handle, _ptr(obs_d), _ptr(act_d), m, n, h, float(discount), ctypes.byref(reward),
                                             ctypes.c_float(lam), seed, offset, _ptr(tab_d), cand_offset, _ptr(out["score"].view),
                                             _ptr(out["spread"].view), _ptr(out["members"].view), _ptr(out["keys"].view), _stream())
    torch.cuda.synchronize()
    what = "ts1 plan n=%d h=%d m=%d lambda=%g offset=%d cand_offset=%d" % (n, h, m, lam, offset, cand_offset)
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, model.lib.l2a_last_error(model.ctx.handle).decode())
    if expect_rc != _lib.L2A_OK:
        assert all(o.untouched(k + " " + what) for k, o in out.items()), "output written by a refused call: " + what
        return rc
    assert model.ctx.launch_status_value() == 0, what
    return {k: o.host(k + " " + what) for k, o in out.items()}


def philox_tables(seed, offset, m, n, h, E, cand_offset=0):
    if h == 1:
        return np.zeros((0, m, n, E), dtype=np.uint8)
    return np.stack([lib_perm_table(seed, offset, t, m, n, E, cand_offset) for t in range(h - 1)])


def _same(a, b):
    return all(np.array_equal(tp._bits(a[k]) if k != "keys" else a[k], tp._bits(b[k]) if k != "keys" else b[k]) for k in a)


@pytest.mark.parametrize("hidden", tp.WIDTHS)
def test_identity_permutations_and_horizon_one_are_ts_infinity_bit_for_bit(hidden):
    for E in (2, 3, 5):
        env, _, _, model = tp.native_model(hidden, E)
        for c, (n, h, m) in enumerate([(16, 2, 1), (50, 7, 3), (50, 2, 3), (16, 7, 1)]):
            obs, actions = tp.plan_inputs(800 + c, n, h, m)
            lam, co, disc = (0.0, 1.0)[c % 2], (0, 13)[c % 2], (1.0, 0.97)[c % 2]
            want = tp.run_plan(model, obs, actions, n, h, m, lam, env.reward_spec, cand_offset=co, discount=disc)
            got = run_ts1(model, obs, actions, n, h, m, lam, env.reward_spec, table=t1.identity_table(m, n, E, h), cand_offset=co, discount=disc)
            assert _same(got, want), "identity: hidden=%s E=%d n=%d h=%d m=%d" % (hidden, E, n, h, m)
        n, m = 50, 3
        obs, actions = tp.plan_inputs(810, n, 1, m)
        want = tp.run_plan(model, obs, actions, n, 1, m, 1.0, env.reward_spec)
        got = run_ts1(model, obs, actions, n, 1, m, 1.0, env.reward_spec, seed=SEEDS[0], offset=3)
        assert _same(got, want), "h = 1: hidden=%s E=%d" % (hidden, E)


PHILOX_GRID = [(n, h, m, disc) for n in (16, 50) for h in (2, 7) for m in (1, 3) for disc in (1.0, 0.97)]


@pytest.mark.parametrize("E", (2, 3, 5))
@pytest.mark.parametrize("hidden", tp.WIDTHS)
def test_philox_plans_against_the_float64_restatement(hidden, E):
    env, sets, norms, model = tp.native_model(hidden, E)
    worst = 0.0
    for c, (n, h, m, disc) in enumerate(PHILOX_GRID):
        seed, offset, lam, co = SEEDS[c % 2], (0, 12345, LIMIT - h * m)[c % 3], (1.0, 0.0, 4.0)[c % 3], (0, 9)[c % 2]
        obs, actions = tp.plan_inputs(900 + c, n, h, m)
        tables = philox_tables(seed, offset, m, n, h, E, co)
        R64 = t1.particle_returns64(env, sets, norms, obs, actions, n, tables, discount=disc)
        scale = float(np.max(np.abs(R64)))
        got = run_ts1(model, obs, actions, n, h, m, lam, env.reward_spec, seed=seed, offset=offset, cand_offset=co, discount=disc)
        what = "hidden=%s E=%d n=%d h=%d m=%d discount=%g" % (hidden, E, n, h, m, disc)
        err = float(np.max(np.abs(got["members"].astype(np.float64) - R64))) / scale
        worst = max(worst, err)
        print("[ts1] %s: particle returns %.2e of max |R|" % (what, err))
        assert err <= BAR, "particle returns off by %.3e of max |R|: %s" % (err, what)
        again = tp.run_score(model.ctx, got["members"], lam, co)
        assert np.array_equal(tp._bits(got["score"]), tp._bits(again["score"])), "score: " + what
        assert np.array_equal(tp._bits(got["spread"]), tp._bits(again["spread"])), "spread: " + what
        assert np.array_equal(got["keys"], again["keys"]), "keys: " + what
        # the same permutations injected are the same plan
        if c % 4 == 0:
            inj = run_ts1(model, obs, actions, n, h, m, lam, env.reward_spec, table=tables, cand_offset=co, discount=disc)
            assert _same(inj, got), "injected = drawn: " + what
    print("[ts1] hidden=%s E=%d: worst particle return %.2e of max |R|" % (hidden, E, worst))


def test_a_shuffle_changes_the_returns():
    """A non-identity table must not give the TS-infinity returns: guards against a shuffle that is silently skipped."""
    hidden, E, n, h, m = (128, 128), 3, 50, 7, 3
    env, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(950, n, h, m)
    want = tp.run_plan(model, obs, actions, n, h, m, 1.0, env.reward_spec)
    table = t1.identity_table(m, n, E, h)
    table[:] = np.array([1, 2, 0], dtype=np.uint8)                  # every boundary rotates the blocks
    got = run_ts1(model, obs, actions, n, h, m, 1.0, env.reward_spec, table=table)
    differ = tp._bits(got["members"]) != tp._bits(want["members"])
    assert differ.mean() > 0.99, "the shuffle changed %.1f%% of the returns only" % (100 * differ.mean())
    one = t1.identity_table(m, n, E, h)
    one[h - 2, 1, 7] = np.array([0, 2, 1], dtype=np.uint8)          # one candidate of one env, at the last boundary only
    got = run_ts1(model, obs, actions, n, h, m, 1.0, env.reward_spec, table=one)
    differ = tp._bits(got["members"]) != tp._bits(want["members"])
    assert differ[1, 1:, 7].all() and differ.sum() == 2


def test_two_shards_combine_to_the_unsharded_plan():
    hidden, E, n, h, m = (128, 128), 3, 50, 7, 3
    env, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(960, n, h, m)
    whole = run_ts1(model, obs, actions, n, h, m, 1.0, env.reward_spec, seed=SEEDS[1], offset=77)
    a4 = actions.reshape(h, m, n, AD)
    parts = []
    for lo, hi in ((0, 23), (23, 50)):
        local = np.ascontiguousarray(a4[:, :, lo:hi]).reshape(h, m * (hi - lo), AD)
        parts.append(run_ts1(model, obs, local, hi - lo, h, m, 1.0, env.reward_spec, seed=SEEDS[1], offset=77, cand_offset=lo))
    keys = np.maximum(parts[0]["keys"].view(np.uint64), parts[1]["keys"].view(np.uint64))
    assert np.array_equal(keys, whole["keys"].view(np.uint64))
    for k in ("score", "spread"):
        assert np.array_equal(tp._bits(np.concatenate([p[k] for p in parts], axis=1)), tp._bits(whole[k])), k
    assert np.array_equal(tp._bits(np.concatenate([p["members"] for p in parts], axis=2)), tp._bits(whole["members"]))


def test_a_diverged_candidate_stays_in_its_column():
    hidden, E, n, h, m = (128, 128), 5, 50, 7, 3
    env, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(970, n, h, m)
    actions = actions.copy()
    actions[1, 2 * n + 31, 0] = np.nan                              # env 2, candidate 31, from horizon step 1 on
    got = run_ts1(model, obs, actions, n, h, m, 1.0, env.reward_spec, seed=SEEDS[0], offset=0)
    nan = np.isnan(got["members"])
    want = np.zeros_like(nan)
    want[2, :, 31] = True
    assert np.array_equal(nan, want), "NaN returns at %s" % (np.argwhere(nan != want)[:5],)
    assert np.isnan(got["score"][2, 31]) and np.isfinite(np.delete(got["score"][2], 31)).all() and np.isfinite(got["score"][:2]).all()
    assert _lib.key_decode(int(got["keys"][2]))[1] == 31


def test_plan_refusals_write_nothing():
    from learning_to_adapt_amd.envs.synthetic_env import SyntheticEnv
    env = SyntheticEnv("half_cheetah")
    obs, actions = tp.plan_inputs(700, 16, 2, 1)
    single = tp.native_model((32, 32), 1, "single")[3]
    per_block = tp.native_model((32, 32), 2, "per_block")[3]
    for model in (single, per_block):
        assert run_ts1(model, obs, actions, 16, 2, 1, 1.0, env.reward_spec, expect_rc=_lib.L2A_EINVAL, E=2) == _lib.L2A_EINVAL
        assert "mean ensemble" in model.lib.l2a_last_error(model.ctx.handle).decode()
    good = tp.native_model((32, 32), 2)[3]
    assert run_ts1(good, obs, actions, 16, 2, 1, float("nan"), env.reward_spec, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_ts1(good, obs, actions, 16, 2, 1, 1.0, env.reward_spec, cand_offset=-1, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    assert run_ts1(good, obs, actions, 16, 2, 1, 1.0, env.reward_spec, offset=LIMIT - 1, expect_rc=_lib.L2A_EINVAL) == _lib.L2A_EINVAL
    run_ts1(good, obs, actions, 16, 2, 1, 1.0, env.reward_spec, offset=LIMIT - 2)       # offset + h m = 2^33: the last legal plan


# ------------------------------------------------------------------------------------------------------------ 3. the controller
def _controller(planner, sampling, hidden, E, n, h, lam):
    env, sets, norms, _ = tp.native_model(hidden, E)
    kw = dict(risk_coef=lam, particle_sampling=sampling)
    if planner == "rs":
        return tp.particle_controller(env, sets, norms, hidden, E, n, h, draw_ahead=False, **kw)
    if planner == "cem":
        return tp.particle_controller(env, sets, norms, hidden, E, n, h, planner="cem", rng="device", cem_mode="fixed", **kw)
    if planner == "mppi":
        return tp.particle_controller(env, sets, norms, hidden, E, n, h, rng="device", use_mppi=True, **kw)
    return tp.particle_controller(env, sets, norms, hidden, E, n, h, rng="device", use_icem=True, icem_iters=1, **kw)


@pytest.mark.parametrize("planner", ["rs", "cem", "mppi", "icem"])
def test_planners_plan_on_the_ts1_score(planner):
    torch = _torch()
    hidden, E, n, h, m, lam = (128, 128), 3, 50, 7, 3, 1.0
    ctrl = _controller(planner, "ts1", hidden, E, n, h, lam)
    native = ctrl.dynamics_model.planner_model()
    obs = synthetic.make_obs0(m, OD)
    torch.manual_seed(11)
    np.random.seed(11)
    for step in range(2):
        plans0 = getattr(native, "particle_plans", 0)
        act, _ = ctrl.get_actions(obs)
        assert np.isfinite(act).all()
        assert native.particle_plans == plans0 + 1
        assert ctrl._particles["ts1_offset"] == step * h * m, "step %d consumed offset %d" % (step, ctrl._particles["ts1_offset"])
        diag = ctrl.particle_diagnostics(tables=True)
        members = diag["member_returns_table"]
        assert members.shape[:2] == (m, E) and np.isfinite(members).all()
        again = tp.run_score(native.ctx, members, lam, cand_offset=ctrl._particles["cand_offset"])
        score = again["score"]
        if diag["score_table"] is not None:
            assert np.array_equal(tp._bits(diag["score_table"]), tp._bits(score)), "the planner's table is not the particle score"
        assert np.array_equal(tp._bits(diag["spread_table"]), tp._bits(again["spread"]))
        idx = np.array([pr.argmax_nan_first(row) for row in score])
        assert np.array_equal(diag["index"], idx) and np.array_equal(ctrl.last_plan["best_index"], idx)
        assert np.array_equal(tp._bits(diag["score"]), tp._bits(score[np.arange(m), idx]))
        assert np.array_equal(tp._bits(diag["member_returns"]), tp._bits(members[np.arange(m), :, idx]))


def test_tsinf_on_the_controller_is_unchanged():
    hidden, E, n, h, m, lam = (128, 128), 3, 50, 7, 3, 1.0
    env, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(990, n, h, m)
    want = tp.run_plan(model, obs, actions, n, h, m, lam, env.reward_spec)
    ts1 = None
    for sampling in ("tsinf", "ts1"):
        ctrl = _controller("rs", sampling, hidden, E, n, h, lam)
        np.random.seed(990)
        ctrl.get_actions(obs)
        diag = ctrl.particle_diagnostics(tables=True)
        if sampling == "tsinf":
            assert np.array_equal(tp._bits(diag["member_returns_table"]), tp._bits(want["members"]))
            assert np.array_equal(tp._bits(diag["spread_table"]), tp._bits(want["spread"]))
            assert diag["index"][0] == _lib.key_decode(int(want["keys"][0]))[1]
            assert "ts1_offset" not in ctrl._particles
        else:
            ts1 = diag["member_returns_table"]
    assert not np.array_equal(tp._bits(ts1), tp._bits(want["members"])), "particle_sampling='ts1' planned TS-infinity"
