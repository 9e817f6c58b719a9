"""TS1 particle plans of reward programs and reward models on the GPU (``csrc/l2a_particle_step.hip``: ``l2a_particle_step_k``;
``l2a_plan_rs_particles_ts1_program`` / ``_reward_model``; ``MPCController(ts1_step_rewards=True)``) against
``tests/particle_ts1_step_reference.py`` and ``tests/particle_ts1_reference.py``.

Bounds (derived, none measured and then set).  The step kernel is held to the fp32 restatement BIT FOR BIT: the dealt states as
32-bit words, NaN payloads included; the returns with every NaN counting as the same NaN (``test_particles_gpu._canon``: which NaN
an operation returns is the one thing IEEE 754 leaves open, and x86 and gfx950 differ on it).  Its Philox permutations are
``l2a_particle_perm``'s.  The plan entries with identity permutations, and at ``h = 1``, are bit-equal to the TS-infinity entries
``l2a_plan_rs_particles_program`` / ``_reward_model`` - three documented facts: the carry chain's bit-identity, the scorers'
"a row's bits are independent of the geometry", and ``R + fp32(disc) * r`` in step order on both sides.  Under Philox permutations
every particle return lies within the project's bar, 1e-4 of max |R|, of the float64 restatement under the SAME permutations; a
particle whose ``INRANGE`` input comes within ``1e-3 max(1, |bound|)`` of a bound anywhere on its way is left out (rounding may flip
a whole coefficient there), at most 2 % of a case's particles.  Scores, spread and keys equal ``l2a_particle_score`` of the exposed
returns bit for bit.  Every test prints the maxima it measured (``-s``).

Seen on an MI355X: 1 280 step launches bit-equal; the worst particle return of the 128 Philox plans is 1.5e-06 of max |R| off the
restatement (program 1.5e-06, reward model 9.6e-07; the bar is 1e-4) with at most 0.53 % of a case's particles left out (the cap
is 2 %); the controller's random-shooting plan 1.1e-06, none left out; an accepted plan of 200 000 particles grows the model's
buffer by 60.8 MB, the same plan refused by none.

``every_kind_program`` reads ``next[5]``: at ``obs_dim = 5`` the same program is built with that one index moved to ``obs_dim - 1``."""

import ctypes

import numpy as np
import pytest

import cases
import particle_reference as pr
import particle_ts1_reference as t1
import particle_ts1_step_reference as ps
import reward_model_cases as rmc
import reward_program_cases as rpc
import test_particles_gpu as tp
import test_particles_ts1_gpu as tg
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs import RewardProgram
from learning_to_adapt_amd.utils import synthetic

pytestmark = pytest.mark.gpu

OD, AD = tp.OD, tp.AD
BAR = 1e-4
MARGIN, MARGIN_CAP = 1e-3, 0.02
SEEDS = tg.SEEDS
TOP, LIMIT = tg.TOP, tg.LIMIT
H = 7
DIMS = ((20, 6), (5, 1), (17, 3), (41, 9))     # the last: 128 rows per pass, not 256 - a 160-particle workgroup takes two uneven passes
RM_HIDDEN = (64,)
EINVAL = _lib.L2A_EINVAL


def _torch():
    import torch
    return torch


_dev, _ptr, _stream = tg._dev, tg._ptr, tg._stream


def _same_returns(a, b):
    return np.array_equal(tp._canon(np.ascontiguousarray(a).view(np.float32)), tp._canon(np.ascontiguousarray(b).view(np.float32)))


def every_kind(obs_dim, act_dim):
    if obs_dim > 5:
        return rpc.every_kind_program(obs_dim, act_dim)
    goal = np.array([0.5, -1.25, 2.0])
    return (RewardProgram().with_bias(0.5)
            .linear("obs", min(3, obs_dim - 1), 0.3)
            .linear("delta", obs_dim - 2, 0.7)
            .in_range("next", obs_dim - 1, -2.0, 3.5, coef=2.0)
            .sqsum("act", 0, act_dim, -0.05)
            .sqsum("obs", obs_dim - 4, 4, -0.01)
            .norm("next", 0, 3, -0.1, target=goal)
            .norm("delta", 2, 2, -0.2))


def float_words(rs, shape, scale=1.5):
    """Finite fp32 values as 32-bit words, with a NaN, both infinities and -0 planted where the array is large enough."""
    a = (rs.randn(*shape) * scale).astype(np.float32).view(np.uint32).copy()
    flat = a.reshape(-1)
    special = np.array([0x7FC00123, 0x7F800000, 0xFF800000, 0x80000000], dtype=np.uint32)
    if flat.size >= 64:
        flat[np.linspace(3, flat.size - 2, len(special)).astype(np.int64)] = special
    return a


def run_step(pre, post, act, program=None, rewards=None, ret_in=None, table=None, last=False, disc=1.0, seed=0, offset=0, t=0,
             cand_offset=0, expect_rc=_lib.L2A_OK, args=None, null=None, alias=None, stride=None, act_buf=None):
    """One ``l2a_particle_step`` on word arrays (``pre [m, E, n, O]`` or ``[m, E, O]``, ``post [m, E, n, O]``, ``act [m, E, n, A]``);
    the outputs sit between guard words, the inputs are checked unchanged, and the outputs of an accepted call are held to the restatement
    under the injected ``table`` or the library's own Philox table.  ``args`` overrides integer arguments of a call that is to be
    refused, ``null`` names a pointer passed as NULL, ``alias`` maps an output to the input whose buffer it is passed; ``act_buf``:
    the action words as they lie in memory where envs are ``stride`` floats apart (``act`` stays what the restatement reads)."""
    torch = _torch()
    ctx = _lib.Context.get(0)
    m, E, n, O = post.shape
    A = act.shape[-1]
    ins = dict(pre=pre, post=post, actions=act if act_buf is None else act_buf, rewards=rewards, ret_in=ret_in)
    dev = {k: (None if v is None else _dev(np.ascontiguousarray(v).view(np.int32))) for k, v in ins.items()}
    tab_d = None if table is None else _dev(np.asarray(table, dtype=np.uint8))
    So, Ro = tg._Words(post.shape), tg._Words((m, E, n))
    a = dict(t=t, m=m, E=E, n=n, obs_dim=O, act_dim=A, cand_offset=cand_offset, pre_per_row=int(pre.ndim == 4),
             act_env_stride=E * n * A if stride is None else stride)
    a.update(args or {})
    ptrs = {k: _ptr(v) for k, v in dev.items()}
    ptrs.update(state_out=None if last else _ptr(So.view), ret_out=_ptr(Ro.view))
    if null:
        ptrs[null] = None
    for out, inp in (alias or {}).items():
        ptrs[out] = ptrs[inp]
    rc = ctx.lib.l2a_particle_step(ctx.handle, ptrs["pre"], a["pre_per_row"], ptrs["post"], ptrs["actions"], a["act_env_stride"],
                                   ptrs["rewards"], None if program is None else ctypes.byref(program), float(disc), ptrs["ret_in"],
                                   ptrs["state_out"], ptrs["ret_out"], _ptr(tab_d), seed, offset, a["t"], a["m"], a["E"], a["n"],
                                   a["obs_dim"], a["act_dim"], a["cand_offset"], _stream())
    torch.cuda.synchronize()
    what = "step m=%d E=%d n=%d O=%d A=%d t=%d offset=%d cand_offset=%d per_row=%d last=%d %s" % (
        m, E, n, O, A, t, offset, cand_offset, a["pre_per_row"], last, args or "")
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, ctx.lib.l2a_last_error(ctx.handle).decode())
    for k, v in ins.items():
        if v is not None:
            assert np.array_equal(dev[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), "input %s changed: %s" % (k, what)
    if expect_rc != _lib.L2A_OK:
        assert So.untouched(what) and Ro.untouched(what), "output written by a refused call: " + what
        return None
    s = So.host(what)
    r = Ro.host(what)
    if last:
        assert np.all(s == tg.FILL), "state_out is NULL, yet the buffer behind it was written: " + what
    tab = None if last else (table if table is not None else tg.lib_perm_table(seed, offset, t, m, n, E, cand_offset))
    ws, wr = ps.step(pre, post, act, ret_in, disc, tab, program=program, rewards=rewards)
    if not last:
        assert np.array_equal(s, ws), "dealt states: " + what
    assert _same_returns(r, wr), "returns: " + what
    return (None if last else s), r


# ------------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("E", [1, 2, 5, 16])
def test_step_is_bit_equal_to_the_restatement(E):
    """The whole shape grid, both modes on every shape; the pre-state form, the table's source, the last-step form, the discount
    and the seed rotate with the shape so that every value of each meets every value of the others' neighbours."""
    rs = np.random.RandomState(60 + E)
    launches, c = 0, 0
    for n in (1, 31, 32, 33, 70):
        for m in (1, 3):
            for O, A in DIMS:
                prog = every_kind(O, A)
                for t in (0, 3):
                    for co in (0, TOP - n):
                        c += 1
                        post, act = float_words(rs, (m, E, n, O)), float_words(rs, (m, E, n, A), 0.6)
                        per_row = (c + t) % 2 == 1
                        pre = float_words(rs, (m, E, n, O) if per_row else (m, E, O))
                        ret_in = None if t == 0 else float_words(rs, (m, E, n), 30.0)
                        disc = (1.0, 0.97 ** t, 0.5)[c % 3]
                        seed, offset = SEEDS[c % 2], (0, 12345, LIMIT - (t + 1) * m)[c % 3]
                        # program mode: Philox and injected tables in turn; every fourth shape in the last-step form
                        inj = tg.injected_table(rs, m, n, E) if c % 2 else None
                        run_step(pre, post, act, program=prog, ret_in=ret_in, table=inj, last=(c % 4 == 0), disc=disc, seed=seed,
                                 offset=offset, t=t, cand_offset=co)
                        # given rewards: arbitrary words (NaNs with payloads, infinities, -0, denormals); the other table source
                        S, R = tg.bit_patterns(m, E, n, O, salt=c * 7919)
                        rewards = tg.bit_patterns(m, E, n, 1, salt=c * 104729 + 1)[1]
                        inj = None if c % 2 else tg.injected_table(rs, m, n, E)
                        run_step(pre, S, act, rewards=rewards, ret_in=None if t == 0 else R, table=inj, last=(c % 4 == 2), disc=disc,
                                 seed=seed, offset=offset, t=t, cand_offset=co)
                        launches += 2
    print("[ts1 step] E=%d: %d launches, all bit-equal to the restatement" % (E, launches))


def test_step_return_input_forms():
    """``ret_in = NULL`` is the literal +0: bit-equal to a ``ret_in`` of +0 words, and different from a ``ret_in`` of -0 exactly where
    the step's discounted reward is -0 (0 + -0 = +0, -0 + -0 = -0) - as the restatement says."""
    rs = np.random.RandomState(7)
    m, E, n, O, A = 3, 5, 33, 17, 3
    pre, post, act = float_words(rs, (m, E, O)), float_words(rs, (m, E, n, O)), float_words(rs, (m, E, n, A))
    rewards = rs.randn(m, E, n).astype(np.float32)
    rewards[rs.rand(m, E, n) < 0.3] = -0.0
    rewards = rewards.view(np.uint32)
    zeros = np.zeros((m, E, n), dtype=np.uint32)
    minus = np.full((m, E, n), 0x80000000, dtype=np.uint32)
    for last in (False, True):
        null = run_step(pre, post, act, rewards=rewards, ret_in=None, last=last, seed=3, offset=9, t=0)
        zero = run_step(pre, post, act, rewards=rewards, ret_in=zeros, last=last, seed=3, offset=9, t=0)
        neg = run_step(pre, post, act, rewards=rewards, ret_in=minus, last=last, seed=3, offset=9, t=0)
        assert np.array_equal(null[1], zero[1])
        differ = null[1] != neg[1]
        assert differ.any() and np.all(neg[1][differ] == 0x80000000) and np.all(null[1][differ] == 0)
        if not last:
            assert np.array_equal(null[0], zero[0]) and np.array_equal(null[0], neg[0])
    prog = every_kind(O, A)
    a = run_step(pre, post, act, program=prog, ret_in=None, seed=3, offset=9, t=0)
    b = run_step(pre, post, act, program=prog, ret_in=zeros, seed=3, offset=9, t=0)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def test_a_poisoned_post_state_lands_in_the_block_the_table_names():
    rs = np.random.RandomState(8)
    m, E, n, O, A = 3, 5, 70, 20, 6
    prog = every_kind(O, A)
    pre = (rs.randn(m, E, n, O)).astype(np.float32)
    post, act = rs.randn(m, E, n, O).astype(np.float32), rs.uniform(-1, 1, (m, E, n, A)).astype(np.float32)
    ret_in = rs.randn(m, E, n).astype(np.float32)
    i, e, j = 1, 3, 40
    post[i, e, j, 0] = np.nan               # NORM(next[0:3]) reads it
    for table in (None, tg.injected_table(rs, m, n, E)):
        seed, offset, t = SEEDS[0], 77, 2
        s, r = run_step(pre.view(np.uint32), post.view(np.uint32), act.view(np.uint32), program=prog, ret_in=ret_in.view(np.uint32),
                        table=table, seed=seed, offset=offset, t=t, disc=0.9)
        tab = table if table is not None else tg.lib_perm_table(seed, offset, t, m, n, E)
        lands = np.minimum(tab[i, j].astype(np.int64), E - 1) == e
        assert lands.any()
        want = np.zeros((m, E, n), dtype=bool)
        want[i, lands, j] = True
        assert np.array_equal(np.isnan(r.view(np.float32)), want)
        assert np.array_equal(np.isnan(s.view(np.float32)).any(axis=3), want)
    # the last step deals nothing: the NaN return stays in its own block
    _, r = run_step(pre.view(np.uint32), post.view(np.uint32), act.view(np.uint32), program=prog, ret_in=ret_in.view(np.uint32), last=True)
    want = np.zeros((m, E, n), dtype=bool)
    want[i, e, j] = True
    assert np.array_equal(np.isnan(r.view(np.float32)), want)


def test_step_refusals_write_nothing():
    rs = np.random.RandomState(9)
    m, E, n, O, A = 2, 3, 10, 20, 6
    pre, post, act = float_words(rs, (m, E, n, O)), float_words(rs, (m, E, n, O)), float_words(rs, (m, E, n, A))
    R = float_words(rs, (m, E, n))
    prog = every_kind(O, A)
    ctx = _lib.Context.get(0)
    base = dict(program=prog, ret_in=R, expect_rc=EINVAL)
    for buf in ("pre", "post", "actions", "ret_out"):
        run_step(pre, post, act, null=buf, **base)
    run_step(pre, post, act, rewards=R, **base)                                 # both
    run_step(pre, post, act, ret_in=R, expect_rc=EINVAL)                        # neither
    bad = every_kind(O, A)
    bad.terms[1].index = O                                                      # a range outside its source vector
    run_step(pre, post, act, program=bad, ret_in=R, expect_rc=EINVAL)
    bad = every_kind(O, A)
    bad.n_terms = 17
    run_step(pre, post, act, program=bad, ret_in=R, expect_rc=EINVAL)
    run_step(pre, post, act, args=dict(obs_dim=8000), **base)                   # 64 rows of 2 * 8001 + 7 words: 4 MB
    assert "LDS" in ctx.lib.l2a_last_error(ctx.handle).decode()
    for alias in (dict(state_out="post"), dict(state_out="pre"), dict(ret_out="ret_in"), dict(ret_out="actions"), dict(state_out="ret_in"),
                  dict(ret_out="post")):
        run_step(pre, post, act, alias=alias, **base)
    run_step(pre, post, act, rewards=R, ret_in=R, alias=dict(ret_out="rewards"), expect_rc=EINVAL)
    for args in (dict(m=0), dict(E=0), dict(n=0), dict(obs_dim=0), dict(act_dim=0), dict(E=17), dict(t=-1), dict(cand_offset=-1),
                 dict(cand_offset=TOP - 9), dict(n=1 << 29), dict(m=-1), dict(act_env_stride=E * n * A - 1), dict(act_env_stride=-1)):
        run_step(pre, post, act, args=args, **base)
    run_step(pre, post, act, offset=LIMIT - 1, **base)                          # env 1's slot would be 2^33
    run_step(pre, post, act, offset=LIMIT - 2 * H, t=H, **base)
    run_step(pre, post, act, offset=(1 << 64) - 1, **base)
    run_step(pre, post, act, program=prog, ret_in=R, offset=LIMIT - 2 * H, t=H - 1)     # the last legal slot
    run_step(pre, post, act, program=prog, ret_in=R, cand_offset=TOP - 10)
    # envs further apart than one slab: the stride is honoured (the rows in between are never read)
    wide = float_words(rs, (m, 2 * E, n, A))
    run_step(pre, post, np.ascontiguousarray(wide[:, :E]), program=prog, ret_in=R, stride=2 * E * n * A, act_buf=wide, seed=5, offset=1, t=1)


# --------------------------------------------------------------------------------------------------------- 2. the plan entries
_REWARDS = {}


def reward_of(kind):
    """``(what the C entry takes, an object whose float64 ``reward`` the restatement sums, the program or None)``."""
    from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel
    if kind not in _REWARDS:
        if kind == "program":
            env = rpc.program_env("half_cheetah")
            _REWARDS[kind] = (env.reward_spec, env, env.reward_spec)
        else:
            params, norm = rmc.reward_weights(OD, AD, RM_HIDDEN), rmc.reward_norm(OD, AD)
            native = NativeRewardModel(OD, AD, RM_HIDDEN, "relu")
            native.set_weights(params)
            native.set_norm(norm)

            class _Env(object):
                reward = staticmethod(rmc.reward_fn(params, norm, "relu"))

            _REWARDS[kind] = (native, _Env(), None)
    return _REWARDS[kind]


def run_ts1(model, obs, actions, n, h, m, lam, reward, seed=0, offset=0, table=None, cand_offset=0, discount=1.0,
            expect_rc=_lib.L2A_OK, E=None, obs_d=None, act_d=None):
    """One ``l2a_plan_rs_particles_ts1_program`` / ``_reward_model``, whichever ``reward`` selects; host copies of the four outputs
    (guards checked), as ``test_particles_ts1_gpu.run_ts1``."""
    torch = _torch()
    E = model.n_sets if E is None else E
    out = dict(score=tp._Out((m, n)), spread=tp._Out((m, n)), members=tp._Out((m, E, n)), keys=tp._Out((m,), keys=True))
    obs_d = tp._up(np.asarray(obs, dtype=np.float32)) if obs_d is None else obs_d
    act_d = tp._up(np.asarray(actions, dtype=np.float32)) if act_d is None else act_d
    tab_d = None if table is None else _dev(np.asarray(table, dtype=np.uint8))
    head = (_ptr(obs_d), _ptr(act_d), m, n, h, float(discount))
    tail = (ctypes.c_float(lam), seed, offset, _ptr(tab_d), cand_offset, _ptr(out["score"].view), _ptr(out["spread"].view),
            _ptr(out["members"].view), _ptr(out["keys"].view), _stream())
    if isinstance(reward, RewardProgram):
        rc = model.lib.l2a_plan_rs_particles_ts1_program(model.handle, *(head + (ctypes.byref(reward),) + tail))
    else:
        rc = model.lib.l2a_plan_rs_particles_ts1_reward_model(model.handle, reward.handle, *(head + tail))
    torch.cuda.synchronize()
    what = "ts1 plan n=%d h=%d m=%d lambda=%g offset=%d cand_offset=%d" % (n, h, m, lam, offset, cand_offset)
    assert rc == expect_rc, "%s: return code %d (%s)" % (what, rc, model.lib.l2a_last_error(model.ctx.handle).decode())
    if expect_rc != _lib.L2A_OK:
        assert all(o.untouched(k + " " + what) for k, o in out.items()), "output written by a refused call: " + what
        return rc
    assert model.ctx.launch_status_value() == 0, what
    return {k: o.host(k + " " + what) for k, o in out.items()}


@pytest.mark.parametrize("kind", ["program", "reward_model"])
@pytest.mark.parametrize("hidden", tp.WIDTHS)
def test_identity_permutations_and_horizon_one_are_ts_infinity_bit_for_bit(hidden, kind):
    reward = reward_of(kind)[0]
    for E in (2, 3, 5):
        _, _, _, model = tp.native_model(hidden, E)
        for c, (n, h, m) in enumerate([(16, 2, 1), (50, H, 3), (50, 2, 3), (16, H, 1)]):
            obs, actions = tp.plan_inputs(800 + c, n, h, m)
            lam, co, disc = (0.0, 1.0)[c % 2], (0, 13)[c % 2], (1.0, 0.97)[c % 2]
            want = tp.run_plan(model, obs, actions, n, h, m, lam, reward, cand_offset=co, discount=disc)
            got = run_ts1(model, obs, actions, n, h, m, lam, reward, table=t1.identity_table(m, n, E, h), cand_offset=co, discount=disc)
            for k in ("members", "score", "spread", "keys"):
                assert np.array_equal(tp._bits(got[k]) if k != "keys" else got[k], tp._bits(want[k]) if k != "keys" else want[k]), \
                    "identity, %s: kind=%s hidden=%s E=%d n=%d h=%d m=%d" % (k, kind, hidden, E, n, h, m)
        n, m = 50, 3
        obs, actions = tp.plan_inputs(810, n, 1, m)
        want = tp.run_plan(model, obs, actions, n, 1, m, 1.0, reward)
        got = run_ts1(model, obs, actions, n, 1, m, 1.0, reward, seed=SEEDS[0], offset=3)
        assert tg._same(got, want), "h = 1: kind=%s hidden=%s E=%d" % (kind, hidden, E)


PHILOX_GRID = [(n, h, m, disc) for n in (16, 50) for h in (2, H) for m in (1, 3) for disc in (1.0, 0.97)]


# The seed of every grid case's inputs, picked on the CPU (where the float64 restatement runs) so that the particles left out for an
# INRANGE input near a bound stay under the cap for both widths and both ensemble sizes: 900 + c, moved on in steps of 16 where
# that seed left more than 1 % out.
INPUT_SEEDS = [900, 901, 902, 903, 904, 905, 922, 923, 908, 909, 926, 911, 912, 929, 914, 947]


def seeded_inputs(seed, n, h, m):
    """``test_particles_gpu.plan_inputs`` with the observations drawn from ``seed`` too: the fixed first row of
    ``synthetic.make_obs0`` starts 0.11 from a bound of the program's ``INRANGE`` term, and at ``m = 1``, ``h = 7`` no choice of
    actions keeps its particles away from it."""
    _, actions = tp.plan_inputs(seed, n, h, m)
    return np.random.RandomState(seed).randn(m, OD), actions


def philox_case(c, h, m):
    """Seed, offset, lambda and candidate offset of grid case ``c``, and the seed of its inputs."""
    return SEEDS[c % 2], (0, 12345, LIMIT - h * m)[c % 3], (1.0, 0.0, 4.0)[c % 3], (0, 9)[c % 2], INPUT_SEEDS[c]


@pytest.mark.parametrize("kind", ["program", "reward_model"])
@pytest.mark.parametrize("E", (2, 5))
@pytest.mark.parametrize("hidden", tp.WIDTHS[:2])
def test_philox_plans_against_the_float64_restatement(hidden, E, kind):
    reward, env64, prog = reward_of(kind)
    _, sets, norms, model = tp.native_model(hidden, E)
    worst, most_left_out = 0.0, 0.0
    for c, (n, h, m, disc) in enumerate(PHILOX_GRID):
        seed, offset, lam, co, input_seed = philox_case(c, h, m)
        obs, actions = seeded_inputs(input_seed, n, h, m)
        tables = tg.philox_tables(seed, offset, m, n, h, E, co)
        R64 = t1.particle_returns64(env64, sets, norms, obs, actions, n, tables, discount=disc)
        keep = np.ones(R64.shape, dtype=bool)
        if prog is not None:
            keep = ps.particle_margins64(prog, sets, norms, obs, actions, n, tables) >= MARGIN
        left_out = 1.0 - keep.mean()
        most_left_out = max(most_left_out, left_out)
        scale = float(np.max(np.abs(R64)))
        got = run_ts1(model, obs, actions, n, h, m, lam, reward, seed=seed, offset=offset, cand_offset=co, discount=disc)
        what = "kind=%s hidden=%s E=%d n=%d h=%d m=%d discount=%g" % (kind, hidden, E, n, h, m, disc)
        err = float(np.max(np.abs(got["members"].astype(np.float64) - R64)[keep])) / scale
        worst = max(worst, err)
        print("[ts1 rewards] %s: particle returns %.2e of max |R|, %.2f%% left out" % (what, err, 100 * left_out))
        assert left_out <= MARGIN_CAP, "%.2f%% of the particles pass within %g of an INRANGE bound: %s" % (100 * left_out, MARGIN, what)
        assert err <= BAR, "particle returns off by %.3e of max |R|: %s" % (err, what)
        again = tp.run_score(model.ctx, got["members"], lam, co)
        assert np.array_equal(tp._bits(got["score"]), tp._bits(again["score"])), "score: " + what
        assert np.array_equal(tp._bits(got["spread"]), tp._bits(again["spread"])), "spread: " + what
        assert np.array_equal(got["keys"], again["keys"]), "keys: " + what
        if c % 4 == 0:      # the same permutations injected are the same plan
            inj = run_ts1(model, obs, actions, n, h, m, lam, reward, table=tables, cand_offset=co, discount=disc)
            assert tg._same(inj, got), "injected = drawn: " + what
    print("[ts1 rewards] kind=%s hidden=%s E=%d: worst particle return %.2e of max |R|, at most %.2f%% of a case left out"
          % (kind, hidden, E, worst, 100 * most_left_out))


@pytest.mark.parametrize("kind", ["program", "reward_model"])
def test_shuffles_shards_and_divergence(kind):
    reward = reward_of(kind)[0]
    hidden, E, n, h, m = (128, 128), 3, 50, H, 3
    _, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(950, n, h, m)
    # a non-identity table must not give the TS-infinity returns
    want = tp.run_plan(model, obs, actions, n, h, m, 1.0, reward)
    table = t1.identity_table(m, n, E, h)
    table[:] = np.array([1, 2, 0], dtype=np.uint8)
    got = run_ts1(model, obs, actions, n, h, m, 1.0, reward, table=table)
    differ = tp._bits(got["members"]) != tp._bits(want["members"])
    assert differ.mean() > 0.99, "the shuffle changed %.1f%% of the returns only" % (100 * differ.mean())
    one = t1.identity_table(m, n, E, h)
    one[h - 2, 1, 7] = np.array([0, 2, 1], dtype=np.uint8)          # one candidate of one env, at the last boundary only
    got = run_ts1(model, obs, actions, n, h, m, 1.0, reward, table=one)
    differ = tp._bits(got["members"]) != tp._bits(want["members"])
    assert differ[1, 1:, 7].all() and differ.sum() == 2
    # two shards through cand_offset combine to the unsharded plan
    whole = run_ts1(model, obs, actions, n, h, m, 1.0, reward, seed=SEEDS[1], offset=77)
    a4 = actions.reshape(h, m, n, AD)
    parts = []
    for lo, hi in ((0, 23), (23, 50)):
        local = np.ascontiguousarray(a4[:, :, lo:hi]).reshape(h, m * (hi - lo), AD)
        parts.append(run_ts1(model, obs, local, hi - lo, h, m, 1.0, reward, seed=SEEDS[1], offset=77, cand_offset=lo))
    keys = np.maximum(parts[0]["keys"].view(np.uint64), parts[1]["keys"].view(np.uint64))
    assert np.array_equal(keys, whole["keys"].view(np.uint64))
    for k in ("score", "spread"):
        assert np.array_equal(tp._bits(np.concatenate([p[k] for p in parts], axis=1)), tp._bits(whole[k])), k
    assert np.array_equal(tp._bits(np.concatenate([p["members"] for p in parts], axis=2)), tp._bits(whole["members"]))
    # a diverged candidate stays in its column
    bad = actions.copy()
    bad[1, 2 * n + 31, 0] = np.nan                                  # env 2, candidate 31, from horizon step 1 on
    got = run_ts1(model, obs, bad, n, h, m, 1.0, reward, seed=SEEDS[0], offset=0)
    nan = np.isnan(got["members"])
    want = np.zeros_like(nan)
    want[2, :, 31] = True
    assert np.array_equal(nan, want), "NaN returns at %s" % (np.argwhere(nan != want)[:5],)
    assert np.isnan(got["score"][2, 31]) and np.isfinite(np.delete(got["score"][2], 31)).all() and np.isfinite(got["score"][:2]).all()
    assert _lib.key_decode(int(got["keys"][2]))[1] == 31


@pytest.mark.parametrize("kind", ["program", "reward_model"])
def test_returns_directly_behind_an_injected_table(kind):
    """The table has h - 1 boundaries and the last step reads none: ``particle_returns_out`` placed at the table's very end, in ONE
    allocation, is no overlap - the plan runs and equals the plan on buffers apart.  Returns that do reach into the table are refused
    before anything is launched."""
    torch = _torch()
    reward = reward_of(kind)[0]
    hidden, E, n, h, m = (128, 128), 3, 50, H, 3
    _, _, _, model = tp.native_model(hidden, E)
    obs, actions = tp.plan_inputs(955, n, h, m)
    table = np.stack([tg.injected_table(np.random.RandomState(t), m, n, E) for t in range(h - 1)])
    want = run_ts1(model, obs, actions, n, h, m, 1.0, reward, table=table)
    tab_bytes, ret_bytes = table.size, 4 * m * E * n
    assert tab_bytes % 4 == 0
    obs_d, act_d = tp._up(np.asarray(obs, dtype=np.float32)), tp._up(np.asarray(actions, dtype=np.float32))
    score, keys = tp._Out((m, n)), tp._Out((m,), keys=True)

    def plan(buf, ret_at):
        buf[:tab_bytes] = _dev(table.reshape(-1))
        rets = buf[ret_at:ret_at + ret_bytes]
        head = (_ptr(obs_d), _ptr(act_d), m, n, h, 1.0)
        tail = (ctypes.c_float(1.0), 0, 0, _ptr(buf), 0, _ptr(score.view), None, _ptr(rets), _ptr(keys.view), _stream())
        if isinstance(reward, RewardProgram):
            rc = model.lib.l2a_plan_rs_particles_ts1_program(model.handle, *(head + (ctypes.byref(reward),) + tail))
        else:
            rc = model.lib.l2a_plan_rs_particles_ts1_reward_model(model.handle, reward.handle, *(head + tail))
        torch.cuda.synchronize()
        return rc, buf.cpu().numpy()

    fill = 0xA5
    rc, host = plan(torch.full((tab_bytes + ret_bytes,), fill, dtype=torch.uint8, device="cuda:0"), tab_bytes)
    assert rc == _lib.L2A_OK, model.lib.l2a_last_error(model.ctx.handle).decode()
    assert np.array_equal(host[:tab_bytes], table.reshape(-1)), "the table was written"
    assert np.array_equal(host[tab_bytes:].view(np.int32).reshape(m, E, n), tp._bits(want["members"]))
    assert np.array_equal(tp._bits(score.host("score")), tp._bits(want["score"])) and np.array_equal(keys.host("keys"), want["keys"])
    # four bytes into the last boundary's table: refused with nothing launched, nothing written
    score, keys = tp._Out((m, n)), tp._Out((m,), keys=True)
    rc, host = plan(torch.full((tab_bytes + ret_bytes,), fill, dtype=torch.uint8, device="cuda:0"), tab_bytes - 4)
    assert rc == EINVAL and "overlaps perm" in model.lib.l2a_last_error(model.ctx.handle).decode()
    assert np.array_equal(host[:tab_bytes], table.reshape(-1)) and np.all(host[tab_bytes:] == fill)
    assert score.untouched("score") and keys.untouched("keys")


def test_the_wrapper_passes_its_arguments_in_order():
    """``NativeModel.particle_step`` (23 positional ctypes arguments behind it) against the restatement: every argument given a
    value that differs from its default and from its neighbours'."""
    torch = _torch()
    rs = np.random.RandomState(12)
    E, m, n = 2, 3, 33
    _, _, _, model = tp.native_model((32, 32), E)
    prog = every_kind(OD, AD)
    pre, post = float_words(rs, (m, E, OD)), float_words(rs, (m, E, n, OD))
    wide = float_words(rs, (m, 2 * E, n, AD), 0.6)                  # envs two slabs apart
    act = np.ascontiguousarray(wide[:, :E])
    ret_in = float_words(rs, (m, E, n), 30.0)
    table = tg.injected_table(rs, m, n, E)
    f32 = lambda words: _dev(words.view(np.float32))                # noqa: E731
    for mode in ("program", "rewards", "philox", "last"):
        rewards = float_words(rs, (m, E, n)) if mode == "rewards" else None
        so = torch.zeros((m, E * n, OD), dtype=torch.float32, device="cuda:0")
        ro = torch.zeros((m, E, n), dtype=torch.float32, device="cuda:0")
        tab = None if mode in ("philox", "last") else table
        model.particle_step(f32(pre), f32(post), f32(wide), ro, m, n, disc_t=0.75, rewards=None if rewards is None else f32(rewards),
                            program=None if mode == "rewards" else prog, ret_in=f32(ret_in), state_out=None if mode == "last" else so,
                            pre_per_row=False, act_env_stride=2 * E * n * AD, t=2, seed=SEEDS[1], offset=40,
                            perm=None if tab is None else _dev(tab), cand_offset=9)
        torch.cuda.synchronize()
        if mode == "philox":
            tab = tg.lib_perm_table(SEEDS[1], 40, 2, m, n, E, 9)
        ws, wr = ps.step(pre, post, act, ret_in, 0.75, None if mode == "last" else tab, program=None if mode == "rewards" else prog,
                         rewards=rewards)
        assert _same_returns(ro.cpu().numpy(), wr), mode
        if mode != "last":
            assert np.array_equal(so.cpu().numpy().view(np.uint32).reshape(m, E, n, OD), ws), mode
    with pytest.raises(_lib.L2AError, match="exactly one of rewards and program"):
        model.particle_step(f32(pre), f32(post), f32(wide), ro, m, n, pre_per_row=False, act_env_stride=2 * E * n * AD)


def test_refused_plans_write_nothing_and_grow_nothing():
    torch = _torch()
    from learning_to_adapt_amd.dynamics.native_model import NativeModel
    prog, native_rm = reward_of("program")[0], reward_of("reward_model")[0]
    obs, actions = tp.plan_inputs(700, 16, 2, 1)
    single = tp.native_model((32, 32), 1, "single")[3]
    per_block = tp.native_model((32, 32), 2, "per_block")[3]
    for reward in (prog, native_rm):
        for model in (single, per_block):
            assert run_ts1(model, obs, actions, 16, 2, 1, 1.0, reward, expect_rc=EINVAL, E=2) == EINVAL
            assert "mean ensemble" in model.lib.l2a_last_error(model.ctx.handle).decode()
        good = tp.native_model((32, 32), 2)[3]
        assert run_ts1(good, obs, actions, 16, 2, 1, float("nan"), reward, expect_rc=EINVAL) == EINVAL
        assert run_ts1(good, obs, actions, 16, 2, 1, 1.0, reward, cand_offset=-1, expect_rc=EINVAL) == EINVAL
        assert run_ts1(good, obs, actions, 16, 2, 1, 1.0, reward, offset=LIMIT - 1, expect_rc=EINVAL) == EINVAL
        run_ts1(good, obs, actions, 16, 2, 1, 1.0, reward, offset=LIMIT - 2)        # offset + h m = 2^33: the last legal plan
    bad = rpc.new_reward_program(OD, AD, 0.05)
    bad.terms[0].index = OD
    assert run_ts1(good, obs, actions, 16, 2, 1, 1.0, bad, expect_rc=EINVAL) == EINVAL
    # a model that never planned particles holds no buffer: a refused plan of 60 MB leaves the free memory where it was, the same
    # plan accepted takes it (the probe sees a growth)
    env = tp.native_model((32, 32), 2)[0]
    sets, norms = synthetic.make_members(env, (32, 32), 2)
    fresh = NativeModel(OD, AD, (32, 32), "relu", None, 2, "mean")
    for e in range(2):
        fresh.set_weights(e, sets[e])
        fresh.set_norm(e, norms[e])
    n, h, m = 100000, 2, 1
    obs_d = tp._up(np.asarray(obs, dtype=np.float32))
    act_d = torch.zeros((h, m * n, AD), dtype=torch.float32, device="cuda:0")
    run_ts1(fresh, None, None, 16, 2, 1, 1.0, prog, offset=LIMIT - 1, expect_rc=EINVAL, obs_d=obs_d, act_d=act_d)     # (warms the helpers)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    out = dict(score=torch.empty((m, n), device="cuda:0"), keys=torch.zeros((m,), dtype=torch.int64, device="cuda:0"))
    free1 = torch.cuda.mem_get_info()[0]

    def plan(offset):
        rc = fresh.lib.l2a_plan_rs_particles_ts1_program(fresh.handle, _ptr(obs_d), _ptr(act_d), m, n, h, 1.0, ctypes.byref(prog),
                                                         ctypes.c_float(0.0), 1, offset, None, 0, _ptr(out["score"]), None, None,
                                                         _ptr(out["keys"]), _stream())
        torch.cuda.synchronize()
        return rc

    states = 4 * (3 * 2 * n * OD)                   # bytes of the three state buffers alone
    assert plan(LIMIT - 1) == EINVAL
    assert free1 - torch.cuda.mem_get_info()[0] < states // 2, "a refused plan grew the model's buffer"
    assert plan(0) == _lib.L2A_OK
    grown = free1 - torch.cuda.mem_get_info()[0]
    print("[ts1 rewards] an accepted plan of %d particles grew the buffer by %.1f MB (the tensors of the test: %.1f MB)"
          % (2 * n, grown / 1e6, (free0 - free1) / 1e6))
    assert grown >= states


# ------------------------------------------------------------------------------------------------------------ 3. the controller
_PRODUCT = {}


def controller(kind, planner, hidden, E, n, h, lam, **kw):
    """An ``MPCController(ensemble_planning="particles", particle_sampling="ts1", ts1_step_rewards=True)`` on an env with a reward
    program, or with a reward model (one dynamics model per kind, width and ensemble size; the env is this module's own)."""
    from learning_to_adapt_amd.dynamics import MLPRewardModel
    case = dict(env="half_cheetah", mode="mean", hidden=hidden, E=E, n=n, h=h, planner="cem" if planner == "cem" else "rs",
                num_cem_iters=1)
    key = (kind, tuple(hidden), E)
    if key not in _PRODUCT:
        env, model = cases.product_model(case)
        rm = None
        if kind == "program":
            env.reward_spec = rpc.new_reward_program(OD, AD, env.dt)
        elif kind == "reward_model":
            rm = MLPRewardModel(name="rew", env=env, hidden_sizes=RM_HIDDEN, init_seed=0)
            rm.set_params(rmc.reward_weights(OD, AD, RM_HIDDEN))
            rm.set_normalization(rmc.reward_norm(OD, AD))
        _PRODUCT[key] = (env, model, rm)
    env, model, rm = _PRODUCT[key]
    kw = dict(dict(risk_coef=lam, particle_sampling="ts1", ts1_step_rewards=True), **kw)
    if rm is not None:
        kw.update(reward_model=rm, use_reward_model=True)
    if planner == "rs":
        kw.update(draw_ahead=False)
    elif planner == "cem":
        kw.update(rng="device", cem_mode="fixed")
    elif planner == "mppi":
        kw.update(rng="device", use_mppi=True)
    else:
        kw.update(rng="device", use_icem=True, icem_iters=1)
    return cases.product_controller(case, model=model, env=env, ensemble_planning="particles", **kw)


def record_plans(native):
    """Wraps ``native.plan_rs_particles_ts1`` so that every call leaves a copy of its inputs behind."""
    calls = []
    stock = native.plan_rs_particles_ts1

    def plan(obs0, actions, m, n, h, discount, reward, **kw):
        calls.append(dict(obs0=obs0.clone(), actions=actions.clone(), m=m, n=n, h=h, discount=discount, reward=reward,
                          seed=kw["seed"], offset=kw["offset"], cand_offset=kw["cand_offset"]))
        return stock(obs0, actions, m, n, h, discount, reward, **kw)

    native.plan_rs_particles_ts1 = plan
    return calls, stock


def test_random_shooting_on_a_program_env_picks_the_restated_argmax():
    torch = _torch()
    hidden, E, n, h, m, lam = (128, 128), 3, 50, H, 3, 1.0
    env64 = reward_of("program")[1]
    _, sets, norms, _ = tp.native_model(hidden, E)
    ctrl = controller("program", "rs", hidden, E, n, h, lam)
    native = ctrl.dynamics_model.planner_model()
    obs, actions = seeded_inputs(306, n, h, m)        # (picked like INPUT_SEEDS: none of its particles is left out)
    torch.manual_seed(4321)
    tables = tg.philox_tables(4321, 0, m, n, h, E)
    R64 = t1.particle_returns64(env64, sets, norms, obs, actions, n, tables)
    s64 = pr.score64(R64, lam)[0]
    scale = float(np.max(np.abs(R64)))
    programs0 = native.program_plans
    np.random.seed(306)
    act, _ = ctrl.get_actions(obs)
    assert native.program_plans == programs0 + 1 and ctrl._particles["ts1_offset"] == 0
    idx = ctrl.last_plan["best_index"]
    diag = ctrl.particle_diagnostics(tables=True)
    members = diag["member_returns_table"]
    keep = ps.particle_margins64(env64.reward_spec, sets, norms, obs, actions, n, tables) >= MARGIN
    err = float(np.max(np.abs(members.astype(np.float64) - R64)[keep])) / scale
    print("[ts1 rewards] controller: particle returns %.2e of max |R|, %.2f%% left out" % (err, 100 * (1 - keep.mean())))
    assert keep.all(), "seed 306 was picked so that no particle is left out: the arg-max check below reads every candidate"
    assert err <= BAR
    score = pr.score_f32(members, lam)[0]
    assert np.array_equal(idx, [pr.argmax_nan_first(row) for row in score])
    first = actions[0].reshape(m, n, AD)
    for i in range(m):
        assert s64[i, idx[i]] >= np.max(s64[i]) - 2 * (1 + lam) * BAR * scale, "env %d chose %d, no tie of the restatement's" % (i, idx[i])
        assert np.array_equal(act[i].view(np.int64), first[i, idx[i]].view(np.int64)), "action of env %d" % i


@pytest.mark.parametrize("kind,planner", [("program", "cem"), ("program", "mppi"), ("program", "icem"), ("reward_model", "rs")])
def test_planners_plan_on_the_step_reward_score(kind, planner):
    torch = _torch()
    hidden, E, n, h, m, lam = (128, 128), 3, 50, H, 3, 1.0
    ctrl = controller(kind, planner, hidden, E, n, h, lam)
    native = ctrl.dynamics_model.planner_model()
    calls, stock = record_plans(native)
    try:
        obs = synthetic.make_obs0(m, OD)
        torch.manual_seed(11)
        np.random.seed(11)
        counts0 = (native.program_plans, native.reward_model_plans)
        act, _ = ctrl.get_actions(obs)
    finally:
        native.plan_rs_particles_ts1 = stock
    assert np.isfinite(act).all() and len(calls) == 1
    counts = (native.program_plans - counts0[0], native.reward_model_plans - counts0[1])
    assert counts == ((1, 0) if kind == "program" else (0, 1))
    call = calls[0]
    assert call["seed"] == 11 and call["offset"] == ctrl._particles["ts1_offset"] == 0 and (call["m"], call["h"]) == (m, h)
    diag = ctrl.particle_diagnostics(tables=True)
    direct = run_ts1(native, None, None, call["n"], h, m, lam, call["reward"], seed=call["seed"], offset=call["offset"],
                     cand_offset=call["cand_offset"], discount=call["discount"], obs_d=call["obs0"], act_d=call["actions"])
    assert np.array_equal(tp._bits(diag["member_returns_table"]), tp._bits(direct["members"]))
    assert np.array_equal(tp._bits(diag["spread_table"]), tp._bits(direct["spread"]))
    if diag["score_table"] is not None:
        assert np.array_equal(tp._bits(diag["score_table"]), tp._bits(direct["score"]))
    idx = np.array([pr.argmax_nan_first(row) for row in direct["score"]]) + call["cand_offset"]
    assert np.array_equal(diag["index"], idx) and np.array_equal(ctrl.last_plan["best_index"], idx)
    assert np.isfinite(diag["member_returns_table"]).all()


def test_the_keyword_changes_nothing_on_a_reward_spec_env():
    hidden, E, n, h, m, lam = (128, 128), 3, 50, H, 3, 1.0
    obs, _ = tp.plan_inputs(990, n, h, m)
    tables = []
    for on in (False, True):
        ctrl = controller("spec", "rs", hidden, E, n, h, lam, ts1_step_rewards=on)
        native = ctrl.dynamics_model.planner_model()
        programs0 = native.program_plans
        _torch().manual_seed(5)
        np.random.seed(990)
        act, _ = ctrl.get_actions(obs)
        assert native.program_plans == programs0
        diag = ctrl.particle_diagnostics(tables=True)
        tables.append((act, diag["member_returns_table"], diag["spread_table"], diag["index"]))
    for a, b in zip(*tables):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
