"""Many envs per workgroup on the GPU (tests/env_layout_cases.py; DESIGN section 7, "Env layouts"): the five kernels that walk
the flat ``m * n`` row axis in workgroups that ignore env boundaries, at every ``n`` of ``N_LAYOUT`` and every tail class of the
last workgroup.

  ``l2a_value_terminal``          at RT = 1, 2, 4, 8 (row counts sized from the device's CU count, the geometry asserted): R' bit
                                  for bit the fp32 fold of ``predict``'s values, keys the arg-max of the kernel's own R'
  ``l2a_score_trajectory``        64 rows per workgroup: returns bit for bit ``RewardProgram.returns_f32``
  ``l2a_score_trajectory_term``   ... ``TerminationProgram.returns_f32`` in both modes, with and without terminal values
  ``l2a_score_trajectory_model``  CT = 1, 2, 4, 8 candidate tiles per workgroup: returns bit for bit the fp32 sum of ``predict``
  the plan entries                ``plan_rs_program`` / ``_reward_model`` / ``_value`` / ``_term`` at (m, n) = (40, 5), (65, 1), (33, 3):
                                  the float64 oracle at the 1e-4 bar, and bit for bit the entry's own scorer on its own trajectory
  ``l2a_policy_propose``          at 40 envs: the closed-loop identity, the untouched rows, the mirror indexing

Every output starts from a sentinel between guard words, inputs are read back unchanged, and the planted rows of
``env_layout_cases.plant`` (winners on an env's first and last row, twins across workgroups and waves, an all -inf env, a NaN row, an
all-NaN env) are asserted one by one on top of ``keys == want_keys(returns)``."""

import numpy as np
import pytest
import torch

import env_layout_cases as elc
import reward_model_cases as rmc
import reward_program_cases as rpc
import termination_cases as tc
import value_model_cases as vmc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.dynamics.native_model import NativeRewardModel, NativeValueModel

pytestmark = pytest.mark.gpu

RTOL = 1e-4         # against float64, |got - want| / max(1, |want|): the bar of tests/test_gpu_parity.py
GUARD = 8
FILL = -123.5
KEY_FILL = -77
DISCOUNT = 0.9


def rel_err(got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _ctx():
    return _lib.Context.get(0)


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """Bit for bit, a NaN matching any NaN (the kernel's NaN and NumPy's may differ in sign and payload)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


class _Out(object):
    """Returns (and step counts) between guard words, keys between guard words: everything starts from a sentinel."""

    def __init__(self, m, rows, steps=False):
        self.m, self.rows = m, rows
        self.r = torch.full((GUARD + rows + GUARD,), FILL, dtype=torch.float32, device="cuda:0")
        self.k = torch.full((GUARD + m + GUARD,), KEY_FILL, dtype=torch.int64, device="cuda:0")
        self.s = torch.full((GUARD + rows + GUARD,), KEY_FILL, dtype=torch.int32, device="cuda:0") if steps else None

    @property
    def returns(self):
        return self.r[GUARD:GUARD + self.rows]

    @property
    def keys(self):
        return self.k[GUARD:GUARD + self.m]

    @property
    def steps(self):
        return self.s[GUARD:GUARD + self.rows]

    def read(self, returns=True, keys=True, steps=None):
        """Host copies; an output that was not asked for must still hold its sentinel, and the guard words always do."""
        torch.cuda.synchronize()
        r, k = self.r.cpu().numpy(), self.k.cpu().numpy()
        assert np.all(r[:GUARD] == FILL) and np.all(r[-GUARD:] == FILL) and np.all(k[:GUARD] == KEY_FILL) and np.all(k[-GUARD:] == KEY_FILL)
        r, k = r[GUARD:-GUARD], k[GUARD:-GUARD]
        if not returns:
            assert np.all(r == FILL)
        if not keys:
            assert np.all(k == KEY_FILL)
        out = [r, k.view(np.uint64)]
        if self.s is not None:
            s = self.s.cpu().numpy()
            assert np.all(s[:GUARD] == KEY_FILL) and np.all(s[-GUARD:] == KEY_FILL)
            if steps is False:
                assert np.all(s[GUARD:-GUARD] == KEY_FILL)
            out.append(s[GUARD:-GUARD])
        return out


def _unchanged(pairs):
    for dev, host in pairs:
        assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(-1), np.ascontiguousarray(host).view(np.uint32).reshape(-1))


def _offset(n, *salt):
    return elc.cand_offset_of(elc.CAND_OFFSETS[(elc.N_LAYOUT.index(n) + sum(salt)) % 3], n)


# ------------------------------------------------------------------------------------------
# 1. l2a_value_terminal at every RT
# ------------------------------------------------------------------------------------------
_VALUE = {}
H_VALUE = 3


def _value_model(hidden, act):
    key = (hidden, act)
    if key not in _VALUE:
        params = vmc.value_weights(elc.VALUE_OBS, hidden)
        norm = vmc.value_norm(elc.VALUE_OBS)
        native = NativeValueModel(elc.VALUE_OBS, hidden, act)
        native.set_weights(params)
        native.set_norm(norm)
        _VALUE[key] = (native, norm)
    return _VALUE[key]


def _value_layout(native, norm, hidden, rt, n, tail, m, rows):
    """One layout through every form of the call.  The values are ``predict``'s own (tests/test_value_model_gpu.py holds them to
    float64 and shows that a row's bits do not depend on the geometry); here every bit of the fold and every key is held."""
    W = 16 * rt
    off = _offset(n, rt, elc.TAILS.index(tail) if tail in elc.TAILS else 4)
    returns = elc.base_returns(11 * rt + n, m, n)
    planted = elc.plant(returns, W)
    states = vmc.states(500 + 3 * rt + n, rows, elc.VALUE_OBS, norm)
    for name in ("twins_wg", "twins_wave"):             # twins: one state, so that R' ties too
        if name in planted:
            e, j_lo, j_hi = planted[name]
            states[e * n + j_hi] = states[e * n + j_lo]
    if "one_nan" in planted:                            # the NaN comes from a non-finite state: the incoming return is finite
        e, j = planted["one_nan"]
        returns[e, j] = np.float32(1.5)
        states[e * n + j, (e + j) % elc.VALUE_OBS] = np.inf if e % 2 else -np.inf
    st_d, r_d = _dev(states), _dev(returns)
    values = native.predict(st_d).cpu().numpy()
    assert np.isnan(values).sum() == ("one_nan" in planted)
    want = vmc.fold_f32(returns.reshape(-1), values, DISCOUNT, H_VALUE, 1.0)

    def call(coef=1.0, in_place=False, keys=True, rets=True):
        out = _Out(m, rows)
        r_in = r_d
        if in_place:
            out.returns.copy_(r_d.reshape(-1))
            r_in = out.returns
        native.terminal(st_d, r_in, m, n, H_VALUE, DISCOUNT, value_coef=coef, cand_offset=off,
                        returns_out=out.returns if (rets or in_place) else None, best_key=out.keys if keys else None)
        return out.read(returns=rets or in_place, keys=keys)

    got, keys = call()
    assert _same(got, want), (rt, n, tail)
    table = got.reshape(m, n)
    assert np.array_equal(keys, elc.want_keys(table, off)), (rt, n, tail, np.nonzero(keys != elc.want_keys(table, off))[0][:8])
    elc.check_plants(table, keys, planted, off)
    got2, keys2 = call(in_place=True)
    assert np.array_equal(_bits(got2), _bits(got)) and np.array_equal(keys2, keys), "in place"
    _, keys3 = call(rets=False)
    assert np.array_equal(keys3, keys), "keys only"
    got4, _ = call(keys=False)
    assert np.array_equal(_bits(got4), _bits(got)), "returns only"
    # value_coef = 0: R' is R bit for bit (the NaN state is not looked at), and the keys are R's - the planted returns themselves
    got5, keys5 = call(coef=0.0)
    assert np.array_equal(_bits(got5), _bits(returns.reshape(-1)))
    assert np.array_equal(keys5, elc.want_keys(returns, off))
    flat = dict(planted)
    flat.pop("one_nan", None)
    elc.check_plants(returns, keys5, flat, off)
    _unchanged([(st_d, states), (r_d, returns)])


def _value_sweep(hidden, act, ns):
    native, norm = _value_model(hidden, act)
    cus = _cus()
    seen, count = set(), 0
    for rt in elc.RTS:
        for n in ns:
            ran = 0
            for tail, m, rows in elc.layouts(16 * rt, n, elc.value_min_rows(rt, cus)):
                g = _lib.value_model_geometry(elc.VALUE_OBS, hidden, rows, cus=cus)
                assert g["RT"] == elc.value_rt(rows, cus) and g["workgroups"] == -(-rows // (16 * g["RT"]))
                if g["RT"] != rt:       # (a small device's row-count window for rt is narrower than the search for the tail
                    continue            # class: tests/test_env_layout_cases.py shows none is lost from 256 CUs on)
                _value_layout(native, norm, hidden, rt, n, tail, m, rows)
                seen.add(rt)
                ran += 1
            assert ran >= 1, "no layout of n = %d runs RT = %d on %d CUs" % (n, rt, cus)
            count += ran
    return seen, count


@pytest.mark.parametrize("n", elc.N_LAYOUT)
def test_value_terminal_keys_and_fold_at_every_rt(n):
    seen, count = _value_sweep(elc.VALUE_HIDDEN, "relu", (n,))
    print("value terminal n = %d: %d layouts, RT %s" % (n, count, sorted(seen)))
    assert seen == {1, 2, 4, 8}


def test_value_terminal_wide_tanh_network_at_every_rt():
    """(256, 256): RT = 8 takes a 128 KiB image - above the 48 KiB a kernel gets without asking."""
    cus = _cus()
    assert _lib.value_model_geometry(elc.VALUE_OBS, elc.VALUE_WIDE, elc.value_min_rows(8, cus), cus=cus)["lds_bytes"] == 128 * 1024
    seen, count = _value_sweep(elc.VALUE_WIDE, "tanh", (5, 33))
    print("value terminal (256, 256) tanh: %d layouts, RT %s" % (count, sorted(seen)))
    assert seen == {1, 2, 4, 8}


# ------------------------------------------------------------------------------------------
# 2. l2a_score_trajectory and l2a_score_trajectory_term: 64 rows per workgroup
# ------------------------------------------------------------------------------------------
DIMS = [(20, 6), (17, 5)]
HS = [1, 3]
NAN_ELEMENT = 3         # rpc.every_kind_program: NORM(DELTA[2:4]) reads it of the step's next observation
INF_ACTION = 2          # ... and SQSUM(ACT) with a negative coefficient turns an infinite action into a -inf reward


def plant_trajectories(prog, obs0, traj, actions, n, W, discount):
    """The planted patterns made the way ``test_score_kernel_ties_nan_and_guards`` makes them - by rows' trajectories, in place:
    an env's best row is moved (swapped) to its first / last row or copied onto the twin rows; an infinite action gives -inf, a
    NaN next observation NaN.  Returns ``env_layout_cases.plant``'s record."""
    h, rows = traj.shape[0], traj.shape[1]
    m = rows // n
    planted = elc.plant(np.zeros((m, n), dtype=np.float32), W)          # which envs and rows
    base = prog.returns_f32(np.repeat(obs0, n, axis=0), traj, actions, discount).reshape(m, n)
    for name, where in planted.items():
        e = where[0]
        lo = e * n
        top = lo + int(np.argmax(base[e]))
        if name in ("twins_wg", "twins_wave"):
            best_t, best_a = traj[:, top].copy(), actions[:, top].copy()
            if top not in (lo + where[1], lo + where[2]):               # the best row itself becomes an ordinary one
                traj[:, top], actions[:, top] = traj[:, lo + where[1]], actions[:, lo + where[1]]
            for j in where[1:]:
                traj[:, lo + j], actions[:, lo + j] = best_t, best_a
        elif name in ("win_first", "win_last"):
            j = lo + where[1]
            for a in (traj, actions):
                a[:, [top, j]] = a[:, [j, top]]
        elif name == "all_ninf":
            actions[0, lo:lo + n, INF_ACTION] = np.inf
        elif name == "one_nan":
            traj[h - 1, lo + where[1], NAN_ELEMENT] = np.nan
        else:
            traj[0, lo:lo + n, NAN_ELEMENT] = np.nan
    return planted


_SCORE = {}


def _score_case(od, ad, h, n, tail, m):
    key = (od, ad, h, n, tail, m)
    if key not in _SCORE:
        prog = rpc.every_kind_program(od, ad)
        obs0, traj, actions = tc.kernel_inputs(40 + n + h, m, n, od, ad, h)
        planted = plant_trajectories(prog, obs0, traj, actions, n, 64, DISCOUNT)
        _SCORE[key] = dict(prog=prog, obs0=obs0, traj=traj, actions=actions, planted=planted,
                           dev=(_dev(obs0), _dev(traj), _dev(actions)))
    return _SCORE[key]


def _assert_many_obs0_rows(obs0, n, rows):
    """The t = 0 gather is held to something: neighbouring envs differ in EVERY element."""
    assert np.all(obs0[1:] != obs0[:-1])
    env = elc.gather_env(rows, n)
    most = max(len(set(env[lo:lo + 16])) for lo in range(0, rows, 16))
    assert most >= -(-16 // n) and (n > 1 or most == 16)                # n = 1: a tile gathers 16 different obs0 rows
    return most


@pytest.mark.parametrize("n", elc.N_LAYOUT)
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("od,ad", DIMS)
def test_score_trajectory_at_every_layout(od, ad, h, n):
    for tail, m, rows in elc.layouts(64, n, elc.min_rows_small(64)):
        c = _score_case(od, ad, h, n, tail, m)
        off = _offset(n, h, od)
        want = c["prog"].returns_f32(np.repeat(c["obs0"], n, axis=0), c["traj"], c["actions"], DISCOUNT)
        elc.check_plants(want.reshape(m, n), elc.want_keys(want.reshape(m, n), off), c["planted"], off)    # the plants took
        _assert_many_obs0_rows(c["obs0"], n, rows)
        out = _Out(m, rows)
        _ctx().score_trajectory(*c["dev"], m, n, h, DISCOUNT, c["prog"], cand_offset=off, returns_out=out.returns, best_key=out.keys)
        got, keys = out.read()
        assert _same(got, want), (n, tail, np.nonzero(_bits(got) != _bits(want))[0][:8])
        assert np.array_equal(keys, elc.want_keys(got.reshape(m, n), off)), (n, tail)
        elc.check_plants(got.reshape(m, n), keys, c["planted"], off)
        out = _Out(m, rows)
        _ctx().score_trajectory(*c["dev"], m, n, h, DISCOUNT, c["prog"], cand_offset=off, best_key=out.keys)
        assert np.array_equal(out.read(returns=False)[1], keys), "keys only"
        out = _Out(m, rows)
        _ctx().score_trajectory(*c["dev"], m, n, h, DISCOUNT, c["prog"], cand_offset=off, returns_out=out.returns)
        assert np.array_equal(_bits(out.read(keys=False)[0]), _bits(got)), "returns only"
        _unchanged(zip(c["dev"], (c["obs0"], c["traj"], c["actions"])))


def _term_score(term, c, m, n, h, off, program=None, step_rewards=None, values=None, keys=True, rets=True, steps=True):
    rows = m * n
    out = _Out(m, rows, steps=True)
    _ctx().score_trajectory_term(c["dev"][0] if program is not None else None, c["dev"][1], c["dev"][2] if program is not None else None,
                                 m, n, h, DISCOUNT, term, program=program, step_rewards=step_rewards, terminal_values=values,
                                 value_coef=0.5, cand_offset=off, returns_out=out.returns if rets else None,
                                 steps_alive_out=out.steps if steps else None, best_key=out.keys if keys else None)
    return out.read(returns=rets, keys=keys, steps=steps)


def _assert_deaths(guards, traj, steps, h):
    alive = tc.survived(guards, traj, steps)
    assert (steps == 1).any() and alive.any()                       # dead at step 0, survivors ...
    if h > 2:
        assert ((steps > 1) & (steps < h)).any()                    # ... and dead at a middle step


@pytest.mark.parametrize("n", elc.N_LAYOUT)
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("od,ad", DIMS)
def test_score_trajectory_term_with_a_program_at_every_layout(od, ad, h, n):
    guards = tc.kernel_guards(od)
    term = tc.program_of(guards, -3.5)
    for tail, m, rows in elc.layouts(64, n, elc.min_rows_small(64)):
        c = _score_case(od, ad, h, n, tail, m)
        off = _offset(n, h, od, 1)
        obs_rows = np.repeat(c["obs0"], n, axis=0)
        values = (2.0 * np.random.RandomState(n + h).randn(rows)).astype(np.float32)
        v_d = _dev(values)
        for vals, vd in ((None, None), (values, v_d)):
            want, wsteps = term.returns_f32(obs_rows, c["traj"], c["actions"], DISCOUNT, program=c["prog"], terminal_values=vals,
                                            value_coef=0.5)
            _assert_deaths(guards, c["traj"], wsteps, h)
            got, keys, steps = _term_score(term, c, m, n, h, off, program=c["prog"], values=vd)
            assert _same(got, want) and np.array_equal(steps, wsteps), (n, tail, vals is not None)
            assert np.array_equal(keys, elc.want_keys(got.reshape(m, n), off)), (n, tail, vals is not None)
        assert not np.array_equal(_bits(got), _bits(term.returns_f32(obs_rows, c["traj"], c["actions"], DISCOUNT, program=c["prog"])[0]))
        _, k2, _ = _term_score(term, c, m, n, h, off, program=c["prog"], values=v_d, rets=False, steps=False)
        assert np.array_equal(k2, keys), "keys only"
        _unchanged(list(zip(c["dev"], (c["obs0"], c["traj"], c["actions"]))) + [(v_d, values)])


@pytest.mark.parametrize("n", elc.N_LAYOUT)
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("od", [20, 17])
def test_score_trajectory_term_with_step_rewards_at_every_layout(od, h, n):
    """The planted returns go in directly: a planted row's reward of step 0 is the planted value and its later rewards are 0, its
    guarded elements are kept inside the guards (twins: one trajectory), so that its return is the value itself."""
    guards = tc.kernel_guards(od)
    term = tc.program_of(guards, -3.5)
    for tail, m, rows in elc.layouts(64, n, elc.min_rows_small(64)):
        off = _offset(n, h, od, 2)
        _, traj, _ = tc.kernel_inputs(70 + n + h, m, n, od, 1, h)
        table = elc.base_returns(5 * n + h, m, n)
        planted = elc.plant(table, 64)
        rewards = (3.0 * np.random.RandomState(n).randn(h, rows)).astype(np.float32)
        for name, where in planted.items():
            e = where[0]
            cols = [e * n + j for j in where[1:]] if name not in ("all_ninf", "all_nan") else list(range(e * n, e * n + n))
            if name in ("one_nan",):
                cols.append(e * n)                      # (the large finite row in front of the NaN)
            for r in cols:
                traj[:, r, 1] = 0.5                     # inside [-8, 8] ...
                traj[:, r, od - 4:od - 1] = 1.0         # ... and below 9: the row survives
                rewards[:, r] = 0.0
                rewards[0, r] = table.reshape(-1)[r]
        values = (2.0 * np.random.RandomState(n + h).randn(rows)).astype(np.float32)
        c = dict(dev=(None, _dev(traj), None))
        sr_d, v_d = _dev(rewards), _dev(values)
        for vals, vd in ((None, None), (values, v_d)):
            want, wsteps = term.returns_f32(None, traj, None, DISCOUNT, step_rewards=rewards, terminal_values=vals, value_coef=0.5)
            _assert_deaths(guards, traj, wsteps, h)
            got, keys, steps = _term_score(term, c, m, n, h, off, step_rewards=sr_d, values=vd)
            assert _same(got, want) and np.array_equal(steps, wsteps), (n, tail, vals is not None)
            assert np.array_equal(keys, elc.want_keys(got.reshape(m, n), off)), (n, tail, vals is not None)
            if vals is None:                            # the planted values themselves came out
                elc.check_plants(got.reshape(m, n), keys, planted, off)
        _, k2, _ = _term_score(term, c, m, n, h, off, step_rewards=sr_d, values=v_d, rets=False, steps=False)
        assert np.array_equal(k2, keys), "keys only"
        _unchanged([(c["dev"][1], traj), (sr_d, rewards), (v_d, values)])


# ------------------------------------------------------------------------------------------
# 3. l2a_score_trajectory_model across CT
# ------------------------------------------------------------------------------------------
MODEL_GEOMETRIES, MODEL_NS = elc.MODEL_GEOMETRIES, elc.MODEL_NS
MODEL_OBS, MODEL_ACT, MODEL_HIDDEN = elc.MODEL_OBS, elc.MODEL_ACT, elc.MODEL_HIDDEN
_MODEL = {}


def _reward_model():
    if not _MODEL:
        params = rmc.reward_weights(MODEL_OBS, MODEL_ACT, MODEL_HIDDEN)
        norm = rmc.reward_norm(MODEL_OBS, MODEL_ACT)
        native = NativeRewardModel(MODEL_OBS, MODEL_ACT, MODEL_HIDDEN, "tanh")
        native.set_weights(params)
        native.set_norm(norm)
        _MODEL.update(native=native, norm=norm, fn=rmc.reward_fn(params, norm, "tanh"))
    return _MODEL


def _accumulate_f32(rewards, discount):
    """``R = R + f32(disc) * r`` in fp32, ``disc`` carried in float64 by repeated multiplication."""
    R = np.zeros(rewards.shape[1], dtype=np.float32)
    disc = 1.0
    for t in range(rewards.shape[0]):
        R = R + np.float32(disc) * rewards[t]
        disc *= discount
    return R


@pytest.mark.parametrize("n", MODEL_NS)
@pytest.mark.parametrize("geo,a,h", MODEL_GEOMETRIES, ids=["g%d%d%d_h%d" % (g + (h,)) for g, _, h in MODEL_GEOMETRIES])
def test_score_trajectory_model_at_every_ct(geo, a, h, n):
    s = _reward_model()
    native = s["native"]
    info = _ctx().info()
    cus, lds = int(info["compute_units"]), int(info["lds_per_block"])
    m = elc.model_envs(a, cus, n)
    rows = m * n
    g = _lib.reward_model_geometry(MODEL_OBS, MODEL_ACT, MODEL_HIDDEN, rows, h, cus=cus, lds_per_block=lds)
    assert (g["RT"], g["CT"], g["S"]) == geo and g["workgroups"] == -(-rows // (16 * geo[1])) and g["passes"] == -(-h // geo[2])
    obs0, traj, actions = rmc.inputs(900 + 7 * n + h, m, n, MODEL_OBS, MODEL_ACT, h, s["norm"])
    _assert_many_obs0_rows(obs0, n, rows)
    dev = (_dev(obs0), _dev(traj), _dev(actions))
    off = _offset(n, h, geo[1])
    out = _Out(m, rows)
    native.score_trajectory(*dev, m, n, h, DISCOUNT, cand_offset=off, returns_out=out.returns, best_key=out.keys)
    got, keys = out.read()
    # (a) bit for bit the fp32 sum of predict's per-step rewards, taken in chunks that run CT = 1 in one pass
    chunk = 16 * cus
    state = _dev(np.repeat(obs0, n, axis=0))
    step = np.empty((h, rows), dtype=np.float32)
    for t in range(h):
        for lo in range(0, rows, chunk):
            hi = min(rows, lo + chunk)
            gg = _lib.reward_model_geometry(MODEL_OBS, MODEL_ACT, MODEL_HIDDEN, hi - lo, 1, cus=cus, lds_per_block=lds)
            assert (gg["CT"], gg["S"], gg["passes"]) == (1, 1, 1)
            step[t, lo:hi] = native.predict(state[lo:hi].contiguous(), dev[2][t, lo:hi].contiguous(), dev[1][t, lo:hi].contiguous()).cpu().numpy()
        state = dev[1][t]
    assert np.array_equal(_bits(got), _bits(_accumulate_f32(step, DISCOUNT))), (geo, n)
    # (b) the float64 restatement
    want = rmc.returns_f64(s["fn"], obs0, traj, actions, n, DISCOUNT)
    err = rel_err(got, want)
    print("reward model %s n = %d, %d envs: vs float64 %.2e" % (geo, n, m, err))
    assert np.isfinite(want).all() and err < RTOL
    # (c) keys
    assert np.array_equal(keys, elc.want_keys(got.reshape(m, n), off)), (geo, n)
    out = _Out(m, rows)
    native.score_trajectory(*dev, m, n, h, DISCOUNT, cand_offset=off, best_key=out.keys)
    assert np.array_equal(out.read(returns=False)[1], keys), "keys only"
    _unchanged(zip(dev, (obs0, traj, actions)))


# ------------------------------------------------------------------------------------------
# 4. the plan entries at many envs x few candidates
# ------------------------------------------------------------------------------------------
PLAN_PARAMS = [(model, m, n) for model in elc.PLAN_MODELS for m, n in elc.PLAN_SHAPES]
PLAN_IDS = ["%s_m%d_n%d" % p for p in PLAN_PARAMS]
_PLANS = {}
_WORST = {}


def _plan_inputs(model, m, n):
    """The oracle's side (``env_layout_cases.plan_case``) plus the product's: dynamics model, reward model, value model, programs -
    built once, never modified.  The dict serves the helpers of tests/test_value_model_gpu.py and tests/test_termination_gpu.py."""
    import cases
    from learning_to_adapt_amd.envs.reward_spec import RewardSpec, reward_spec_for_env
    key = (model, m, n)
    if key not in _PLANS:
        p = dict(elc.plan_case(model, m, n))
        case = dict(p["case"], discount=p["discount"])
        env, dyn_model = cases.product_model(case)
        od, ad = env.observation_space.shape[0], env.action_space.shape[0]
        base = cases.recipe(case)[2][0]
        r_params, r_norm = rmc.reward_weights(od, ad, (64,)), rmc.reward_norm(od, ad, base=base)
        rm = NativeRewardModel(od, ad, (64,), "relu")
        rm.set_weights(r_params)
        rm.set_norm(r_norm)
        v_params, v_norm = vmc.value_weights(od, (128, 64)), vmc.value_norm(od, base=base, value=(0.5, 20.0))
        vm = NativeValueModel(od, (128, 64), "relu")
        vm.set_weights(v_params)
        vm.set_norm(v_norm)
        prog = rpc.new_reward_program(od, ad, env.dt)
        spec = reward_spec_for_env(env)
        assert isinstance(spec, RewardSpec)
        p.update(case=case, model=dyn_model, native=dyn_model.planner_model(), gold=dict(obs0=p["obs0"]), rm=rm, vm=vm,
                 vfn=vmc.value_fn(v_params, v_norm, "relu"), dyn=cases.oracle_dynamics(case), term=tc.program_of(p["guards"], -3.5),
                 rewards=dict(spec=(spec, p["reward_fn"]), program=(prog, prog.evaluate), model=(rm, rmc.reward_fn(r_params, r_norm, "relu"))))
        _PLANS[key] = p
    return _PLANS[key]


def _note(what, err):
    _WORST[what] = max(_WORST.get(what, 0.0), err)
    print("%s at many envs against float64: %.2e (worst so far %.2e)" % (what, err, _WORST[what]))


def _both_micro(native, run):
    """``run()`` under the default micro-tile policy and with the micro-tile kernels off: the same bits."""
    first = run()
    try:
        native.ctx.set_micro(0)
        second = run()
    finally:
        native.ctx.set_micro(1)
    for a, b in zip(first, second):
        a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    return first


@pytest.mark.parametrize("kind", ["program", "model"])
@pytest.mark.parametrize("model,m,n", PLAN_PARAMS, ids=PLAN_IDS)
def test_plan_rs_program_and_reward_model_at_many_envs(model, m, n, kind):
    from oracle.planner import rollout_trace
    p = _plan_inputs(model, m, n)
    native, h, disc = p["native"], elc.PLAN_H, p["discount"]
    reward, rf = p["rewards"][kind]
    obs0_d, a_d = _dev(p["obs0"]), _dev(p["actions"])
    off = _offset(n, m)

    def run():
        out = _Out(m, m * n)
        traj = torch.full((h, m * n, native.obs_dim), float("nan"), dtype=torch.float32, device="cuda:0")
        plan = native.plan_rs_program if kind == "program" else native.plan_rs_reward_model
        plan(obs0_d, a_d, m, n, h, disc, reward, cand_offset=off, returns_out=out.returns.view(m, n), best_key=out.keys, traj_out=traj)
        assert native.ctx.launch_status_value() == 0
        return out.read() + [traj]

    rets, keys, traj = _both_micro(native, run)
    want, states = rollout_trace(p["dyn"], rf, p["obs0"], p["actions"], n, disc)
    err_r, err_s = rel_err(rets, want), rel_err(traj.cpu().numpy(), states)
    _note("plan_rs_%s" % kind, err_r)
    assert err_r < RTOL and err_s < RTOL
    # the returns ARE the entry's own scorer applied to the trajectory that was written out
    if kind == "program":
        again = reward.returns_f32(np.repeat(p["obs0"].astype(np.float32), n, axis=0), traj.cpu().numpy(), p["actions"].astype(np.float32), disc)
        assert np.array_equal(_bits(rets), _bits(again))
    else:
        out = _Out(m, m * n)
        reward.score_trajectory(obs0_d, traj, a_d, m, n, h, disc, cand_offset=off, returns_out=out.returns, best_key=out.keys)
        again, again_k = out.read()
        assert np.array_equal(_bits(rets), _bits(again)) and np.array_equal(keys, again_k)
    assert np.array_equal(keys, elc.want_keys(rets.reshape(m, n), off))
    _unchanged([(obs0_d, p["obs0"].astype(np.float32)), (a_d, p["actions"].astype(np.float32))])


@pytest.mark.parametrize("kind", ["spec", "program", "model"])
@pytest.mark.parametrize("model,m,n", PLAN_PARAMS, ids=PLAN_IDS)
def test_plan_rs_value_at_many_envs(model, m, n, kind):
    from test_value_model_gpu import _plan_value, _two_calls
    p = _plan_inputs(model, m, n)
    off = _offset(n, m, 1)
    rets, keys = _both_micro(p["native"], lambda: _plan_value(p, kind, 0.5, cand_offset=off))
    want_r, want_k, plain = _two_calls(p, kind, 0.5, cand_offset=off)
    assert np.array_equal(_bits(rets), _bits(want_r)) and np.array_equal(keys, want_k)
    assert not np.array_equal(_bits(rets), _bits(plain))                # the term is there
    assert np.array_equal(keys, elc.want_keys(rets, off))
    aug, total, _ = vmc.augmented_returns(p["dyn"], p["rewards"][kind][1], p["vfn"], p["obs0"], p["actions"], n, p["discount"], 0.5)
    err = rel_err(rets.reshape(-1), aug)
    _note("plan_rs_value", err)
    assert err < RTOL and np.std(aug - total) > 0.01
    r2, _ = _plan_value(p, kind, 0.5, cand_offset=off, keys=False)
    _, k2 = _plan_value(p, kind, 0.5, cand_offset=off, rets=False)
    assert np.array_equal(_bits(r2), _bits(rets)) and np.array_equal(k2, keys)


@pytest.mark.parametrize("kind", ["program", "model"])
@pytest.mark.parametrize("model,m,n", PLAN_PARAMS, ids=PLAN_IDS)
def test_plan_rs_term_at_many_envs(model, m, n, kind):
    from test_termination_gpu import _plan
    p = _plan_inputs(model, m, n)
    native, h, disc, rm, vm = p["native"], elc.PLAN_H, p["discount"], p["rm"], p["vm"]
    off = _offset(n, m, 2)
    tv = p["vfn"](p["trace"][-1])
    want, wsteps, ambiguous, alive = tc.plan_want(p, p["rewards"][kind][1], terminal_reward=-3.5, terminal_values=tv, value_coef=0.5)
    assert ambiguous.mean() <= 0.01 and (wsteps < h).mean() >= 0.20 and alive.mean() >= 0.20
    r, s, keys, traj = _both_micro(native, lambda: _plan(p, kind, p["term"], vm=vm, coef=0.5, cand_offset=off, traj=True))
    clear = ~ambiguous
    err = rel_err(r.reshape(-1)[clear], want[clear])
    _note("plan_rs_term", err)
    assert np.array_equal(s.reshape(-1)[clear], wsteps[clear]) and err < RTOL
    assert np.array_equal(keys, elc.want_keys(r, off))
    # the entry's own scorer on the entry's own trajectory
    obs0_d, a_d = _dev(p["obs0"]), _dev(p["actions"])
    values = vm.predict(traj[h - 1].contiguous())
    out = _Out(m, m * n, steps=True)
    kw = dict(terminal_values=values, value_coef=0.5, cand_offset=off, returns_out=out.returns, steps_alive_out=out.steps, best_key=out.keys)
    if kind == "program":
        _ctx().score_trajectory_term(obs0_d, traj, a_d, m, n, h, disc, p["term"], program=p["rewards"][kind][0], **kw)
    else:           # the per-step rewards as the entry produces them: one h = 1 scoring call, one predict over the other steps
        rewards = torch.empty((h, m * n), dtype=torch.float32, device="cuda:0")
        rm.score_trajectory(obs0_d, traj[:1], a_d[:1], m, n, 1, 1.0, returns_out=rewards[0])
        rm.predict(traj[:h - 1].reshape(-1, native.obs_dim), a_d[1:].reshape(-1, native.act_dim), traj[1:].reshape(-1, native.obs_dim),
                   out=rewards[1:].reshape(-1))
        _ctx().score_trajectory_term(None, traj, None, m, n, h, disc, p["term"], step_rewards=rewards, **kw)
    r2, k2, s2 = out.read()
    assert np.array_equal(_bits(r2), _bits(r.reshape(-1))) and np.array_equal(s2, s.reshape(-1)) and np.array_equal(k2, keys)


# ------------------------------------------------------------------------------------------
# 5. l2a_policy_propose at many envs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("n_pi", [1, 3])
def test_policy_propose_at_many_envs(n_pi, h):
    """The closed-loop identity of ``test_propose_closed_loop_identity_untouched_rows_and_oracle`` at 40 envs: a 16-row tile of the
    policy kernel gathers the states of up to 16 envs."""
    import policy_reference as pr
    from test_policy_model_gpu import N_TOTAL, _act, _env_box, _model, _oracle, _propose, _same as same_rows, _words
    s = _model("mean", 128)
    native, policy, od, ad = s["native"], s["policy"], s["od"], s["ad"]
    sigma, low, high = _env_box(s)
    m, n = 40, 5
    what = "m=%d n=%d n_pi=%d h=%d" % (m, n, n_pi, h)
    obs0 = pr.states(90 + n_pi, m, od, s["norm"])
    assert np.all(obs0[1:] != obs0[:-1])
    z = np.random.RandomState(10 * n_pi + h).randn(h, m, n_pi, ad).astype(np.float32)
    seq, mir, seq0, mir0 = _propose(s, obs0, m, n, n_pi, h, sigma, low, high, z=z)
    got = seq.cpu().numpy().reshape(h, m, n, ad)
    w_seq, w_mir = _words(seq).reshape(h, m, n, ad), _words(mir).reshape(N_TOTAL, m, h, ad)
    assert np.array_equal(w_seq[:, :, n_pi:], seq0.reshape(h, m, n, ad)[:, :, n_pi:]), what          # rows >= n_pi untouched
    assert np.array_equal(w_mir[n_pi:], mir0.reshape(N_TOTAL, m, h, ad)[n_pi:]), what
    prop = np.ascontiguousarray(got[:, :, :n_pi])
    assert np.isfinite(prop).all(), what
    assert np.array_equal(w_mir[:n_pi].transpose(2, 1, 0, 3), w_seq[:, :, :n_pi]), what               # the mirror indexing
    flat = prop.reshape(h, m * n_pi, ad)
    traj = native.rollout_traj(_dev(obs0), _dev(flat), m, n_pi, h).cpu().numpy()
    for t in range(h):
        st = np.repeat(obs0, n_pi, axis=0) if t == 0 else traj[t - 1]
        same_rows(_act(policy, st, sigma, low, high, z[t].reshape(m * n_pi, ad)), flat[t], what + " t=%d" % t)
    want, _ = pr.propose64(_oracle(s, m), s["params"], s["norm"], s["act"], obs0, n_pi, h, sigma, low, high, z)
    err = rel_err(flat, want)
    print("l2a_policy_propose at %s vs float64 closed loop: %.2e" % (what, err))
    assert err < RTOL
