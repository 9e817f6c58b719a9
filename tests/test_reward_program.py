"""Reward programs on the host: the C struct, the validator, the float64 / float32 evaluations and the controller's
routing.  No GPU."""

import ctypes
import os
import re

import numpy as np
import pytest

import cases
import oracle_backend
import reward_program_cases as rpc
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs import RewardProgram, RewardSpec
from learning_to_adapt_amd.envs import reward_spec as rs_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"half_cheetah": (20, 6, 0.01), "ant": (41, 8, 0.02), "arm_7dof": (23, 7, 0.02)}


def _spec(kind):
    od, ad, dt = SHAPES[kind]
    return (RewardSpec.arm_7dof(od) if kind == "arm_7dof" else getattr(RewardSpec, kind)(od, dt)), od, ad


def _rows(seed, rows, od, ad, scale):
    """fp32-representable rows of magnitude up to ``scale`` (the float32 evaluation then starts from the same numbers)."""
    rs = np.random.RandomState(seed)
    return [rs.uniform(-scale, scale, (rows, d)).astype(np.float32).astype(np.float64) for d in (od, ad, od)]


def test_structs_match_header():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    body = re.search(r"typedef struct l2a_reward_term \{(.*?)\} l2a_reward_term;", text, flags=re.S).group(1)
    fields = re.findall(r"(float|int)\s+([a-z_]+);", body)
    assert [f[1] for f in fields] == [f[0] for f in rs_mod.RewardTerm._fields_]
    assert [ctypes.c_float if f[0] == "float" else ctypes.c_int for f in fields] == [f[1] for f in rs_mod.RewardTerm._fields_]
    assert ctypes.sizeof(rs_mod.RewardTerm) == 4 * len(fields) == 32
    body = re.search(r"typedef struct l2a_reward_program \{(.*?)\} l2a_reward_program;", text, flags=re.S).group(1)
    fields = re.findall(r"(float|int|l2a_reward_term)\s+([a-z_]+)(?:\[(\w+)\])?;", body)
    assert [f[1] for f in fields] == [f[0] for f in RewardProgram._fields_]
    caps = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (L2A_PROGRAM_MAX_\w+) (\d+)", text)}
    assert caps == {"L2A_PROGRAM_MAX_TERMS": rs_mod.PROGRAM_MAX_TERMS, "L2A_PROGRAM_MAX_CONSTS": rs_mod.PROGRAM_MAX_CONSTS}
    assert [caps[f[2]] for f in fields if f[2]] == [16, 64]
    assert ctypes.sizeof(RewardProgram) == 16 + 16 * 32 + 64 * 4
    for name, value in (("SRC_OBS", 0), ("SRC_ACT", 1), ("SRC_NEXT", 2), ("SRC_DELTA", 3)):
        assert re.search(r"#define L2A_%s %d\b" % (name, value), text) and getattr(rs_mod, name) == value
    for name, value in (("TERM_LINEAR", 0), ("TERM_SQSUM", 1), ("TERM_NORM", 2), ("TERM_INRANGE", 3)):
        assert re.search(r"#define L2A_%s %d\b" % (name, value), text) and getattr(rs_mod, name) == value


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("l2a_reward_program_check", "l2a_score_trajectory", "l2a_plan_rs_program"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _check(prog, od=20, ad=6):
    return _lib.load().l2a_reward_program_check(ctypes.byref(prog), od, ad)


def test_validator_accepts_valid_programs():
    assert _check(rpc.every_kind_program(20, 6)) == 0
    assert _check(rpc.every_kind_program(17, 5), 17, 5) == 0
    assert _check(rpc.new_reward_program(41, 8, 0.02), 41, 8) == 0
    assert _check(RewardProgram()) == 0                                  # no terms: r = bias
    full = RewardProgram()
    for _ in range(16):
        full.sqsum("obs", 0, 4, 1.0, target=np.ones(4))                  # 16 terms, 64 constants: the capacities
    assert _check(full) == 0
    for kind in SHAPES:
        spec, od, ad = _spec(kind)
        assert _check(RewardProgram.from_spec(spec, od, ad), od, ad) == 0
    rpc.every_kind_program(20, 6).check(20, 6)


def _broken(**change):
    prog = RewardProgram().sqsum("obs", 2, 3, 1.0, target=[1.0, 2.0, 3.0]).linear("act", 1, 1.0)
    term = change.pop("term", 0)
    for key, value in change.items():
        if key in ("n_terms", "n_consts"):
            setattr(prog, key, value)
        else:
            setattr(prog.terms[term], key, value)
    return prog


@pytest.mark.parametrize("change,word", [
    (dict(kind=4), "kind"), (dict(kind=-1), "kind"),
    (dict(source=4), "source"), (dict(source=-1), "source"),
    (dict(index=18), "range"), (dict(index=-1), "range"), (dict(len=19), "range"), (dict(len=0), "range"),
    (dict(term=1, index=6), "range"),                                       # ACT ranges end at act_dim, not obs_dim
    (dict(term=1, len=2), "len"), (dict(kind=3), "len"),                    # LINEAR / INRANGE read one element
    (dict(target=1), "target"), (dict(target=-2), "target"), (dict(target=3), "target"), (dict(n_consts=2), "target"),
    (dict(n_terms=17), "terms"), (dict(n_terms=-1), "terms"),
    (dict(n_consts=65), "constants"), (dict(n_consts=-1), "constants"),
])
def test_validator_rejects(change, word):
    lib = _lib.load()
    assert _check(_broken()) == 0
    assert _check(_broken(**change)) == -1                                  # L2A_EINVAL
    assert word in lib.l2a_last_error(None).decode()
    with pytest.raises(ValueError):
        _broken(**change).check(20, 6)


def test_validator_rejects_null():
    assert _lib.load().l2a_reward_program_check(None, 20, 6) == -1


def test_builders_refuse_more_than_the_capacities():
    prog = RewardProgram()
    for _ in range(16):
        prog.linear("obs", 0, 1.0)
    with pytest.raises(ValueError):
        prog.linear("obs", 0, 1.0)
    prog = RewardProgram().sqsum("obs", 0, 20, 1.0, target=np.zeros(20)).sqsum("obs", 0, 20, 1.0, target=np.zeros(20)) \
        .sqsum("obs", 0, 20, 1.0, target=np.zeros(20))
    with pytest.raises(ValueError):
        prog.sqsum("obs", 0, 5, 1.0, target=np.zeros(5))


@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_from_spec_evaluates_like_the_spec(kind):
    spec, od, ad = _spec(kind)
    prog = RewardProgram.from_spec(spec, od, ad)
    obs, act, nxt = _rows(1, 500, od, ad, 10.0)
    want, got = spec.evaluate(obs, act, nxt), prog.evaluate(obs, act, nxt)
    if spec.dist_coef != 0.0:
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0.0)        # the norm term
    else:
        assert np.array_equal(got, want)


@pytest.mark.parametrize("od,ad", [(20, 6), (17, 5), (41, 8), (64, 16)])
def test_evaluate_f32_is_close_to_float64(od, ad):
    prog = rpc.every_kind_program(od, ad)
    obs, act, nxt = _rows(2, 2000, od, ad, 10.0)
    want, got = prog.evaluate(obs, act, nxt), prog.evaluate_f32(obs, act, nxt)
    assert got.dtype == np.float32
    err = np.max(np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want)))
    print("evaluate_f32 vs evaluate (obs %d, act %d): %.2e" % (od, ad, err))
    assert err < 1e-5


def test_non_finite_rows_propagate_like_numpy():
    od, ad = 20, 6
    prog = rpc.every_kind_program(od, ad)
    obs, act, nxt = _rows(3, 8, od, ad, 3.0)
    obs[1, 3] = np.nan            # LINEAR(OBS)
    nxt[2, 5] = np.nan            # INRANGE(NEXT) -> 0, the row stays finite
    act[3, 2] = np.inf            # SQSUM(ACT) -> inf * -0.05 = -inf
    nxt[4, 0] = -np.inf           # NORM(NEXT - goal) -> inf
    nxt[5, od - 2] = np.inf       # LINEAR(DELTA) -> +inf ...
    obs[5, od - 2] = np.inf       # ... inf - inf = nan
    nxt[6, 2] = np.inf
    obs[6, 2] = -np.inf           # NORM(DELTA) inf
    want = prog.evaluate(obs, act, nxt)
    got = prog.evaluate_f32(obs, act, nxt)
    assert np.isnan(want[1]) and np.isfinite(want[2]) and want[3] == -np.inf and want[4] == -np.inf and np.isnan(want[5])
    assert want[6] == -np.inf and np.isfinite(want[[0, 7]]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(want[np.isinf(want)]))
    # INRANGE on NaN gives 0: the row's reward is that of a row whose height is out of range
    out = nxt.copy()
    out[2, 5] = 100.0
    assert prog.evaluate(obs, act, out)[2] == want[2]
    # term by term: a hand-written NumPy restatement of the same program
    goal = np.array([0.5, -1.25, 2.0])
    with np.errstate(all="ignore"):
        ref = (0.5 + 0.3 * obs[:, 3] + 0.7 * (nxt[:, od - 2] - obs[:, od - 2])
               + 2.0 * ((nxt[:, 5] >= -2.0) & (nxt[:, 5] <= 3.5))
               - 0.05 * np.sum(act ** 2, axis=1) - 0.01 * np.sum(obs[:, od - 4:] ** 2, axis=1)
               - 0.1 * np.sqrt(np.sum((nxt[:, :3] - goal) ** 2, axis=1))
               - 0.2 * np.sqrt(np.sum((nxt[:, 2:4] - obs[:, 2:4]) ** 2, axis=1)))
    np.testing.assert_allclose(want, ref, rtol=1e-13, equal_nan=True)


def _program_controller(name, **kw):
    case = cases.CASES[name]
    _, model = cases.product_model(case)
    env = rpc.program_env(case["env"])
    return case, env, cases.product_controller(case, model=model, env=env, **kw)


def test_controller_is_fusable_and_plans_like_the_oracle():
    """The host logic of a controller whose env declares a program, on the oracle backend with the program as the
    reward: chosen action, index and RNG consumption are the reference planner's."""
    from oracle.planner import rollout_returns, rs_plan
    case, env, ctrl = _program_controller("hc_rs_m3_n64_h5")
    assert isinstance(ctrl._reward_spec, RewardProgram) and ctrl._fusable() and ctrl._program()
    gold = cases.load_golden("hc_rs_m3_n64_h5_s0")
    oracle_backend.install(ctrl, case)
    dyn, lib = cases.oracle_dynamics(case), _lib.load()
    calls = []

    def _rollout(observations, actions_local, n_local, cand_offset, want_returns, obs_dev=None):
        import torch
        m = len(observations)
        rets = rollout_returns(dyn, env.reward, observations, actions_local.numpy().astype(np.float64), n_local,
                               ctrl.discount).reshape(m, n_local).astype(np.float32)
        keys = np.array([max(lib.l2a_key_encode(ctypes.c_float(float(rets[i, j])), cand_offset + j) for j in range(n_local))
                         for i in range(m)], dtype=np.int64)
        calls.append(n_local)
        return torch.from_numpy(keys), (torch.from_numpy(rets) if want_returns else None)

    ctrl._rollout = _rollout
    np.random.seed(0)
    want, best, returns, _ = rs_plan(dyn, env.reward, gold["obs0"], env.action_space.low, env.action_space.high, case["n"],
                                     case["h"], case.get("discount", 1.0))
    state = np.random.get_state()
    np.random.seed(0)
    got, _ = ctrl.get_actions(gold["obs0"])
    assert calls == [case["n"]]
    assert np.array_equal(ctrl.last_plan["best_index"], best)
    np.testing.assert_array_equal(got, want)
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    # the program's reward is not the case's own: the plan differs from the golden one somewhere
    assert not np.array_equal(returns, gold["returns"])


def test_program_declines_the_l2a_reward_paths():
    case, env, ctrl = _program_controller("hc_rs_m3_n64_h5")
    assert not ctrl._can_pipeline(case["h"] + 5, case["n"]) and not ctrl._can_pipeline_cem(1, 1, case["n"])
    assert ctrl._native_rs_step(np.zeros((3, 20)), 3) is None and ctrl._native_cem_step(np.zeros((3, 20))) is None
    spec_ctrl = cases.product_controller(case)
    assert not spec_ctrl._program() and spec_ctrl._fusable()
