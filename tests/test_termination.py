"""Termination programs without a GPU: the struct against the header, the host-only check, the fp32 restatement against the
float64 plain-loop reference, the controller's refusals, ``SyntheticEnv``'s ``done`` and the input conditions of the plan cases
that tests/test_termination_gpu.py runs against the oracle."""

import ctypes
import os
import re

import numpy as np
import pytest

import cases
import reward_program_cases as rpc
import termination_cases as tc
import termination_reference as tref
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.envs import SyntheticEnv, TerminationProgram, termination_spec_for_env
from learning_to_adapt_amd.envs import termination as term_mod
from learning_to_adapt_amd.policies import MPCController, RNNMPCController

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def test_structs_match_header():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    body = re.search(r"typedef struct l2a_guard \{(.*?)\} l2a_guard;", text, flags=re.S).group(1)
    fields = re.findall(r"(float|int)\s+([a-z_0-9]+);", body)
    assert [f[1] for f in fields] == [f[0] for f in term_mod.Guard._fields_] == ["index", "len", "lo", "hi"]
    assert [ctypes.c_float if f[0] == "float" else ctypes.c_int for f in fields] == [f[1] for f in term_mod.Guard._fields_]
    assert ctypes.sizeof(term_mod.Guard) == 16
    body = re.search(r"typedef struct l2a_termination \{(.*?)\} l2a_termination;", text, flags=re.S).group(1)
    fields = re.findall(r"(float|int|l2a_guard)\s+([a-z_0-9]+)(?:\[(\w+)\])?;", body)
    assert [f[1] for f in fields] == [f[0] for f in TerminationProgram._fields_] == \
        ["n_guards", "reserved", "terminal_reward", "reserved2", "guards"]
    kinds = {"float": ctypes.c_float, "int": ctypes.c_int}
    assert [kinds[f[0]] for f in fields[:4]] == [f[1] for f in TerminationProgram._fields_[:4]]
    assert fields[4][2] == "L2A_TERMINATION_MAX_GUARDS"
    assert int(re.search(r"#define L2A_TERMINATION_MAX_GUARDS (\d+)", text).group(1)) == term_mod.TERMINATION_MAX_GUARDS == 8
    assert ctypes.sizeof(TerminationProgram) == 16 + 8 * 16


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("l2a_termination_check", "l2a_score_trajectory_term", "l2a_plan_rs_term"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def _raw(guards, terminal_reward=0.0, n_guards=None):
    term = TerminationProgram()
    for i, (index, length, lo, hi) in enumerate(guards):
        term.guards[i] = term_mod.Guard(index, length, lo, hi)
    term.n_guards = len(guards) if n_guards is None else n_guards
    term.terminal_reward = terminal_reward
    return term


@pytest.mark.parametrize("term, word", [
    (_raw([]), "0 guards"),
    (_raw([(0, 1, 0.0, 1.0)], n_guards=9), "9 guards"),
    (_raw([(0, 1, 0.0, 1.0)], n_guards=-1), "guards"),
    (_raw([(0, 1, 0.0, 1.0)], terminal_reward=INF), "terminal_reward"),
    (_raw([(0, 1, 0.0, 1.0)], terminal_reward=float("nan")), "terminal_reward"),
    (_raw([(0, 0, 0.0, 1.0)]), "guard 0: range"),
    (_raw([(0, 1, 0.0, 1.0), (-1, 1, 0.0, 1.0)]), "guard 1: range"),
    (_raw([(20, 1, 0.0, 1.0)]), "range"),
    (_raw([(18, 3, 0.0, 1.0)]), "range"),
    (_raw([(0, 1, float("nan"), 1.0)]), "NaN"),
    (_raw([(0, 1, 0.0, float("nan"))]), "NaN"),
    (_raw([(0, 1, 1.0, 0.5)]), "lo > hi"),
])
def test_check_refuses(term, word):
    lib = _lib.load()
    assert lib.l2a_termination_check(ctypes.byref(term), 20) == _lib.L2A_EINVAL
    assert word in lib.l2a_last_error(None).decode()
    with pytest.raises(ValueError, match=re.escape(word)):
        term.check(20)


def test_check_accepts_and_null():
    lib = _lib.load()
    assert lib.l2a_termination_check(None, 20) == _lib.L2A_EINVAL and "null" in lib.l2a_last_error(None).decode()
    term = TerminationProgram(-1.5).alive_in_range(0, -INF, 2.0).alive_in_range(17, -1.0, INF, length=3).alive_in_range(3, 1.0, 1.0)
    assert term.check(20) is term and term.n_guards == 3 and term.terminal_reward == -1.5
    assert lib.l2a_termination_check(ctypes.byref(term), 19) == _lib.L2A_EINVAL          # 17 + 3 > 19
    full = TerminationProgram()
    for i in range(8):
        full.alive_in_range(i, -1.0, 1.0)
    full.check(8)
    with pytest.raises(ValueError, match="at most 8"):
        full.alive_in_range(0, -1.0, 1.0)


def test_alive_is_the_plain_loop_in_float64():
    rs = np.random.RandomState(3)
    x = rs.randn(200, 9)
    x[5, 2] = np.nan
    guards = [(2, 1, -1.0, 1.5), (4, 3, -INF, 1.0), (0, 1, -2.0, INF)]
    term = tc.program_of(guards)
    want = np.array([not tref.is_terminal(guards, row) for row in x])
    assert np.array_equal(term.alive(x), want) and not want[5] and 0 < want.sum() < len(want)


@pytest.mark.parametrize("terminal_reward", [0.0, -3.5])
@pytest.mark.parametrize("discount", [1.0, 0.9])
@pytest.mark.parametrize("shape", tc.KERNEL_SHAPES, ids=tc.KERNEL_IDS)
def test_returns_f32_follows_the_float64_reference(shape, discount, terminal_reward):
    m, n, od, ad, h = shape
    guards = tc.kernel_guards(od)
    term = tc.program_of(guards, terminal_reward)
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = tc.kernel_inputs(10 + n, m, n, od, ad, h)
    tc.keep_off_bounds(traj, guards)
    obs_rows = np.repeat(obs0, n, axis=0)
    rs = np.random.RandomState(n)
    values = rs.randn(m * n).astype(np.float32)
    given = rs.randn(h, m * n).astype(np.float32)
    for kw, rewards in ((dict(program=prog), tref.step_rewards_f64(prog.evaluate, obs_rows, traj, actions)),
                        (dict(step_rewards=given), given)):
        for tv, coef in ((None, 1.0), (values, 0.5)):
            got, steps = term.returns_f32(obs_rows, traj, actions, discount, terminal_values=tv, value_coef=coef, **kw)
            want, want_steps = tref.returns_f64(guards, terminal_reward, traj, rewards, discount, tv, coef)
            assert got.dtype == np.float32 and steps.dtype == np.int32
            assert np.array_equal(steps, want_steps)
            assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-5
    # the rows the kernel tests rely on: dead at step 0, at a middle step, at the last step, and survivors
    alive = tc.survived(guards, traj, want_steps)
    assert (want_steps == 1).any() and alive.any()
    if h > 1:
        assert ((want_steps == h) & ~alive).any()
    if h > 2:
        assert ((want_steps > 1) & (want_steps < h)).any()


def test_returns_f32_never_firing_is_the_reward_programs_own_sum():
    m, n, od, ad, h = tc.KERNEL_SHAPES[2]
    prog = rpc.every_kind_program(od, ad)
    obs0, traj, actions = tc.kernel_inputs(1, m, n, od, ad, h)
    obs_rows = np.repeat(obs0, n, axis=0)
    got, steps = tc.program_of(tc.never_guards(od), -3.5).returns_f32(obs_rows, traj, actions, 0.9, program=prog)
    want = prog.returns_f32(obs_rows, traj, actions, 0.9)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (steps == h).all()


def test_synthetic_env_done():
    env = SyntheticEnv("half_cheetah")
    assert termination_spec_for_env(env) is None
    env.reset()
    for _ in range(3):
        assert env.step(np.ones(6))[2] is False
    env.termination_spec = TerminationProgram().alive_in_range(0, -INF, INF)
    assert termination_spec_for_env(env) is env.termination_spec
    env.reset()
    nxt, _, done, _ = env.step(np.ones(6))
    assert done is False
    env.termination_spec = TerminationProgram().alive_in_range(3, nxt[3] + 1.0, INF)       # the state just reached is outside
    env.reset()
    assert env.step(np.ones(6))[2] is True


def test_constructor_errors():
    case = cases.CASES["hc_rs_m3_n64_h5"]
    env, model = cases.product_model(case)
    term = TerminationProgram().alive_in_range(0, -1.0, 1.0)
    kw = dict(name="policy", env=env, dynamics_model=model, n_candidates=case["n"], horizon=case["h"])
    with pytest.raises(_lib.L2AError, match="must be a TerminationProgram"):
        MPCController(termination=lambda obs: obs[:, 0] > 0, **kw)
    with pytest.raises(_lib.L2AError, match="range outside the observation"):
        MPCController(termination=TerminationProgram().alive_in_range(20, -1.0, 1.0), **kw)
    for key in ("native_cem_step", "native_mppi_step", "native_icem_step"):
        with pytest.raises(_lib.L2AError, match="plans through the Python loop: the C controller steps"):
            MPCController(termination=term, rng="device", use_cem=(key == "native_cem_step"), use_mppi=(key == "native_mppi_step"),
                          use_icem=(key == "native_icem_step"), **dict(kw, **{key: True}))
    ens_case = cases.CASES["hc_rs_m2_n100_h7_e2"]
    env2, ens = cases.product_model(ens_case)
    for sampling in ("tsinf", "ts1"):
        with pytest.raises(_lib.L2AError, match="not built"):
            MPCController(name="policy", env=env2, dynamics_model=ens, ensemble_planning="particles", particle_sampling=sampling,
                          termination=term)

    class Custom(SyntheticEnv):         # a reward the library does not know, and no reward model: nothing would score the plan
        def reward(self, obs, act, nxt):
            return np.zeros(len(obs))

    custom = Custom("half_cheetah")
    custom.reward_spec = None
    with pytest.raises(_lib.L2AError, match="needs a plan the library scores"):
        MPCController(name="policy", env=custom, dynamics_model=model, termination=term)
    # the recurrent planner refuses an env that terminates
    rnn_case = cases.CASES[cases.rnn_case_ids()[0].rsplit("_s", 1)[0]]
    renv, rnn_model = cases.product_rnn_model(rnn_case)
    RNNMPCController(name="policy", env=renv, dynamics_model=rnn_model)
    renv.termination_spec = term
    with pytest.raises(_lib.L2AError, match="recurrent planner scores no termination"):
        RNNMPCController(name="policy", env=renv, dynamics_model=rnn_model)
    # without a termination program nothing changes; the env's own spec is the default
    plain = MPCController(**kw)
    assert plain._termination is None and not plain._program() and plain.termination_diagnostics() is None
    with_term = MPCController(termination=term, **kw)
    assert with_term._program() and with_term._fusable()
    assert not with_term._can_pipeline(case["h"] + 5, case["n"]) and not with_term._can_pipeline_cem(1, 1, case["n"])
    env.termination_spec = term
    assert MPCController(**kw)._termination is term


@pytest.mark.parametrize("cid", tc.PLAN_CASES)
def test_plan_cases_meet_their_input_conditions(cid):
    """Checked on the oracle alone: few ambiguous rows, enough rows that terminate early, enough that survive."""
    p = tc.plan_case(cid)
    want, steps, ambiguous, alive = tc.plan_want(p, p["reward_fn"])
    h = p["case"]["h"]
    print("%s: guard %s, %.1f %% ambiguous, %.1f %% terminate before h, %.1f %% survive"
          % (cid, p["guards"], 100 * ambiguous.mean(), 100 * (steps < h).mean(), 100 * alive.mean()))
    assert ambiguous.mean() <= 0.01
    assert (steps < h).mean() >= 0.20
    assert alive.mean() >= 0.20
    assert np.isfinite(want).all()
