"""The MPPI plan step as ONE C call (``l2a_mppi_controller_create_device``, ``policies/native_mppi_step.py``) and
``MPCController(native_mppi_step=True)`` on one GPU, against the Python loop ``get_mppi_action`` under the same seed: bit for bit
(the C step enqueues the same three launches per iteration with the same Philox offsets, shift vectors and mean buffers).

Not covered here: the sharded step (``tests/test_sharded_mppi_step_gpu.py``) and timing."""

import ctypes

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from mppi_step_cases import Setup, bits, restore_context, same_step

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    c = _lib.Context.get(0)
    torch.cuda.synchronize()
    c.launch_status_value()         # (whatever an earlier test file left behind)
    restore_context(c)
    yield c
    torch.cuda.synchronize()
    c.launch_status_value()
    restore_context(c)


def _c_steps(setup, seed, steps, resets=None, reseeds=None, inject_on=None, ctx=None):
    st = setup.controller(seed)
    outs = []
    try:
        for k in range(steps):
            if reseeds and k in reseeds:
                st.reseed(reseeds[k])
            if resets and k in resets:
                st.reset(resets[k])
            if k == inject_on:
                ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
            out = setup.snapshot(st, st.step(setup.obs[k], setup.stream))
            out["stats"] = st.stats()
            outs.append(out)
        return outs
    finally:
        st.close()


@pytest.mark.parametrize("which,iters", [("mlp", 1), ("ens5", 1), ("mlp", 2)])
def test_three_consecutive_steps_equal_the_python_loop(which, iters, ctx):
    setup = Setup(which, mppi_iters=iters, mppi_kappa=0.5)
    want = setup.python_steps(1234, 3)
    got = _c_steps(setup, 1234, 3)
    assert bits(want[0]["plan"]["mppi_mean"]) != bits(want[1]["plan"]["mppi_mean"])      # (the plan moves from step to step)
    for k in range(3):
        assert got[k]["rc"] == _lib.L2A_OK and got[k]["rets"].shape == (iters, setup.m, setup.n)
        same_step(got[k], want[k], "%s, step %d" % (which, k))
        assert got[k]["stats"]["steps"] == k + 1 and got[k]["stats"]["relaunches"] == 0
    if iters == 2:
        assert bits(got[0]["rets"][0]) != bits(got[0]["rets"][1])


def test_two_consecutive_steps_over_several_passes_equal_the_python_loop(ctx):
    """h = 90 at A = 6: ``l2a_mppi_sample_k`` walks the horizon in two passes (85 + 5 steps); step 1 samples around step 0's mean
    shifted across the pass boundary, and the update refits 540 elements per env."""
    setup = Setup("long", mppi_kappa=0.5)
    assert setup.h == 90 and setup.h > 512 // 6
    want = setup.python_steps(1234, 2)
    got = _c_steps(setup, 1234, 2)
    assert bits(want[0]["plan"]["mppi_mean"]) != bits(want[1]["plan"]["mppi_mean"])
    for k in range(2):
        assert got[k]["rc"] == _lib.L2A_OK and got[k]["rets"].shape == (1, setup.m, setup.n)
        same_step(got[k], want[k], "long, step %d" % k)
        assert got[k]["stats"]["steps"] == k + 1 and got[k]["stats"]["relaunches"] == 0


def test_reset_of_one_env_between_two_steps(ctx):
    """Env 1 is reset in front of step 2 on both sides: its plan starts from zeros, the others move on one step."""
    setup = Setup("mlp")
    dones = [False, True, False]
    want = setup.python_steps(77, 3, resets={2: dones})
    got = _c_steps(setup, 77, 3, resets={2: dones})
    for k in range(3):
        same_step(got[k], want[k], "step %d" % k)
    plain = setup.python_steps(77, 3)
    assert bits(plain[2]["plan"]["mppi_mean"]) != bits(want[2]["plan"]["mppi_mean"])     # (the reset shows)


def test_reseed_between_two_steps(ctx):
    """A changed seed restarts the stream at 0 and keeps the mean, as the Python loop does when torch.initial_seed() changes."""
    setup = Setup("mlp")
    want = setup.python_steps(5, 3, reseeds={1: 6})
    got = _c_steps(setup, 5, 3, reseeds={1: 6})
    for k in range(3):
        same_step(got[k], want[k], "step %d" % k)


def test_one_flagged_launch_replays_the_step_unsplit_once(ctx):
    """The status word is set in front of step 1 (what a lost tile-split partner reports): the step is repeated unsplit from the
    same mean with the same offsets - L2A_STEP_UNSPLIT, one relaunch, the Python loop's bits - and the stream position moves by
    `iters` exactly once: step 2 equals the Python loop's step 2."""
    setup = Setup("mlp", mppi_iters=2)
    want = setup.python_steps(31, 3)
    got = _c_steps(setup, 31, 3, inject_on=1, ctx=ctx)
    assert [g["rc"] for g in got] == [_lib.L2A_OK, _lib.L2A_STEP_UNSPLIT, _lib.L2A_OK]
    assert [g["stats"]["relaunches"] for g in got] == [0, 1, 1] and got[2]["stats"]["steps"] == 3
    assert ctx.split_degraded and ctx.launch_status_value() == 0
    for k in range(3):
        same_step(got[k], want[k], "step %d" % k)


def test_create_refusals(ctx):
    setup = Setup("mlp")
    lds = ctx.info()["lds_per_block"]
    n_max = (lds - 4480) // 4                   # n * 4 + L2A_MPPI_UPDATE_STATIC_LDS <= lds_per_block
    with pytest.raises(_lib.L2AError, match="LDS"):
        setup.controller(1, n=n_max + 1)
    sigma = setup.python()._mppi_sigma_vector().astype(np.float64)
    for over, text in ((dict(sigma=np.where(np.arange(sigma.size) == 2, -0.1, sigma)), "sigma"),
                       (dict(sigma=np.where(np.arange(sigma.size) == 0, np.nan, sigma)), "sigma"),
                       (dict(sigma=np.where(np.arange(sigma.size) == 5, np.inf, sigma)), "sigma"),
                       (dict(beta=0.0), "beta"), (dict(beta=1.5), "beta"), (dict(beta=float("nan")), "beta"),
                       (dict(kappa=0.0), "kappa"), (dict(kappa=float("inf")), "kappa"), (dict(kappa=-1.0), "kappa"),
                       (dict(iters=0), "iters"), (dict(m=65), "m <= 64")):
        with pytest.raises(_lib.L2AError, match=text):
            setup.controller(1, **over)
    st = setup.controller(1, sigma=np.zeros_like(sigma), beta=1.0)          # the edges that are allowed
    st.close()


def test_state_and_argument_errors(ctx):
    setup = Setup("mlp")
    lib = ctx.lib
    st = setup.controller(9)
    try:
        with pytest.raises(_lib.L2AError, match="no step has finished"):
            st.result()
        np.copyto(st.obs, setup.obs[0])
        p = st._p
        assert lib.l2a_controller_begin(st.handle, p[0], setup.stream) == _lib.L2A_OK
        for call in (lambda: st.reset([True, False, False]), lambda: st.reset(None), lambda: st.reseed(10), lambda: st.result()):
            with pytest.raises(_lib.L2AError, match=r"\(-4\).*in flight"):      # L2A_ESTATE
                call()
        assert lib.l2a_controller_begin(st.handle, p[0], setup.stream) == _lib.L2A_ESTATE
        assert lib.l2a_controller_finish(st.handle, p[1], p[2], p[3]) == _lib.L2A_OK
        first = setup.snapshot(st, _lib.L2A_OK)
        same_step(first, setup.python_steps(9, 1)[0], "begin / finish")      # (the refused calls changed nothing)
        # the recurrent step functions on an MLP controller
        dummy = torch.zeros(8, device=setup.native.device)
        d = ctypes.c_void_p(dummy.data_ptr())
        assert lib.l2a_lstm_controller_step(st.handle, p[0], d, d, None, None, p[1], p[2], p[3], setup.stream) == _lib.L2A_EINVAL
        assert lib.l2a_lstm_controller_begin(st.handle, p[0], d, d, None, None, setup.stream) == _lib.L2A_EINVAL
        assert lib.l2a_controller_finish(st.handle, p[1], p[2], p[3]) == _lib.L2A_ESTATE      # nothing was launched
        with pytest.raises(ValueError):
            st.reset([True, False])
        assert st.stats()["steps"] == 1
    finally:
        st.close()
    # the entry points of one kind of controller refuse the other kind
    from learning_to_adapt_amd.policies.native_step import NativeStep
    rs = NativeStep(setup.native, False, setup.m, setup.n, setup.h, setup.env.action_space.low, setup.env.action_space.high, 1.0,
                    setup.python()._reward_spec, device_seed=3)
    try:
        assert lib.l2a_mppi_controller_reset(rs.handle, None) == _lib.L2A_EINVAL
        assert lib.l2a_mppi_controller_reseed(rs.handle, 1) == _lib.L2A_EINVAL
        assert lib.l2a_mppi_controller_result(rs.handle, None, None, None, None) == _lib.L2A_EINVAL
    finally:
        rs.close()


def test_mpc_controller_takes_the_c_step(ctx):
    """`MPCController(native_mppi_step=True)`: the C controller serves every step, `reset` and a changed seed reach it, and
    `last_plan` has the Python loop's keys and bits."""
    setup = Setup("ens5", mppi_iters=2)
    dones = [True] + [False] * (setup.m - 1)
    want = setup.python_steps(21, 4, resets={2: dones}, reseeds={3: 22})
    torch.manual_seed(21)
    ctrl = setup.python(native_mppi_step=True)
    try:
        for k in range(4):
            if k == 3:
                torch.manual_seed(22)
            if k == 2:
                ctrl.reset(dones=dones)
            act, info = ctrl.get_actions(setup.obs[k])
            st = ctrl._mppistep
            assert info == {} and st is not None and ctrl._mppi_side == "c" and st.shard is None
            assert st.stats()["steps"] == k + 1 and st.steps == k + 1
            assert "mppi_means" not in ctrl._bufs                           # the plan lives on the C side
            plan = ctrl.last_plan
            assert set(plan) == set(want[k]["plan"])
            assert act.dtype == np.float64 and bits(act) == bits(want[k]["act"]), k
            for key, ref in want[k]["plan"].items():
                assert plan[key].dtype == ref.dtype and plan[key].shape == ref.shape and bits(plan[key]) == bits(ref), (k, key)
        ctrl.mppi_fetch_returns = False                                     # the documented switch: the table stays on the device
        ctrl.get_actions(setup.obs[0])
        assert "returns" not in ctrl.last_plan and set(ctrl.last_plan) == set(want[0]["plan"]) - {"returns"}
        assert ctrl._mppistep.result()[3].shape == (2, setup.m, setup.n)
    finally:
        if ctrl._mppistep is not None:
            ctrl._mppistep.close()
            ctrl._mppistep = None


def test_a_reward_program_keeps_the_python_loop_and_still_plans(ctx):
    from test_reward_program_gpu import _controller as program_controller
    cid = "hc_rs_m3_n64_h5_s0"
    case, seed, env, model, ctrl = program_controller(cid, rng="device", use_mppi=True, native_mppi_step=True)
    obs = cases.load_golden(cid)["obs0"]
    torch.manual_seed(seed)
    for k in range(2):
        action, _ = ctrl.get_actions(obs)
        assert ctrl._mppistep is None and ctrl._mppi_side == "python"
        assert action.shape == (case["m"], 6) and np.isfinite(action).all()
        assert ctrl._bufs["mppi_calls"] == k + 1 and "mppi_means" in ctrl._bufs
    assert model.planner_model().program_plans == 2
    # a replaced normal hook keeps the Python loop as well
    setup = Setup("mlp")
    hooked = setup.python(native_mppi_step=True)
    hooked._mppi_normal_device = lambda shape, device: None
    hooked.get_actions(setup.obs[0])
    assert hooked._mppistep is None and hooked._mppi_side == "python"
