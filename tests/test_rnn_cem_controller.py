"""The recurrent (ReBAL) device-mode CEM controller step in one C call (``l2a_lstm_cem_controller_create_device`` +
``l2a_lstm_controller_step``; ``RNNMPCController(use_cem=True, rng="device", native_cem_step=True)``) against the Python device
path (``get_cem_action_device`` + ``_advance_hidden``): same seed, same Philox offsets - the same action, index, return, final
mean / std, every iteration's returns and the advanced hidden state, bit for bit, step after step.  And ``l2a_cem_pick_act``
against ``l2a_cem_pick``: the same launch with the winners' first actions written once more for the state advance."""

import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from learning_to_adapt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "learning_to_adapt_amd", "csrc", "_obj", "l2a_cem.o")
NEW = ("l2a_cem_pick_act", "l2a_lstm_cem_controller_create_device", "l2a_lstm_cem_controller_create_sharded_device")
L2A_EINVAL = -1
RNN_CASES = ["hc_rnn_cem_n200_h5_m2", "ant_rnn_cem_gru2_n60_h3", "ant_rnn_cem_gru2x256_n200_h4_m2"]


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_recurrent_cem_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert re.search(r"\bT %s$" % name, nm, flags=re.M), name
        assert getattr(lib, name).restype is ctypes.c_int, name
    assert len(lib.l2a_cem_pick_act.argtypes) == 13
    assert len(lib.l2a_lstm_cem_controller_create_device.argtypes) == 14
    assert len(lib.l2a_lstm_cem_controller_create_sharded_device.argtypes) == 18


def test_rnn_native_cem_step_is_the_last_parameter_and_off_by_default():
    from learning_to_adapt_amd.policies.rnn_mpc_controller import RNNMPCController
    params = inspect.signature(RNNMPCController.__init__).parameters
    assert params["native_cem_step"].default is False
    assert list(params)[-1] == "native_cem_step"


def test_pick_kernel_has_no_scratch():
    if not os.path.exists(OBJ):
        pytest.skip("library not built")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "isa_notes.sh"), OBJ, "cem_pick"], capture_output=True,
                         text=True, check=True).stdout
    line = [ln for ln in out.splitlines() if "l2a_cem_pick_k" in ln]
    assert len(line) == 1, out
    assert "private_segment_fixed_size:0" in line[0] and "vgpr_spill_count:0" in line[0], line[0]


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _flat(hidden):
    """The arrays of a hidden-state structure (LSTMStateTuple / array / list of those), in order."""
    if isinstance(hidden, (list, tuple)):
        return [a for part in hidden for a in _flat(part)]
    return [np.asarray(hidden)]


def _pair(name, cem_mode, seed):
    """(case, C controller, Python controller, the Python path's per-iteration returns) on ONE model under one torch seed."""
    import torch
    case = dict(cases.CASES[name])
    torch.manual_seed(seed)
    env, model = cases.product_rnn_model(case)
    c_ctrl = cases.product_rnn_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode, native_cem_step=True)
    py_ctrl = cases.product_rnn_controller(case, model=model, env=env, rng="device", cem_mode=cem_mode)
    tables = []
    stock = py_ctrl._rollout

    def recording_rollout(*args, **kwargs):         # (the stock rollout reuses one returns buffer: copy before the next iteration)
        best, rets = stock(*args, **kwargs)
        tables.append(rets.detach().cpu().numpy().copy())
        return best, rets

    py_ctrl._rollout = recording_rollout            # only here: a replaced `_rollout` on the C controller makes it fall back
    return case, c_ctrl, py_ctrl, tables


def _same_plan(c_ctrl, py_ctrl, a_c, a_py):
    assert a_c.dtype == np.float64 and _bits(a_c) == _bits(a_py)
    assert np.array_equal(c_ctrl.last_plan["best_index"], py_ctrl.last_plan["best_index"])
    assert _bits(np.asarray(c_ctrl.last_plan["best_return"], dtype=np.float32)) == \
        _bits(np.asarray(py_ctrl.last_plan["best_return"], dtype=np.float32))
    assert _bits(c_ctrl.last_plan["cem_mean"]) == _bits(py_ctrl.last_plan["cem_mean"])
    assert _bits(c_ctrl.last_plan["cem_std"]) == _bits(py_ctrl.last_plan["cem_std"])


def _same_hidden(c_ctrl, py_ctrl):
    got, want = _flat(c_ctrl._hidden_state), _flat(py_ctrl._hidden_state)
    assert len(got) == len(want) and len(got) >= 1
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and _bits(g) == _bits(w)


@pytest.mark.gpu
@pytest.mark.parametrize("cem_mode", ["reference", "fixed"])
@pytest.mark.parametrize("name", RNN_CASES)
def test_rnn_device_step_equals_device_path(name, cem_mode):
    case, c_ctrl, py_ctrl, tables = _pair(name, cem_mode, 17)
    obs = cases.load_golden(name + "_s0")["obs"][0]
    iters, m, n = case["num_cem_iters"], case["m"], case["n"]
    rs = np.random.RandomState(4)
    for k in range(4):
        if k == 2:
            c_ctrl.reset(dones=[True, False])
            py_ctrl.reset(dones=[True, False])
        del tables[:]
        a_c, _ = c_ctrl.get_actions(obs)
        a_py, _ = py_ctrl.get_actions(obs)
        assert c_ctrl._cemstep is not None and c_ctrl._cemstep.steps == k + 1      # the C controller served the step
        assert py_ctrl._cemstep is None
        _same_plan(c_ctrl, py_ctrl, a_c, a_py)
        assert set(c_ctrl.last_plan) >= {"best_index", "best_return", "cem_mean", "cem_std", "cem_trace"}
        trace = c_ctrl.last_plan["cem_trace"]
        assert len(trace) == iters and len(tables) == iters
        for it in range(iters):                                                     # EVERY iteration's returns
            assert trace[it]["returns"].shape == (m, n) == tables[it].shape
            assert _bits(trace[it]["returns"]) == _bits(tables[it]), (k, it)
        _same_hidden(c_ctrl, py_ctrl)
        obs = obs + 0.01 * rs.randn(*obs.shape)


@pytest.mark.gpu
def test_rnn_device_step_flagged_launch_relaunches_unsplit():
    """A launch flagged invalid (l2a_inject_status) makes the step repeat itself unsplit, the advance included, from the same state
    with the same offsets: L2A_STEP_UNSPLIT, one relaunch, and the unflagged result and state."""
    import torch
    name = "hc_rnn_cem_n200_h5_m2"
    case, c_ctrl, py_ctrl, _ = _pair(name, "reference", 23)
    obs = cases.load_golden(name + "_s0")["obs"][0]
    native = c_ctrl.dynamics_model.planner_model()
    ctx = native.ctx
    try:
        a_c, _ = c_ctrl.get_actions(obs)
        a_py, _ = py_ctrl.get_actions(obs)
        _same_plan(c_ctrl, py_ctrl, a_c, a_py)
        _same_hidden(c_ctrl, py_ctrl)
        st = c_ctrl._cemstep
        state, (c1, h1) = c_ctrl._native_step_state(native, case["m"])
        ctx.check(ctx.lib.l2a_inject_status(ctx.handle, 1), "l2a_inject_status")
        stream = torch.cuda.current_stream(c_ctrl._device()).cuda_stream
        rc = st.step(obs, stream, state)
        assert rc == _lib.L2A_STEP_UNSPLIT
        stats = (ctypes.c_double * 16)()
        ctx.check(ctx.lib.l2a_controller_stats(st.handle, stats, 16), "l2a_controller_stats")
        assert int(stats[8]) == 1                       # one relaunch
        mean, std, _ = st.result(with_returns=False)
        a_py, _ = py_ctrl.get_actions(obs)
        assert _bits(st.act) == _bits(a_py)
        assert np.array_equal(st.idx, py_ctrl.last_plan["best_index"])
        assert _bits(mean) == _bits(py_ctrl.last_plan["cem_mean"])
        assert _bits(std) == _bits(py_ctrl.last_plan["cem_std"])
        torch.cuda.synchronize()
        c_py, h_py = py_ctrl._hid_dev
        assert _bits(c1.cpu().numpy()) == _bits(c_py.cpu().numpy())
        assert _bits(h1.cpu().numpy()) == _bits(h_py.cpu().numpy())
    finally:
        ctx.set_split(1)
        ctx.split_degraded = False


@pytest.mark.gpu
def test_rnn_device_step_falls_back_when_the_normals_are_injected():
    """A test hook that replaces the device normals keeps the Python path (the C controller draws its own)."""
    import torch
    name = "ant_rnn_cem_gru2_n60_h3"
    case, c_ctrl, _, _ = _pair(name, "fixed", 5)
    obs = cases.load_golden(name + "_s0")["obs"][0]
    n, m, D = case["n"], case["m"], case["h"] * 8
    zs = iter([np.random.RandomState(i).normal(size=(n, m, D)) for i in range(case["num_cem_iters"])])
    c_ctrl._cem_normal_device = lambda shape, device: torch.from_numpy(next(zs).astype(np.float32)).to(device)
    a, _ = c_ctrl.get_actions(obs)
    assert c_ctrl._cemstep is None and c_ctrl._hid_next is None and a.shape == (m, 8)
    assert all(np.isfinite(x).all() for x in _flat(c_ctrl._hidden_state))


def _direct(ctrl, case, seed):
    """A NativeCemStep built the way `_native_cem_step` builds it, on the controller's planner model."""
    from learning_to_adapt_amd.policies.native_cem_step import NativeCemStep
    native = ctrl.dynamics_model.planner_model()
    n = case["n"]
    return NativeCemStep(native, case["m"], n, case["h"], ctrl.action_space.low, ctrl.action_space.high, ctrl.discount,
                         ctrl._reward_spec, case["num_cem_iters"], max(int(n * ctrl.percent_elites), 1), ctrl.alpha,
                         ctrl.cem_mode == "reference", seed)


@pytest.mark.gpu
def test_recurrent_cem_controller_refuses_the_mlp_entry_points_and_half_a_next_state():
    """l2a_controller_step / _begin on a recurrent CEM controller and c_next without h_next are L2A_EINVAL with nothing launched or
    consumed - the next valid step is the Python path's first - and a plan-only step returns the advancing step's action."""
    import torch
    name = "ant_rnn_cem_gru2_n60_h3"
    seed = 31
    case, _, py_ctrl, _ = _pair(name, "reference", seed)
    obs = cases.load_golden(name + "_s0")["obs"][0]
    native = py_ctrl.dynamics_model.planner_model()
    lib, dev, m = native.lib, native.device, case["m"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    a_py, _ = py_ctrl.get_actions(obs)               # (zero state: `get_actions` resets every env first)
    c_py, h_py = py_ctrl._hid_dev
    c0 = torch.zeros((m, native.units), dtype=torch.float32, device=dev)
    h0 = torch.zeros_like(c0)
    c1, h1 = torch.full_like(c0, 7.0), torch.full_like(c0, 7.0)
    st, plan_only = _direct(py_ctrl, case, seed), _direct(py_ctrl, case, seed)
    try:
        np.copyto(st.obs, obs)
        p = st._p
        assert lib.l2a_controller_step(st.handle, p[0], p[1], p[2], p[3], stream) == L2A_EINVAL
        assert lib.l2a_controller_begin(st.handle, p[0], stream) == L2A_EINVAL
        assert lib.l2a_lstm_controller_step(st.handle, p[0], c0.data_ptr(), h0.data_ptr(), c1.data_ptr(), None, p[1], p[2], p[3],
                                            stream) == L2A_EINVAL
        assert lib.l2a_lstm_controller_step(st.handle, p[0], c0.data_ptr(), h0.data_ptr(), None, h1.data_ptr(), p[1], p[2], p[3],
                                            stream) == L2A_EINVAL
        assert lib.l2a_lstm_controller_step(st.handle, p[0], c0.data_ptr(), h0.data_ptr(), c0.data_ptr(), h1.data_ptr(), p[1], p[2],
                                            p[3], stream) == L2A_EINVAL      # an output that aliases the state
        torch.cuda.synchronize()
        assert float(c1.min()) == 7.0 and float(h1.min()) == 7.0            # nothing was launched
        assert st.stats()["steps"] == 0
        assert st.step(obs, stream, (c0.data_ptr(), h0.data_ptr(), c1.data_ptr(), h1.data_ptr())) == _lib.L2A_OK
        mean, std, _ = st.result(with_returns=False)
        assert _bits(st.act) == _bits(a_py) and np.array_equal(st.idx, py_ctrl.last_plan["best_index"])
        assert _bits(mean) == _bits(py_ctrl.last_plan["cem_mean"]) and _bits(std) == _bits(py_ctrl.last_plan["cem_std"])
        torch.cuda.synchronize()
        assert _bits(c1.cpu().numpy()) == _bits(c_py.cpu().numpy()) and _bits(h1.cpu().numpy()) == _bits(h_py.cpu().numpy())
        assert plan_only.step(obs, stream, (c0.data_ptr(), h0.data_ptr(), None, None)) == _lib.L2A_OK
        assert _bits(plan_only.act) == _bits(st.act) and np.array_equal(plan_only.idx, st.idx)
        assert _bits(plan_only.ret) == _bits(st.ret)
    finally:
        st.close()
        plan_only.close()


@pytest.mark.gpu
def test_mlp_cem_controller_refuses_the_recurrent_entry_points():
    """l2a_lstm_controller_step / _begin on an MLP CEM controller: L2A_EINVAL, the stream position has not moved."""
    import torch
    name = "hc_cem_m2_n100_h4"
    seed = 37
    case = dict(cases.CASES[name])
    torch.manual_seed(seed)
    py_ctrl = cases.product_controller(case, rng="device", cem_mode="reference")
    obs = cases.load_golden(name + "_s0")["obs0"]
    native = py_ctrl.dynamics_model.planner_model()
    lib, dev = native.lib, native.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    a_py, _ = py_ctrl.get_actions(obs)
    z = [torch.zeros((case["m"], 64), dtype=torch.float32, device=dev) for _ in range(4)]
    st = _direct(py_ctrl, case, seed)
    try:
        np.copyto(st.obs, obs)
        p = st._p
        ptr = [t.data_ptr() for t in z]
        assert lib.l2a_lstm_controller_step(st.handle, p[0], ptr[0], ptr[1], ptr[2], ptr[3], p[1], p[2], p[3], stream) == L2A_EINVAL
        assert lib.l2a_lstm_controller_begin(st.handle, p[0], ptr[0], ptr[1], ptr[2], ptr[3], stream) == L2A_EINVAL
        assert st.stats()["steps"] == 0
        assert st.step(obs, stream) == _lib.L2A_OK
        mean, std, _ = st.result(with_returns=False)
        assert _bits(st.act) == _bits(a_py) and np.array_equal(st.idx, py_ctrl.last_plan["best_index"])
        assert _bits(mean) == _bits(py_ctrl.last_plan["cem_mean"]) and _bits(std) == _bits(py_ctrl.last_plan["cem_std"])
    finally:
        st.close()


@pytest.mark.gpu
@pytest.mark.parametrize("reference", [1, 0])
@pytest.mark.parametrize("m,n,D,act_dim", [(1, 7, 6, 6), (3, 300, 12, 6), (2, 64, 24, 8)])
def test_pick_act_equals_pick(m, n, D, act_dim, reference):
    """`l2a_cem_pick_act`: `out` is `l2a_cem_pick`'s bit for bit, `act_out[i]` holds the bits of `out[i, :act_dim]` - with a row of
    NaN returns (index 0), a row of -inf returns (index 0) and an exact tie (the first maximum)."""
    import torch
    from learning_to_adapt_amd.dynamics.native_model import _ptr, _stream_ptr
    ctx = _lib.Context.get(0)
    lib, dev = ctx.lib, torch.device("cuda", 0)
    rs = np.random.RandomState(1000 * m + n + reference)
    returns = (rs.randn(m, n) * 10).astype(np.float32)
    returns[0, n // 2] = returns[0, 1] = returns[0].max() + np.float32(1.0)         # a tie: candidate 1 wins
    if m > 1:
        returns[1, :] = np.nan
    if m > 2:
        returns[2, :] = -np.inf
    cand = rs.randn(n * m, D).astype(np.float32)
    mean, std = rs.randn(m, D).astype(np.float32), rs.rand(m, D).astype(np.float32)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    r_d, c_d, mean_d, std_d = up(returns), up(cand), up(mean), up(std)
    W = act_dim + 2
    words = m * W + 2 * m * D
    out_a = torch.full((words,), -3.0, dtype=torch.float32, device=dev)
    out_b = torch.full((words,), -4.0, dtype=torch.float32, device=dev)
    act = torch.full((m + 1, act_dim), -5.0, dtype=torch.float32, device=dev)     # (one guard row behind the output)
    s = _stream_ptr(dev)
    ctx.check(lib.l2a_cem_pick(ctx.handle, _ptr(r_d), _ptr(c_d), _ptr(mean_d), _ptr(std_d), n, m, D, act_dim, reference, _ptr(out_a), s),
              "l2a_cem_pick")
    ctx.check(lib.l2a_cem_pick_act(ctx.handle, _ptr(r_d), _ptr(c_d), _ptr(mean_d), _ptr(std_d), n, m, D, act_dim, reference,
                                   _ptr(out_b), _ptr(act), s), "l2a_cem_pick_act")
    assert lib.l2a_cem_pick_act(ctx.handle, _ptr(r_d), _ptr(c_d), _ptr(mean_d), _ptr(std_d), n, m, D, act_dim, reference,
                                _ptr(out_b), None, s) == L2A_EINVAL
    torch.cuda.synchronize()
    a, b, act_h = out_a.cpu().numpy(), out_b.cpu().numpy(), act.cpu().numpy()
    assert _bits(a) == _bits(b)
    head = b[:m * W].reshape(m, W)
    assert _bits(act_h[:m]) == _bits(head[:, :act_dim])
    assert (act_h[m] == -5.0).all()
    idx = head[:, act_dim + 1].copy().view(np.int32)
    want = [1] + [0] * (m - 1) if m <= 3 else None
    assert idx.tolist() == want
    for i in range(m):                                                              # the rows the two readings name
        row = i * n + idx[i] if reference else idx[i] * m + i
        assert _bits(act_h[i]) == _bits(cand[row, :act_dim])
