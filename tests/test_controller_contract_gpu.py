"""What the 12 ``l2a_*controller_create*`` entry points, ``l2a_controller_destroy`` and ``l2a_controller_stats`` promise beside
the numbers the other files pin: which arguments are refused with which code and text (nothing is launched), that a controller
destroyed between ``begin`` and ``finish`` leaves the context's in-flight counters at zero, and where the stats slots are.

The MLP entry points run on ``hc_rs_m2_n100_h7_e2``, the recurrent ones on ``hc_rnn_rs_m2_n64_h4_reset``, the CEM ones on
``hc_cem_m2_n100_h4`` (the recurrent CEM entry points: the recurrent case's model and shape with that case's CEM parameters)."""

import ctypes

import numpy as np
import pytest
import torch

import cases
from learning_to_adapt_amd import _lib
from learning_to_adapt_amd.policies.native_cem_step import NativeCemStep
from learning_to_adapt_amd.policies.native_step import NativeStep
from learning_to_adapt_amd.utils import fast_rng

pytestmark = pytest.mark.gpu

L2A_EINVAL, L2A_ESTATE = -1, -4
SHAPE_TEXT = "needs 1 <= m <= 64 envs (at most 4096 observation floats), n >= 1, h >= 1"
CEM_TEXT = "needs iters >= 1 and 1 <= num_elites <= n"

# entry point -> (model family, "parity" | "device" | "cem", sharded)
ENTRY_POINTS = {
    "l2a_controller_create": ("mlp", "parity", False),
    "l2a_controller_create_device": ("mlp", "device", False),
    "l2a_controller_create_sharded": ("mlp", "parity", True),
    "l2a_controller_create_sharded_device": ("mlp", "device", True),
    "l2a_lstm_controller_create": ("rnn", "parity", False),
    "l2a_lstm_controller_create_device": ("rnn", "device", False),
    "l2a_lstm_controller_create_sharded": ("rnn", "parity", True),
    "l2a_lstm_controller_create_sharded_device": ("rnn", "device", True),
    "l2a_cem_controller_create_device": ("cem", "cem", False),
    "l2a_cem_controller_create_sharded_device": ("cem", "cem", True),
    "l2a_lstm_cem_controller_create_device": ("rnn", "cem", False),
    "l2a_lstm_cem_controller_create_sharded_device": ("rnn", "cem", True),
}


class _Family(object):
    """One case's model on the process's context, with what a create call takes beside the shape."""

    def __init__(self, name, recurrent=False, **ctrl_kw):
        self.case = dict(cases.CASES[name])
        self.case.pop("reset_after", None)
        if recurrent:
            self.env, self.model = cases.product_rnn_model(self.case)
            self.ctrl = cases.product_rnn_controller(self.case, model=self.model, env=self.env)
        else:
            self.env, self.model = cases.product_model(self.case)
            self.ctrl = cases.product_controller(self.case, model=self.model, env=self.env, **ctrl_kw)
        self.native = self.model.planner_model()
        self.m, self.n, self.h = self.case["m"], self.case["n"], self.case["h"]
        self.low = np.ascontiguousarray(self.env.action_space.low, dtype=np.float64)
        self.high = np.ascontiguousarray(self.env.action_space.high, dtype=np.float64)
        self.reward = self.ctrl._reward_spec
        self.stream = torch.cuda.current_stream(self.native.device).cuda_stream


@pytest.fixture(scope="module")
def families():
    return dict(mlp=_Family("hc_rs_m2_n100_h7_e2"), rnn=_Family("hc_rnn_rs_m2_n64_h4_reset", recurrent=True),
                cem=_Family("hc_cem_m2_n100_h4", rng="device", cem_mode="reference"))


@pytest.fixture
def split_off():
    ctx = _lib.Context.get(0)
    torch.cuda.synchronize()
    ctx.launch_status_value()
    ctx.set_split(0)
    yield ctx
    torch.cuda.synchronize()
    ctx.launch_status_value()
    ctx.set_split(1)
    ctx.split_degraded = False


# ---- 1. the refusal table ------------------------------------------------------------------------------------------------------------
def _create(lib, name, fam, cem, keep, **fault):
    """Calls entry point `name` with one argument replaced; returns (return code, handle)."""
    _, rng, sharded = ENTRY_POINTS[name]
    v = dict(model=fam.native.handle, m=fam.m, n=fam.n, h=fam.h, rank=0, world=2, iters=cem.case["num_cem_iters"],
             num_elites=max(int(fam.n * cem.ctrl.percent_elites), 1))
    v.update(fault)
    handle = ctypes.c_void_p()
    args = [v["model"], v["m"], v["n"], v["h"], fam.low.ctypes.data, fam.high.ctypes.data, 1.0, ctypes.byref(fam.reward)]
    if rng == "parity":
        args += [fast_rng._global_addr(), fast_rng.threads()]
    elif rng == "device":
        args += [ctypes.c_ulonglong(7)]
    else:
        args += [v["iters"], v["num_elites"], float(cem.ctrl.alpha), 1, ctypes.c_ulonglong(7)]
    if sharded:
        reduce = lib.REDUCE_FN(lambda arg, ptr, words, stream: 0)        # (never called: nothing is launched)
        keep.append(reduce)
        args += [v["rank"], v["world"], None if fault.get("no_reduce") else ctypes.cast(reduce, ctypes.c_void_p), None]
    args.append(None if fault.get("null_out") else ctypes.byref(handle))
    return getattr(lib, name)(*args), handle


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_create_refuses_one_bad_argument_at_a_time(name, families):
    family, rng, sharded = ENTRY_POINTS[name]
    fam, cem = families[family], families["cem"]
    ctx, lib = fam.native.ctx, fam.native.lib
    assert getattr(ctx, "native_comm", None) is None                     # (no communicator: a sharded create needs `reduce`)
    faults = [(dict(null_out=True), L2A_EINVAL, "out is null")]
    faults += [(f, L2A_EINVAL, SHAPE_TEXT) for f in (dict(m=0), dict(m=65), dict(n=0), dict(h=0))]
    if sharded:
        faults += [(dict(rank=2, world=2), L2A_EINVAL, "bad rank / world"),
                   (dict(no_reduce=True), L2A_ESTATE, "no reduce function and no communicator")]
    if rng == "cem":
        faults += [(dict(num_elites=fam.n + 1), L2A_EINVAL, CEM_TEXT), (dict(iters=0), L2A_EINVAL, CEM_TEXT)]
    keep = []
    for fault, code, text in faults:
        rc, handle = _create(lib, name, fam, cem, keep, **fault)
        error = lib.l2a_last_error(ctx.handle).decode()
        assert rc == code and text in error and not handle.value, (name, fault, rc, error)
    # a null model is refused before any context is known: the context's error text stays what the last refusal left
    before = lib.l2a_last_error(ctx.handle).decode()
    rc, handle = _create(lib, name, fam, cem, keep, model=None)
    assert rc == L2A_EINVAL and not handle.value and lib.l2a_last_error(ctx.handle).decode() == before
    # ... and the same arguments without a fault build a controller (the table above refused for the reason it names)
    rc, handle = _create(lib, name, fam, cem, keep)
    assert rc == _lib.L2A_OK and handle.value, (name, lib.l2a_last_error(ctx.handle).decode())
    lib.l2a_controller_destroy(handle)


# ---- 2. destroy with a step in flight ------------------------------------------------------------------------------------------------
def _cem_step(fam, seed):
    return NativeCemStep(fam.native, fam.m, fam.n, fam.h, fam.low, fam.high, 1.0, fam.reward, fam.case["num_cem_iters"],
                         max(int(fam.n * fam.ctrl.percent_elites), 1), fam.ctrl.alpha, True, seed)


def _snapshot(st):
    mean, std, rets = st.result()
    return [np.ascontiguousarray(a).tobytes() for a in (st.act, st.idx, st.ret, mean, std, rets)]


@pytest.fixture(scope="module")
def untouched_step():
    """The CEM step of `hc_cem_m2_n100_h4` (seed 21, tile split off) on a context of its own, which sees no other controller."""
    main = _lib.Context.get(0)
    try:
        _lib.Context._by_device[0] = _lib.Context(0)
        fam = _Family("hc_cem_m2_n100_h4", rng="device", cem_mode="reference")
    finally:
        _lib.Context._by_device[0] = main
    assert fam.native.ctx is not main and fam.native.ctx.handle.value != main.handle.value
    fam.native.ctx.set_split(0)
    st = _cem_step(fam, 21)
    try:
        assert st.step(cases.load_golden("hc_cem_m2_n100_h4_s0")["obs0"], fam.stream) == _lib.L2A_OK
        return _snapshot(st)
    finally:
        st.close()


@pytest.mark.parametrize("kind", ["parity", "device", "cem"])
def test_destroy_with_a_step_in_flight_returns_the_contexts_counters(kind, families, untouched_step, split_off):
    cem = families["cem"]
    fam = cem if kind == "cem" else families["mlp"]
    lib = fam.native.lib
    assert fam.native.ctx is split_off and cem.native.ctx is split_off
    obs = cases.load_golden("hc_cem_m2_n100_h4_s0")["obs0"]
    np.random.seed(3)
    if kind == "cem":
        gone = _cem_step(fam, 5)
    else:
        gone = NativeStep(fam.native, False, fam.m, fam.n, fam.h, fam.low, fam.high, 1.0, fam.reward,
                          device_seed=(5 if kind == "device" else None))
    np.copyto(gone.obs, cases.load_golden("hc_cem_m2_n100_h4_s0" if kind == "cem" else "hc_rs_m2_n100_h7_e2_s0")["obs0"])
    st = _cem_step(cem, 21)
    try:
        np.copyto(st.obs, obs)
        assert lib.l2a_controller_begin(gone.handle, gone._p[0], fam.stream) == _lib.L2A_OK
        assert lib.l2a_controller_begin(st.handle, st._p[0], cem.stream) == L2A_ESTATE       # the abandoned step is counted ...
        lib.l2a_controller_destroy(gone.handle)                                              # ... never finished ...
        gone.handle = None
        assert lib.l2a_controller_begin(st.handle, st._p[0], cem.stream) == _lib.L2A_OK      # ... and no longer counted
        assert lib.l2a_controller_finish(st.handle, st._p[1], st._p[2], st._p[3]) == _lib.L2A_OK
        assert _snapshot(st) == untouched_step
    finally:
        gone.close()
        st.close()


# ---- 3. the stats slots ----------------------------------------------------------------------------------------------------------------
def test_stats_slots_after_one_parity_step(families, split_off):
    fam = families["mlp"]
    lib = fam.native.lib
    np.random.seed(4)
    st = NativeStep(fam.native, False, fam.m, fam.n, fam.h, fam.low, fam.high, 1.0, fam.reward)
    try:
        assert st.step(cases.load_golden("hc_rs_m2_n100_h7_e2_s0")["obs0"], fam.stream)
        full = (ctypes.c_double * 16)(*([-7.0] * 16))
        assert lib.l2a_controller_stats(st.handle, full, 16) == _lib.L2A_OK
        v = list(full)
        assert v[7] == 1.0 and v[15] == 1.0, v                          # steps, sync_draws (nothing was armed: the step drew itself)
        assert v[6] >= v[4] >= 0.0, v                                    # stage_us: call >= wait
        part = (ctypes.c_double * 16)(*([-7.0] * 16))
        assert lib.l2a_controller_stats(st.handle, part, 4) == _lib.L2A_OK
        assert list(part)[:4] == v[:4] and list(part)[4:] == [-7.0] * 12
    finally:
        st.close()
