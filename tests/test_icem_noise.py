"""iCEM's power-law noise without a GPU: the four entry points' declarations and bindings, ``l2a_icem_noise_matrix`` (host only)
against the float64 restatement ``icem_noise_reference.noise_matrix``, the ``icem_noise`` / ``icem_beta`` keywords, pickling, and
which sample entry ``get_icem_action`` reaches (native calls stubbed)."""

import ctypes
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import torch

import cases
import icem_noise_reference as nr
from learning_to_adapt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "hc_cem_m2_n100_h4"
NEW = dict(l2a_icem_noise_matrix=3, l2a_icem_sample_noise=24, l2a_icem_sample_noise_shard=26, l2a_icem_controller_set_noise=2)


def _controller(**kw):
    case = dict(cases.CASES[CASE], planner="rs")
    return cases.product_controller(case, rng="device", use_icem=True, **kw)


def test_the_four_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    lib = _lib.load()
    for name, count in NEW.items():
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count, name
    assert re.search(r"#define L2A_ICEM_NOISE_MAX_H 128\b", text)
    # the AR(1) entries keep their signatures; the noise entries take a pointer where those take rho
    assert len(lib.l2a_icem_sample.argtypes) == 24 and len(lib.l2a_icem_sample_shard.argtypes) == 26
    for noise, ar1 in ((lib.l2a_icem_sample_noise, lib.l2a_icem_sample), (lib.l2a_icem_sample_noise_shard, lib.l2a_icem_sample_shard)):
        assert noise.argtypes[:10] == ar1.argtypes[:10] and noise.argtypes[11:] == ar1.argtypes[11:]
        assert ar1.argtypes[10] is ctypes.c_float and noise.argtypes[10] is ctypes.c_void_p
    assert "a power-law noise spectrum" not in text and "the recurrence is AR(1)" not in text


# ---------------------------------------------------------------------------------------------------------- l2a_icem_noise_matrix
def _matrix(h, beta, rows=None):
    lib = _lib.load()
    M = np.full((h if rows is None else rows, max(h, 1)), -7.0, dtype=np.float32)
    return lib.l2a_icem_noise_matrix(h, float(beta), M.ctypes.data), M


@pytest.mark.parametrize("h", [1, 2, 3, 4, 7, 30, 33, 127, 128])
def test_noise_matrix_is_the_float64_restatement_rounded_once(h):
    """Every entry within ``2^-23 |x| + 1e-15`` of the float64 restatement: one fp32 rounding, which may fall to either side where
    the two float64 values straddle a tie, plus the libm difference at entries that are zero in exact arithmetic.  Row norms
    within ``(h + 2) 2^-24`` of 1: ``h`` entries each off by at most ``2^-24`` of their magnitude move the squared norm by at most
    ``2 * 2^-24 sum x^2``, the norm by half of that; the rest covers the float64 matrix's own error."""
    for beta in (0.0, 0.5, 1.0, 2.0, 4.0, 8.0):
        rc, M = _matrix(h, beta)
        assert rc == _lib.L2A_OK
        want = nr.noise_matrix(h, beta)
        err = np.abs(M.astype(np.float64) - want)
        assert np.all(err <= 2.0 ** -23 * np.abs(want) + 1e-15), (h, beta, float(err.max()))
        norms = np.sqrt((M.astype(np.float64) ** 2).sum(axis=1))
        assert np.max(np.abs(norms - 1.0)) <= (h + 2) * 2.0 ** -24, (h, beta)


def test_noise_matrix_refusals_write_nothing():
    lib = _lib.load()
    for h, beta in ((0, 1.0), (129, 1.0), (30, -1.0), (30, float("nan")), (30, 8.5), (30, float("inf"))):
        rc, M = _matrix(h, beta, rows=130)
        assert rc == _lib.L2A_EINVAL and np.all(M == -7.0), (h, beta)
    assert lib.l2a_icem_noise_matrix(30, 1.0, None) == _lib.L2A_EINVAL


# ------------------------------------------------------------------------------------------------------------------ the keywords
def test_keywords_default_to_ar1_and_are_validated():
    from learning_to_adapt_amd.policies import MPCController
    params = inspect.signature(MPCController.__init__).parameters
    assert params["icem_noise"].default == "ar1" and params["icem_beta"].default == 2.0
    ctrl = _controller()
    assert ctrl.icem_noise == "ar1" and ctrl.icem_beta == 2.0
    ctrl = _controller(icem_noise="powerlaw", icem_beta=1)
    assert ctrl.icem_noise == "powerlaw" and ctrl.icem_beta == 1.0 and isinstance(ctrl.icem_beta, float)
    assert _controller(icem_noise="powerlaw", icem_beta=0.0).icem_beta == 0.0
    assert _controller(icem_noise="powerlaw", icem_beta=8.0).icem_beta == 8.0
    for bad in (dict(icem_noise="pink"), dict(icem_noise=None), dict(icem_noise="powerlaw", icem_beta=float("nan")),
                dict(icem_noise="powerlaw", icem_beta=float("inf")), dict(icem_noise="powerlaw", icem_beta=-0.5),
                dict(icem_noise="powerlaw", icem_beta=8.5)):
        with pytest.raises(ValueError):
            _controller(**bad)


def test_pickling_keeps_the_keywords():
    twin = pickle.loads(pickle.dumps(_controller(icem_noise="powerlaw", icem_beta=1.5, native_icem_step=True)))
    assert twin.icem_noise == "powerlaw" and twin.icem_beta == 1.5 and twin.native_icem_step is True
    assert twin._icemstep is None and "icem_noise" not in twin._bufs
    twin = pickle.loads(pickle.dumps(_controller()))
    assert twin.icem_noise == "ar1" and twin.icem_beta == 2.0


# ------------------------------------------------------------------------------------------ which entry a plan step reaches (stubbed)
class _FakeLib(object):
    """The sample and refit entries record their call and touch nothing; the matrix builder is the library's (host only)."""

    def __init__(self, with_noise=True):
        self.calls = []
        self.l2a_icem_sample = lambda *a: self._note("l2a_icem_sample", a)
        self.l2a_icem_refit = lambda *a: self._note("l2a_icem_refit", a)
        if with_noise:
            self.l2a_icem_sample_noise = lambda *a: self._note("l2a_icem_sample_noise", a)
            self.l2a_icem_noise_matrix = _lib.load().l2a_icem_noise_matrix

    def _note(self, name, args):
        self.calls.append((name, args))
        return _lib.L2A_OK


class _FakeCtx(object):
    handle = ctypes.c_void_p(0)

    def check(self, rc, what):
        assert rc == _lib.L2A_OK, what

    def check_or_degrade(self):
        return True


class _FakeNative(object):
    def __init__(self, lib):
        self.device = torch.device("cpu")
        self.obs_dim, self.act_dim = 20, 6
        self.lib, self.ctx = lib, _FakeCtx()


def _stubbed(monkeypatch, lib, horizon=None, **kw):
    from learning_to_adapt_amd.dynamics import native_model
    case = dict(cases.CASES[CASE], planner="rs")
    if horizon is not None:
        case["h"] = horizon
    ctrl = cases.product_controller(case, rng="device", use_icem=True, **kw)
    fake = _FakeNative(lib)
    ctrl.dynamics_model.planner_model = lambda: fake
    monkeypatch.setattr(native_model, "_stream_ptr", lambda device=None: ctypes.c_void_p(0))
    monkeypatch.setattr(_lib, "load", lambda: lib)
    ctrl._upload_obs = lambda observations: None
    ctrl._rollout = lambda observations, seq, n_it, *a, **k: (None, torch.zeros((len(observations), n_it), dtype=torch.float32))
    return case, ctrl, fake


def _zero_bufs(ctrl):
    """``_buf`` hands out uninitialised memory and the stubbed refit writes nothing: start the read-back from zeros."""
    stock = ctrl._buf

    def buf(key, shape, dtype, device):
        fresh = key not in ctrl._bufs
        t = stock(key, shape, dtype, device)
        if fresh:
            t.zero_()
        return t

    ctrl._buf = buf


def test_ar1_reaches_the_recurrence_entry_and_powerlaw_the_noise_entry(monkeypatch):
    obs = cases.load_golden(CASE + "_s0")["obs0"]
    lib = _FakeLib()
    case, ctrl, _ = _stubbed(monkeypatch, lib)
    _zero_bufs(ctrl)
    ctrl.get_actions(obs)
    names = [c[0] for c in lib.calls]
    assert names == ["l2a_icem_sample", "l2a_icem_refit"] * ctrl.icem_iters
    assert lib.calls[0][1][10] == ctrl.icem_rho and "icem_noise" not in ctrl._bufs
    assert ctrl.last_plan["icem_noise"] == "ar1" and ctrl.last_plan["icem_beta"] == 2.0

    lib = _FakeLib()
    case, ctrl, _ = _stubbed(monkeypatch, lib, icem_noise="powerlaw", icem_beta=1.0)
    _zero_bufs(ctrl)
    ctrl.get_actions(obs)
    ctrl.get_actions(obs)
    names = [c[0] for c in lib.calls]
    assert names == ["l2a_icem_sample_noise", "l2a_icem_refit"] * (2 * ctrl.icem_iters)
    (h, beta), M = ctrl._bufs["icem_noise"]
    assert (h, beta) == (case["h"], 1.0) and M.dtype == torch.float32 and tuple(M.shape) == (h, h)
    want = nr.noise_matrix(h, 1.0)
    assert np.all(np.abs(M.numpy().astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-15)
    # the matrix is built once and every call passes its address where the AR(1) entry takes rho
    assert {c[1][10].value for c in lib.calls if c[0] == "l2a_icem_sample_noise"} == {M.data_ptr()}
    assert ctrl.last_plan["icem_noise"] == "powerlaw" and ctrl.last_plan["icem_beta"] == 1.0


def test_powerlaw_refuses_a_horizon_above_the_limit_and_an_old_library(monkeypatch):
    obs = cases.load_golden(CASE + "_s0")["obs0"]
    lib = _FakeLib()
    _, ctrl, _ = _stubbed(monkeypatch, lib, horizon=129, icem_noise="powerlaw")
    with pytest.raises(_lib.L2AError, match="128"):
        ctrl.get_actions(obs)
    assert lib.calls == []
    _, ctrl, _ = _stubbed(monkeypatch, lib, horizon=129)          # AR(1) has no such limit
    _zero_bufs(ctrl)
    ctrl.get_actions(obs)
    assert lib.calls[0][0] == "l2a_icem_sample"
    old = _FakeLib(with_noise=False)
    _, ctrl, _ = _stubbed(monkeypatch, old, icem_noise="powerlaw")
    with pytest.raises(_lib.L2AError, match="rebuild"):
        ctrl.get_actions(obs)
    assert old.calls == []
