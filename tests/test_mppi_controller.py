"""The reward-weighted (MPPI) planner's Python surface without a GPU: constructor keywords and their errors, the forms of
``mppi_sigma``, ``reset`` bookkeeping, pickling, the C entry points' declarations, and the ``L2AError`` a plan step raises when
there is no device."""

import inspect
import os
import pickle
import re

import numpy as np
import pytest

import cases
from learning_to_adapt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "hc_cem_m2_n100_h4"
DEFAULTS = dict(use_mppi=False, mppi_kappa=1.0, mppi_sigma=None, mppi_beta=0.6, mppi_iters=1)


def _controller(**kw):
    case = dict(cases.CASES[CASE], planner="rs")
    kw.setdefault("rng", "device")
    return cases.product_controller(case, **kw)


def test_constructor_defaults():
    from learning_to_adapt_amd.policies import MPCController, RNNMPCController
    for cls in (MPCController, RNNMPCController):
        params = inspect.signature(cls.__init__).parameters
        for name, default in DEFAULTS.items():
            assert params[name].default == default and (default is not None or params[name].default is None), (cls, name)


def test_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "l2a.h")).read()
    for name in ("l2a_mppi_sample", "l2a_mppi_update"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert len(lib.l2a_mppi_sample.argtypes) == 18 and len(lib.l2a_mppi_update.argtypes) == 11
    assert int(re.search(r"#define L2A_MPPI_UPDATE_STATIC_LDS (\d+)", text).group(1)) == __import__("mppi_reference").UPDATE_STATIC_LDS


def test_constructor_errors():
    with pytest.raises(ValueError, match="use_cem"):
        cases.product_controller(dict(cases.CASES[CASE]), rng="device", use_mppi=True)          # the case's planner is CEM
    with pytest.raises(ValueError, match="rng='device'"):
        _controller(use_mppi=True, rng="numpy")
    for bad in (dict(mppi_kappa=0.0), dict(mppi_kappa=float("inf")), dict(mppi_beta=0.0), dict(mppi_beta=1.5), dict(mppi_iters=0),
                dict(mppi_sigma=-1.0), dict(mppi_sigma=[0.1, 0.2]), dict(mppi_sigma=float("nan"))):
        with pytest.raises(ValueError):
            _controller(use_mppi=True, **bad)
    _controller(use_mppi=False, mppi_kappa=0.0)             # (the planner's keywords are only judged when it is chosen)


def test_sigma_forms():
    ctrl = _controller(use_mppi=True)
    low, high = ctrl.action_space.low, ctrl.action_space.high
    s = ctrl._mppi_sigma_vector()
    assert s.dtype == np.float32 and np.array_equal(s, (0.25 * (high.astype(np.float64) - low)).astype(np.float32))
    assert np.array_equal(_controller(use_mppi=True, mppi_sigma=0.3)._mppi_sigma_vector(), np.full(low.shape, 0.3, dtype=np.float32))
    per_dim = np.linspace(0.0, 0.5, low.shape[0])
    assert np.array_equal(_controller(use_mppi=True, mppi_sigma=per_dim)._mppi_sigma_vector(), per_dim.astype(np.float32))


def test_reset_marks_envs_and_stays_a_no_op_without_mppi():
    plain = _controller()
    plain.reset(dones=[True, False])
    plain.reset()
    assert "mppi_fresh" not in plain._bufs
    ctrl = _controller(use_mppi=True)
    ctrl._bufs["mppi_fresh"] = np.zeros(3, dtype=bool)      # as a step over three envs leaves it
    ctrl.reset(dones=[False, True, False])
    assert ctrl._bufs["mppi_fresh"].tolist() == [False, True, False]
    ctrl.reset(dones=[True, False, False])
    assert ctrl._bufs["mppi_fresh"].tolist() == [True, True, False]
    ctrl.reset(dones=[True, False])                         # another number of envs: all start afresh
    assert ctrl._bufs["mppi_fresh"] is None
    ctrl._bufs["mppi_fresh"] = np.zeros(3, dtype=bool)
    ctrl.reset()
    assert ctrl._bufs["mppi_fresh"] is None


def test_pickling_keeps_the_keywords_and_drops_the_plan():
    ctrl = _controller(use_mppi=True, mppi_kappa=2.5, mppi_sigma=0.2, mppi_beta=0.8, mppi_iters=2)
    ctrl._bufs["mppi_fresh"] = np.zeros(2, dtype=bool)
    twin = pickle.loads(pickle.dumps(ctrl))
    assert (twin.use_mppi, twin.mppi_kappa, twin.mppi_sigma, twin.mppi_beta, twin.mppi_iters, twin.rng) == (True, 2.5, 0.2, 0.8, 2, "device")
    assert "mppi_fresh" not in twin._bufs and "mppi_means" not in twin._bufs


def test_rnn_controller_takes_the_keywords():
    name = cases.rnn_case_ids()[0]
    case, _ = cases.split_id(name)
    ctrl = cases.product_rnn_controller(dict(case, planner="rnn_rs"), rng="device", use_mppi=True, mppi_iters=2)
    assert ctrl.use_mppi and ctrl.mppi_iters == 2
    twin = pickle.loads(pickle.dumps(ctrl))
    assert twin.use_mppi and twin.mppi_iters == 2
    with pytest.raises(ValueError):
        cases.product_rnn_controller(dict(case, planner="rnn_cem"), rng="device", use_mppi=True)


def test_plan_step_without_a_gpu_raises_l2a_error():
    import torch
    if torch.cuda.is_available():
        return
    ctrl = _controller(use_mppi=True)
    obs = cases.load_golden(CASE + "_s0")["obs0"]
    with pytest.raises(_lib.L2AError):
        ctrl.get_actions(obs)
    with pytest.raises(_lib.L2AError):
        ctrl.get_action(obs[0])
