"""Python handle on an ``l2a_controller`` (``include/l2a.h``: ``l2a_controller_*``) - the whole parity-mode controller step
of ``MPCController.get_actions`` / ``RNNMPCController.get_actions`` in ONE C call.

The reference's step (``policies/mpc_controller.py:59-69,108-129``) draws ``h*n*m`` candidate rows from NumPy's global
generator, rolls them out and returns the best candidate's first action.  The C controller keeps that contract - same numbers,
same generator state afterwards - with the draw done ahead of time by a C thread (``csrc/l2a_rng.c``, adopted only when the
global generator is still in the state the block started from), and the launch, the wait for the mailbox word, the key decode
and the gather of the float64 action inside ``l2a_controller_step``.  What is left on the Python side of a step: one copy of
the observations into a preallocated array, one ``ctypes`` call, two small array copies.
"""

import ctypes
import os

import numpy as np

from .. import _lib
from ..utils import fast_rng


class _DevWords(object):
    """``__cuda_array_interface__`` view of ``words`` int64 words at a raw device address (the C controller's payload buffer)."""

    def __init__(self, ptr, words):
        self.__cuda_array_interface__ = {"shape": (int(words),), "typestr": "<i8", "data": (int(ptr), False), "version": 2}


def _alias_int64(ptr, words, device):
    import torch
    return torch.as_tensor(_DevWords(ptr, words), device=device)


def make_reduce_cb(owner, lib, native, reduce):
    """ctypes callback around ``reduce(tensor)`` for a sharded C controller (``l2a_reduce_fn``; None: the library's own RCCL
    communicator is used).  The collective runs on a tensor torch allocated itself (what every backend is used to); the library's
    words are copied in and out on the same stream (two tiny copies) - the alias of the library's buffer never reaches the process
    group.  The callback is kept alive on ``owner`` (``_reduce_cb``); an exception raised by ``reduce`` is parked in
    ``owner.reduce_error`` - it must not unwind through the C frame - and the C step fails."""
    owner._reduce_cb = None
    owner.reduce_error = None
    if reduce is None:
        return None
    owner._payload = None

    def _cb(arg, ptr, words, stream, _reduce=reduce):
        try:
            if owner._payload is None or owner._payload[0] != (ptr, words):
                import torch
                alias = _alias_int64(ptr, words, native.device)
                owner._payload = ((ptr, words), alias, torch.empty_like(alias))
            _, alias, own = owner._payload
            own.copy_(alias)
            _reduce(own)
            alias.copy_(own)
            return 0
        except Exception as exc:          # an exception must not unwind through the C frame
            owner.reduce_error = exc
            return -1
    owner._reduce_cb = lib.REDUCE_FN(_cb)    # (kept alive with the controller)
    return ctypes.cast(owner._reduce_cb, ctypes.c_void_p)


def _seed(seed):
    return ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF)


class StepHandle(object):
    """What `NativeStep`, `NativeCemStep` (policies/native_cem_step.py), `NativeMppiStep` (policies/native_mppi_step.py) and
    `NativeIcemStep` (policies/native_icem_step.py) share: the create call, the I/O arrays of a step, the
    step's return code, the stats call and the teardown.  (`PlanStep` and `WarmStep` below: what the latter three share beyond that.)"""

    def _open(self, native, create, m, n, h, low, high, discount, reward, extra, shard):
        """``lib.<create>(model, m, n, h, low, high, discount, reward, *extra[, rank, world, reduce, NULL], &handle)``."""
        lib = native.lib
        self.lib, self.ctx, self.native = lib, native.ctx, native
        self.m, self.n, self.h = int(m), int(n), int(h)
        self.recurrent = hasattr(native, "units")
        if not hasattr(lib, create):
            raise _lib.L2AError("this libl2a_hip.so has no %s" % create)
        low = np.ascontiguousarray(low, dtype=np.float64)
        high = np.ascontiguousarray(high, dtype=np.float64)
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        cb = make_reduce_cb(self, lib, native, None if shard is None else shard[2])
        tail = () if shard is None else self.shard + (cb, None)
        handle = ctypes.c_void_p()
        rc = getattr(lib, create)(native.handle, self.m, self.n, self.h, low.ctypes.data, high.ctypes.data, float(discount),
                                  ctypes.byref(reward), *extra, *tail, ctypes.byref(handle))
        self.ctx.check(rc, create)
        self.handle = handle
        self.pid = os.getpid()      # a forked child must not tear down the parent's HIP objects (it drops the handle instead)
        self.obs = np.empty((self.m, native.obs_dim), dtype=np.float64)
        self.act = np.empty((self.m, native.act_dim), dtype=np.float64)
        self.idx = np.empty((self.m,), dtype=np.int64)
        self.ret = np.empty((self.m,), dtype=np.float32)
        self._p = (self.obs.ctypes.data, self.act.ctypes.data, self.idx.ctypes.data, self.ret.ctypes.data)
        self._stats = (ctypes.c_double * 16)()

    def _call(self, state, stream):
        """The whole step in one call.  ``state`` (recurrent): ``(c0, h0, c_next, h_next)`` device pointers."""
        p = self._p
        if self.recurrent:
            return self.lib.l2a_lstm_controller_step(self.handle, p[0], state[0], state[1], state[2], state[3], p[1], p[2], p[3], stream)
        return self.lib.l2a_controller_step(self.handle, p[0], p[1], p[2], p[3], stream)

    def _raise(self, rc, what):
        """A failed call: the exception the reduce callback parked (it could not unwind through the C frame), else the library's."""
        if self.reduce_error is not None:
            exc, self.reduce_error = self.reduce_error, None
            raise exc
        self.ctx.check(rc, what)

    def _settle(self, rc, what):
        if rc == _lib.L2A_STEP_UNSPLIT:        # the C side has switched the context to the unsplit geometry (same bits)
            self.ctx.split_degraded = True
        elif rc != _lib.L2A_OK:
            self._raise(rc, what)

    def _stat_slots(self):
        self.ctx.check(self.lib.l2a_controller_stats(self.handle, self._stats, 16), "l2a_controller_stats")
        return list(self._stats)

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self, "pid", None) == os.getpid():
                self.lib.l2a_controller_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanStep(StepHandle):
    """What the device-mode plan steps (`NativeCemStep`, `NativeMppiStep`, `NativeIcemStep`) share: the step call and its stats.
    ``label``: the planner's name in error messages."""

    label = None

    def step(self, observations, stream, state=None):
        """One plan step; ``self.act`` / ``self.idx`` / ``self.ret`` hold the result afterwards.  Returns the C step's code
        (``L2A_OK`` or ``L2A_STEP_UNSPLIT``)."""
        np.copyto(self.obs, observations, casting="same_kind")
        rc = self._call(state, stream)
        self._settle(rc, "l2a_controller_step (%s)" % self.label)
        self.steps += 1
        return rc

    def stats(self):
        v = self._stat_slots()
        return dict(stage_us=dict(sample=v[1], launch=v[2], wait=v[4], decode=v[5], call=v[6]), steps=int(v[7]), relaunches=int(v[8]))


class WarmStep(PlanStep):
    """A plan that persists from step to step on the device (`NativeMppiStep`, `NativeIcemStep`): the reset marks and the reseed.
    ``prefix``: the planner's entry points are ``l2a_<prefix>_controller_*``."""

    prefix = None

    def step(self, observations, stream):       # (no recurrent state: these planners take an MLP model)
        return PlanStep.step(self, observations, stream)

    def reset(self, dones=None):
        """The marked envs' next step starts afresh (MPPI: from a zero mean; iCEM: zero mean, the initial spread, no kept elites);
        ``None``: every env's."""
        flags = None if dones is None else np.ascontiguousarray(np.asarray(dones, dtype=bool), dtype=np.uint8)
        if flags is not None and flags.shape != (self.m,):
            raise ValueError("dones must hold one flag per env (%d), got shape %s" % (self.m, flags.shape))
        name = "l2a_%s_controller_reset" % self.prefix
        self.ctx.check(getattr(self.lib, name)(self.handle, None if flags is None else flags.ctypes.data), name)

    def reseed(self, seed):
        """The Philox stream restarts at 0 under ``seed``; the plan (MPPI: the mean; iCEM: mean, spread, kept elites and counts) is
        kept."""
        name = "l2a_%s_controller_reseed" % self.prefix
        self.ctx.check(getattr(self.lib, name)(self.handle, _seed(seed)), name)


class NativeStep(StepHandle):
    def __init__(self, native, recurrent, m, n, h, low, high, discount, reward, device_seed=None, shard=None):
        """``device_seed``: None = parity mode (NumPy's global generator, candidates drawn ahead by a C thread); an integer =
        ``rng="device"``: the candidates come from the library's counter-based Philox stream under that seed, drawn on the GPU.
        ``shard``: None, or ``(rank, world, reduce)`` - the sharded step (``l2a_controller_create_sharded[_device]``; recurrent
        models: ``l2a_lstm_controller_create_sharded[_device]``, which also advance the hidden state with the GLOBAL winner's
        action behind the collective): ``reduce`` = None runs the step's one collective over the library's own RCCL communicator
        (``l2a_comm_init``), else a callable ``reduce(payload)`` that MAX-all-reduces the int64 CUDA tensor it is handed in place
        (torch.distributed)."""
        self.device_rng = device_seed is not None
        self.addr = None if self.device_rng else fast_rng._global_addr()
        self.lock = None if self.device_rng else fast_rng._global_lock()
        if not self.device_rng and self.addr is None:
            raise _lib.L2AError("np.random's global generator is not the legacy MT19937")
        create = "l2a_%scontroller_create%s%s" % ("lstm_" if recurrent else "", "_sharded" if shard is not None else "",
                                                  "_device" if self.device_rng else "")
        extra = (_seed(device_seed),) if self.device_rng else (self.addr, fast_rng.threads())
        self._open(native, create, m, n, h, low, high, discount, reward, extra, shard)
        self.recurrent = bool(recurrent)
        self.misses_in_row = 0
        self.cooldown = 0

    def step(self, observations, stream, state=None):
        """One controller step.  Returns True (``self.act`` / ``self.idx`` / ``self.ret`` hold the result; when no valid block of
        candidates was waiting the C step drew them itself from the global generator), or False when the controller cannot serve
        the call (a forked child) - nothing has been consumed or launched then.  ``state`` (recurrent): ``(c0, h0, c_next,
        h_next)`` device pointers."""
        np.copyto(self.obs, observations, casting="same_kind")
        p = self._p
        if self.device_rng:
            rc = self._call(state, stream)
        else:
            # The generator's own lock - no other thread draws between the state compare and the adoption - held around the
            # FIRST half of the step only (take / draw, launch, producer kick: everything that touches the generator,
            # include/l2a.h "threading contract"); the wait for the GPU runs without it, so a thread that draws from
            # np.random meanwhile (an env reset) is not stalled for the length of a plan.
            with self.lock:
                rc = self._begin(p, state, stream)
            if rc == _lib.L2A_OK:
                rc = self.lib.l2a_controller_finish(self.handle, p[1], p[2], p[3])
        if rc == _lib.L2A_STEP_MISS:
            return False
        if rc != _lib.L2A_OK and rc != _lib.L2A_STEP_DREW:   # (DREW: no valid block was waiting, the step drew synchronously itself)
            self._settle(rc, "l2a_controller_step")
        self.misses_in_row = 0
        return True

    def _begin(self, p, state, stream):
        if self.recurrent:
            return self.lib.l2a_lstm_controller_begin(self.handle, p[0], state[0], state[1], state[2], state[3], stream)
        return self.lib.l2a_controller_begin(self.handle, p[0], stream)

    def rearm(self):
        """After a synchronous draw: the chain restarts at the current global state.  Backs off while steps keep missing
        (a consumer of ``np.random`` runs between the controller's steps: every block drawn ahead would be thrown away)."""
        if self.device_rng:
            return
        self.misses_in_row += 1
        if self.misses_in_row > 2:
            self.cooldown += 1
            if self.cooldown % 16 != 0:
                return
        with self.lock:
            self.ctx.check(self.lib.l2a_controller_rearm(self.handle), "l2a_controller_rearm")

    def stats(self):
        v = self._stat_slots()
        return dict(stage_us=dict(take=v[0], stage_obs=v[1], launch=v[2], kick=v[3], wait=v[4], decode=v[5], call=v[6]),
                    steps=int(v[7]), relaunches=int(v[8]), sync_draws=int(v[15]), hits=int(v[9]), misses=int(v[10]), produced=int(v[11]),
                    producer_us_per_block=v[12], consumer_wait_us_per_take=v[13], armed=bool(v[14]))

    def actions_ptr(self):
        return self.lib.l2a_controller_actions(self.handle)
