"""Python handle on a CEM ``l2a_controller`` (``include/l2a.h``: ``l2a_cem_controller_create_device``) - the whole device-mode
plan step of ``MPCController.get_cem_action_device`` in ONE C call.

Per step the C controller enqueues iteration 0's sampling, then per iteration the fused rollout and one ``l2a_cem_refit_sample``
(iteration i's returns -> iteration i + 1's candidates), the pick of the best candidate, and one read-back; the Python path makes
three ctypes calls and a torch call per iteration.  Same Philox offsets as the Python path: with the same seed and the same number
of iterations planned so far the result is bit-identical.

``shard=(rank, world, reduce)`` builds ONE rank of a plan sharded over ``world`` GPUs (``l2a_cem_controller_create_sharded_device``):
the rank rolls out its slice of the candidates and every iteration's returns are gathered by an int64 MAX all-reduce of
``m * n + 3`` words - ``reduce(tensor)`` in place (torch.distributed), or the library's own RCCL communicator when ``reduce`` is
None.  Every rank's step equals the unsharded one bit for bit.

A recurrent native model (one with ``units``: ``RNNMPCController``) builds ``l2a_lstm_cem_controller_create_device`` /
``_sharded_device``: every rollout starts from the controller's hidden state and ``step(..., state=(c0, h0, c_next, h_next))``
also advances that state with the chosen actions, behind the pick and in front of the one read-back.
"""

import ctypes
import os

import numpy as np

from .. import _lib
from .native_step import make_reduce_cb


class NativeCemStep(object):
    def __init__(self, native, m, n, h, low, high, discount, reward, iters, num_elites, alpha, reference, seed, shard=None):
        lib = native.lib
        self.lib, self.ctx, self.native = lib, native.ctx, native
        self.m, self.n, self.h, self.iters = int(m), int(n), int(h), int(iters)
        self.D = self.h * native.act_dim
        self.recurrent = hasattr(native, "units")
        if self.recurrent and not hasattr(lib, "l2a_lstm_cem_controller_create_device"):
            raise _lib.L2AError("this libl2a_hip.so has no recurrent CEM controller step")
        low = np.ascontiguousarray(low, dtype=np.float64)
        high = np.ascontiguousarray(high, dtype=np.float64)
        handle = ctypes.c_void_p()
        self.reduce_error = None
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        seed = ctypes.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF)
        if shard is None:
            create = lib.l2a_lstm_cem_controller_create_device if self.recurrent else lib.l2a_cem_controller_create_device
            rc = create(native.handle, self.m, self.n, self.h, low.ctypes.data, high.ctypes.data,
                        float(discount), ctypes.byref(reward), self.iters, int(num_elites), float(alpha),
                        1 if reference else 0, seed, ctypes.byref(handle))
            self.ctx.check(rc, "l2a_cem_controller_create_device")
        else:
            rank, world, reduce = shard
            cb = make_reduce_cb(self, lib, native, reduce)
            create = (lib.l2a_lstm_cem_controller_create_sharded_device if self.recurrent
                      else lib.l2a_cem_controller_create_sharded_device)
            rc = create(native.handle, self.m, self.n, self.h, low.ctypes.data, high.ctypes.data,
                        float(discount), ctypes.byref(reward), self.iters, int(num_elites),
                        float(alpha), 1 if reference else 0, seed, int(rank), int(world), cb, None,
                        ctypes.byref(handle))
            self.ctx.check(rc, "l2a_cem_controller_create_sharded_device")
        self.handle = handle
        self.pid = os.getpid()
        self.obs = np.empty((self.m, native.obs_dim), dtype=np.float64)
        self.act = np.empty((self.m, native.act_dim), dtype=np.float64)
        self.idx = np.empty((self.m,), dtype=np.int64)
        self.ret = np.empty((self.m,), dtype=np.float32)
        self._p = (self.obs.ctypes.data, self.act.ctypes.data, self.idx.ctypes.data, self.ret.ctypes.data)
        self.steps = 0
        self._stats = (ctypes.c_double * 16)()

    def step(self, observations, stream, state=None):
        """One plan step; ``self.act`` / ``self.idx`` / ``self.ret`` hold the result afterwards.  ``state`` (recurrent):
        ``(c0, h0, c_next, h_next)`` device pointers; ``c_next`` and ``h_next`` both None plan without advancing the state."""
        np.copyto(self.obs, observations, casting="same_kind")
        p = self._p
        if self.recurrent:
            rc = self.lib.l2a_lstm_controller_step(self.handle, p[0], state[0], state[1], state[2], state[3], p[1], p[2], p[3], stream)
        else:
            rc = self.lib.l2a_controller_step(self.handle, p[0], p[1], p[2], p[3], stream)
        if rc == _lib.L2A_STEP_UNSPLIT:         # the C side has switched the context to the unsplit geometry (same bits)
            self.ctx.split_degraded = True
        elif rc != _lib.L2A_OK:
            if self.reduce_error is not None:
                exc, self.reduce_error = self.reduce_error, None
                raise exc
            self.ctx.check(rc, "l2a_controller_step (CEM)")
        self.steps += 1
        return rc

    def result(self, with_returns=True):
        """``(mean [m, D], std [m, D], returns [iters, m, n] or None)`` of the latest step (host fp32)."""
        mean = np.empty((self.m, self.D), dtype=np.float32)
        std = np.empty((self.m, self.D), dtype=np.float32)
        rets = np.empty((self.iters, self.m, self.n), dtype=np.float32) if with_returns else None
        self.ctx.check(self.lib.l2a_cem_controller_result(self.handle, mean.ctypes.data, std.ctypes.data,
                                                          rets.ctypes.data if rets is not None else None),
                       "l2a_cem_controller_result")
        return mean, std, rets

    def stats(self):
        self.ctx.check(self.lib.l2a_controller_stats(self.handle, self._stats, 16), "l2a_controller_stats")
        v = list(self._stats)
        return dict(stage_us=dict(sample=v[1], launch=v[2], wait=v[4], decode=v[5], call=v[6]), steps=int(v[7]), relaunches=int(v[8]))

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
