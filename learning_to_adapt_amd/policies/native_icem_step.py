"""Python handle on an iCEM ``l2a_controller`` (``include/l2a.h``: ``l2a_icem_controller_create_device``) - the whole plan step
of ``MPCController.get_icem_action`` in ONE C call.

Per step the C controller enqueues, for every iteration, ``l2a_icem_sample``, the fused rollout of the iteration's population and
``l2a_icem_refit``, and reads back the refits' packed result rows only (``iters * m * (act_dim + 4)`` floats); mean, spread, kept
elites, their counts and every iteration's returns stay on the device until ``result()`` asks for them.  The Python path makes two
ctypes calls, one ``_rollout`` and a tensor copy per iteration, adds four to five packing copies per step and copies the state and
a table of returns back on every step.  Same Philox offsets as the Python path: with the same seed, the same number of iterations
planned so far and the same envs reset, the result is bit-identical.

``shard=(rank, world, reduce)`` builds ONE rank of a plan sharded over ``world`` GPUs (``l2a_icem_controller_create_sharded_device``):
every rank samples all candidates of the same stream (``l2a_icem_sample_shard``), rolls out its window of the iteration's
population, and every iteration's returns are gathered by an int64 MAX all-reduce of ``m * pops[it] + 3`` words - ``reduce(tensor)``
in place (torch.distributed), or the library's own RCCL communicator when ``reduce`` is None - in front of the unchanged refit.
Every rank's step equals the unsharded one bit for bit.
"""

import numpy as np

from .._lib import L2AError
from .native_step import WarmStep, _seed


class NativeIcemStep(WarmStep):
    """After ``step``: ``self.act`` is the first action of the last iteration's best candidate, ``self.idx`` / ``self.ret`` its index and
    return."""

    prefix, label = "icem", "iCEM"

    def __init__(self, native, m, n, h, low, high, discount, reward, pops, K, Kk, alpha, rho, sigma0, add_mean, seed, shard=None):
        """``pops``, ``K``, ``Kk``: ``MPCController._icem_sizes`` (the populations per iteration, the elites, the kept elites);
        ``sigma0``: the initial spread per action dimension (``MPCController._icem_sigma_vector``)."""
        self.pops = np.ascontiguousarray(pops, dtype=np.int32)          # (kept: the create call reads it)
        self.iters = int(len(self.pops))
        self.K, self.Kk = int(K), int(Kk)
        self.sigma0 = np.ascontiguousarray(sigma0, dtype=np.float64)    # (kept: the create call reads it)
        create = "l2a_icem_controller_create%s_device" % ("_sharded" if shard is not None else "")
        extra = (self.iters, self.pops.ctypes.data, self.K, self.Kk, float(alpha), float(rho), self.sigma0.ctypes.data,
                 int(bool(add_mean)), _seed(seed))
        self._open(native, create, m, n, h, low, high, discount, reward, extra, shard)
        self.A = native.act_dim
        self.D = self.h * self.A
        self.steps = 0

    def set_noise(self, M):
        """From the next step on every iteration samples with ``nz = M z`` (``l2a_icem_sample_noise``; sharded:
        ``l2a_icem_sample_noise_shard``) in place of the AR(1) recurrence: ``M [h, h]``, any matrix - ``l2a_icem_noise_matrix``'s for
        power-law noise -, copied to the device as fp32.  ``None`` returns the controller to its ``rho``."""
        if not hasattr(self.lib, "l2a_icem_controller_set_noise"):
            raise L2AError("this libl2a_hip.so has no power-law iCEM noise (l2a_icem_controller_set_noise): rebuild it")
        if M is not None:
            M = np.ascontiguousarray(M, dtype=np.float32)
            if M.shape != (self.h, self.h):
                raise ValueError("the noise matrix must be [h, h] = [%d, %d], got shape %s" % (self.h, self.h, M.shape))
        self.ctx.check(self.lib.l2a_icem_controller_set_noise(self.handle, None if M is None else M.ctypes.data),
                       "l2a_icem_controller_set_noise")

    def heads(self):
        """The latest step's result rows ``[iters, m, act_dim + 4]`` - the step's own read-back, no copy from the device."""
        heads = np.empty((self.iters, self.m, self.A + 4), dtype=np.float32)
        self.ctx.check(self.lib.l2a_icem_controller_result(self.handle, None, None, None, None, heads.ctypes.data, None),
                       "l2a_icem_controller_result")
        return heads

    def result(self, with_returns=True):
        """``(mean [m, D], std [m, D], kept [m, Kk, D], counts [m] int64, heads [iters, m, act_dim + 4], returns or None)`` of the
        latest step (host).  ``kept``: env i's first ``counts[i]`` rows are its kept elites in rank order, zeros behind them.
        ``returns``: a list of the iterations' tables ``[m, pops[it]]`` (sharded: the gathered ones).  State and returns come back
        in one copy from the device, on the step's stream."""
        mean = np.empty((self.m, self.D), dtype=np.float32)
        std = np.empty((self.m, self.D), dtype=np.float32)
        kept = np.zeros((self.m, self.Kk, self.D), dtype=np.float32)
        kc = np.empty((self.m,), dtype=np.int32)
        heads = np.empty((self.iters, self.m, self.A + 4), dtype=np.float32)
        flat = np.empty((self.m * int(self.pops.sum()),), dtype=np.float32) if with_returns else None
        self.ctx.check(self.lib.l2a_icem_controller_result(self.handle, mean.ctypes.data, std.ctypes.data,
                                                           kept.ctypes.data if self.Kk else None, kc.ctypes.data, heads.ctypes.data,
                                                           flat.ctypes.data if flat is not None else None),
                       "l2a_icem_controller_result")
        counts = kc.astype(np.int64)
        for i in range(self.m):         # the refit writes an env's first `count` kept rows only
            kept[i, counts[i]:] = 0.0
        rets = None
        if flat is not None:
            rets, at = [], 0
            for n_it in self.pops:
                rets.append(flat[at:at + self.m * int(n_it)].reshape(self.m, int(n_it)))
                at += self.m * int(n_it)
        return mean, std, kept, counts, heads, rets
