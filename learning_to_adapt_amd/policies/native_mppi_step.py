"""Python handle on an MPPI ``l2a_controller`` (``include/l2a.h``: ``l2a_mppi_controller_create_device``) - the whole plan step
of ``MPCController.get_mppi_action`` in ONE C call.

Per step the C controller enqueues, for every iteration, ``l2a_mppi_sample``, the fused rollout and ``l2a_mppi_update``, and reads
back the update's packed head only (``m * (act_dim + 4)`` floats); the plan mean and every iteration's returns stay on the device
until ``result()`` asks for them.  The Python path makes two ctypes calls, one ``_rollout`` and two tensor copies per iteration and
copies the mean and the returns back on every step.  Same Philox offsets as the Python path: with the same seed, the same number
of iterations planned so far and the same envs reset, the result is bit-identical.

``shard=(rank, world, reduce)`` builds ONE rank of a plan sharded over ``world`` GPUs (``l2a_mppi_controller_create_sharded_device``):
every rank samples all candidates of the same stream (``l2a_mppi_sample_shard``), rolls out its slice, and every iteration's returns
are gathered by an int64 MAX all-reduce of ``m * n + 3`` words - ``reduce(tensor)`` in place (torch.distributed), or the library's
own RCCL communicator when ``reduce`` is None - in front of the unchanged update.  Every rank's step equals the unsharded one bit
for bit.
"""

import numpy as np

from .native_step import WarmStep, _seed


class NativeMppiStep(WarmStep):
    """After ``step``: ``self.act`` is the new mean's first step, ``self.idx`` / ``self.ret`` the best valid candidate's index and return."""

    prefix, label = "mppi", "MPPI"

    def __init__(self, native, m, n, h, low, high, discount, reward, iters, kappa, beta, sigma, seed, shard=None):
        """``sigma``: the noise scale per action dimension (``MPCController._mppi_sigma_vector``)."""
        self.iters = int(iters)
        self.sigma = np.ascontiguousarray(sigma, dtype=np.float64)      # (kept: the create call reads it)
        create = "l2a_mppi_controller_create%s_device" % ("_sharded" if shard is not None else "")
        extra = (self.iters, float(kappa), float(beta), self.sigma.ctypes.data, _seed(seed))
        self._open(native, create, m, n, h, low, high, discount, reward, extra, shard)
        self.D = self.h * native.act_dim
        self.steps = 0

    def result(self, with_returns=True):
        """``(mean [m, D], ess [m], valid [m] int64, returns [iters, m, n] or None)`` of the latest step (host; the mean and the
        returns come back in one copy from the device, on the step's stream)."""
        mean = np.empty((self.m, self.D), dtype=np.float32)
        ess = np.empty((self.m,), dtype=np.float32)
        valid = np.empty((self.m,), dtype=np.int32)
        rets = np.empty((self.iters, self.m, self.n), dtype=np.float32) if with_returns else None
        self.ctx.check(self.lib.l2a_mppi_controller_result(self.handle, mean.ctypes.data, ess.ctypes.data, valid.ctypes.data,
                                                           rets.ctypes.data if rets is not None else None),
                       "l2a_mppi_controller_result")
        return mean, ess, valid.astype(np.int64), rets
