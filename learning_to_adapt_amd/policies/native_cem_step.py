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

import numpy as np

from .native_step import PlanStep, _seed


class NativeCemStep(PlanStep):
    """``step(observations, stream, state=None)`` - ``state`` (recurrent): ``(c0, h0, c_next, h_next)`` device pointers; ``c_next`` and
    ``h_next`` both None plan without advancing the state."""

    label = "CEM"

    def __init__(self, native, m, n, h, low, high, discount, reward, iters, num_elites, alpha, reference, seed, shard=None):
        self.iters = int(iters)
        create = "l2a_%scem_controller_create%s_device" % ("lstm_" if hasattr(native, "units") else "", "_sharded" if shard is not None else "")
        extra = (self.iters, int(num_elites), float(alpha), 1 if reference else 0, _seed(seed))
        self._open(native, create, m, n, h, low, high, discount, reward, extra, shard)
        self.D = self.h * native.act_dim
        self.steps = 0

    def result(self, with_returns=True):
        """``(mean [m, D], std [m, D], returns [iters, m, n] or None)`` of the latest step (host fp32)."""
        mean = np.empty((self.m, self.D), dtype=np.float32)
        std = np.empty((self.m, self.D), dtype=np.float32)
        rets = np.empty((self.iters, self.m, self.n), dtype=np.float32) if with_returns else None
        self.ctx.check(self.lib.l2a_cem_controller_result(self.handle, mean.ctypes.data, std.ctypes.data,
                                                          rets.ctypes.data if rets is not None else None),
                       "l2a_cem_controller_result")
        return mean, std, rets
