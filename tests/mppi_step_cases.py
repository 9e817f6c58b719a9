"""What the tests of the MPPI plan step as one C call share (``tests/test_mppi_step_gpu.py``, ``tests/test_sharded_mppi_step_gpu.py``):
the two small golden-case models of ``tests/test_mppi_controller_gpu.py``, a C controller and a Python ``MPCController`` on the same
model, and the bit-for-bit comparison of their steps.  The Python loop ``get_mppi_action`` under the same seed is the reference
everywhere; nothing is left to a tolerance."""

import numpy as np
import torch

import cases
from learning_to_adapt_amd.policies.native_mppi_step import NativeMppiStep

MODELS = {"mlp": dict(cases.CASES["hc_rs_m3_n64_h5"]),
          "ens5": dict(cases.CASES["c2_hc_rs_n2000_h30_e5"], n=96, h=6),        # the 5-member mean ensemble on a small plan
          "long": dict(cases.CASES["hc_rs_m3_n64_h5"], h=90)}   # l2a_mppi_sample_k walks this horizon in two passes (85 + 5 at A = 6)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def restore_context(ctx):
    """What a rank that owns its process would find: the context's default policies, no degradation, a clear status word."""
    torch.cuda.synchronize()
    ctx.set_split(1)
    ctx.set_fan(1)
    ctx.set_micro(1)
    ctx.set_double_rounds(1)
    ctx.split_degraded = False
    assert ctx.launch_status_value() == 0, "an earlier launch left the status word set"


class Setup(object):
    def __init__(self, which, **mppi):
        """``mppi``: the planner's keywords (``mppi_iters``, ``mppi_kappa``, ...) of both sides."""
        self.case = dict(MODELS[which])
        self.env, self.model = cases.product_model(self.case)
        self.native = self.model.planner_model()
        self.mppi = mppi
        self.n, self.m, self.h = self.case["n"], self.case["m"], self.case["h"]
        self.stream = torch.cuda.current_stream(self.native.device).cuda_stream
        obs0 = cases.load_golden("%s_s%d" % (self.case["name"], self.case["seeds"][0]))["obs0"]
        rs = np.random.RandomState(8)
        self.obs = [obs0 + 0.01 * k * rs.randn(*obs0.shape) for k in range(4)]

    def python(self, **kw):
        """An ``MPCController`` on the shared model (``native_mppi_step=True`` in ``kw``: the one under test)."""
        return cases.product_controller(self.case, model=self.model, env=self.env, rng="device", use_mppi=True, **dict(self.mppi, **kw))

    def controller(self, seed, shard=None, **over):
        """A ``NativeMppiStep`` with the Python controller's constants; ``over`` replaces create arguments by name."""
        ref = self.python()
        args = dict(m=self.m, n=self.n, h=self.h, iters=ref.mppi_iters, kappa=ref.mppi_kappa, beta=ref.mppi_beta,
                    sigma=ref._mppi_sigma_vector())
        args.update(over)
        return NativeMppiStep(self.native, args["m"], args["n"], args["h"], self.env.action_space.low, self.env.action_space.high,
                              self.case.get("discount", 1.0), ref._reward_spec, args["iters"], args["kappa"], args["beta"], args["sigma"],
                              seed, shard=shard)

    @staticmethod
    def snapshot(st, rc):
        mean, ess, valid, rets = st.result()
        return dict(rc=rc, act=st.act.copy(), idx=st.idx.copy(), ret=st.ret.copy(), mean=mean, ess=ess, valid=valid, rets=rets)

    def python_steps(self, seed, steps, resets=None, reseeds=None):
        """``steps`` consecutive steps of the Python loop under ``torch.manual_seed(seed)``; ``resets[k]`` / ``reseeds[k]``: the
        ``dones`` / the new seed applied in front of step ``k``."""
        torch.manual_seed(seed)
        ctrl = self.python()
        outs = []
        for k in range(steps):
            if reseeds and k in reseeds:
                torch.manual_seed(reseeds[k])
            if resets and k in resets:
                ctrl.reset(dones=resets[k])
            act, _ = ctrl.get_actions(self.obs[k])
            assert ctrl._mppistep is None
            outs.append(dict(act=act.copy(), plan=dict(ctrl.last_plan)))
        return outs


def same_step(got, want, where):
    """A C step's snapshot against a Python step: action, index, Rmax, mean, ESS, valid count and the returns, bit for bit."""
    plan = want["plan"]
    assert got["act"].dtype == np.float64 and bits(got["act"]) == bits(want["act"]), where
    assert np.array_equal(got["idx"], plan["best_index"]), where
    assert bits(got["ret"]) == bits(np.asarray(plan["best_return"], dtype=np.float32)), where
    assert bits(got["mean"]) == bits(plan["mppi_mean"]), where
    assert bits(got["ess"]) == bits(plan["mppi_ess"]), where
    assert np.array_equal(got["valid"], plan["mppi_valid"]), where
    assert bits(got["rets"][-1]) == bits(plan["returns"]), where        # (the Python loop keeps the last iteration's table)


def same_snapshot(got, want, where):
    """Two C steps' snapshots (sharded against unsharded): everything, every iteration's gathered table included."""
    for key in ("act", "idx", "ret", "mean", "ess", "valid", "rets"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and bits(got[key]) == bits(want[key]), (where, key)
