"""What the tests of the iCEM plan step as one C call share (``tests/test_icem_step_gpu.py``, ``tests/test_sharded_icem_step_gpu.py``):
the two small golden-case models of ``tests/test_icem_controller_gpu.py``, a C controller and a Python ``MPCController`` on the same
model, and the bit-for-bit comparison of their steps.  The Python loop ``get_icem_action`` under the same seed is the reference
everywhere; nothing is left to a tolerance.

``icem_keep=0.5`` by default, so that rows are kept: with ``percent_elites=0.1`` and ``icem_decay=1.25`` three iterations plan on
64 / 51 / 40 candidates (K = 6, Kk = 3) on ``mlp`` and on 96 / 76 / 61 (K = 9, Kk = 4) on ``ens5`` - small, uneven, different from
``n`` from iteration 1 on and not divisible by 3."""

import numpy as np
import torch

import cases
from learning_to_adapt_amd.policies.native_icem_step import NativeIcemStep

MODELS = {"mlp": dict(cases.CASES["hc_rs_m3_n64_h5"]),
          "ens5": dict(cases.CASES["c2_hc_rs_n2000_h30_e5"], n=96, h=6)}        # the 5-member mean ensemble on a small plan


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
    def __init__(self, which, n=None, **icem):
        """``icem``: the planner's keywords (``icem_iters``, ``icem_keep``, ...) of both sides; ``n``: another number of candidates."""
        self.case = dict(MODELS[which])
        if n is not None:
            self.case["n"] = n
        self.env, self.model = cases.product_model(self.case)
        self.native = self.model.planner_model()
        self.icem = dict(dict(icem_keep=0.5, icem_iters=3), **icem)
        self.n, self.m, self.h = self.case["n"], self.case["m"], self.case["h"]
        self.stream = torch.cuda.current_stream(self.native.device).cuda_stream
        obs0 = cases.load_golden("%s_s%d" % (self.case["name"], self.case["seeds"][0]))["obs0"]
        rs = np.random.RandomState(8)
        self.obs = [obs0 + 0.01 * k * rs.randn(*obs0.shape) for k in range(4)]

    def python(self, **kw):
        """An ``MPCController`` on the shared model (``native_icem_step=True`` in ``kw``: the one under test).  Every iteration's
        table of returns is traced, so that the comparison covers them all."""
        ctrl = cases.product_controller(self.case, model=self.model, env=self.env, rng="device", use_icem=True, **dict(self.icem, **kw))
        ctrl.icem_trace_returns = True
        return ctrl

    def sizes(self):
        """``(K, Kk, pops)`` of the Python controller."""
        return self.python()._icem_sizes()

    def controller(self, seed, shard=None, **over):
        """A ``NativeIcemStep`` with the Python controller's constants; ``over`` replaces create arguments by name."""
        ref = self.python()
        K, Kk, pops = ref._icem_sizes()
        args = dict(m=self.m, n=self.n, h=self.h, pops=pops, K=K, Kk=Kk, alpha=ref.alpha, rho=ref.icem_rho,
                    sigma0=ref._icem_sigma_vector(), add_mean=ref.icem_add_mean)
        args.update(over)
        return NativeIcemStep(self.native, args["m"], args["n"], args["h"], self.env.action_space.low, self.env.action_space.high,
                              self.case.get("discount", 1.0), ref._reward_spec, args["pops"], args["K"], args["Kk"], args["alpha"],
                              args["rho"], args["sigma0"], args["add_mean"], seed, shard=shard)

    @staticmethod
    def snapshot(st, rc):
        mean, std, kept, counts, heads, rets = st.result()
        return dict(rc=rc, act=st.act.copy(), idx=st.idx.copy(), ret=st.ret.copy(), mean=mean, std=std, kept=kept, counts=counts,
                    heads=heads, rets=rets)

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
            assert ctrl._icemstep is None
            outs.append(dict(act=act.copy(), plan=dict(ctrl.last_plan)))
        return outs


def same_step(got, want, where):
    """A C step's snapshot against a Python step: action, index, best return, mean, spread, kept rows, counts, the valid and elite
    counts of every iteration, every iteration's best return and index, and every iteration's returns, bit for bit."""
    plan = want["plan"]
    A = got["act"].shape[1]
    assert got["act"].dtype == np.float64 and bits(got["act"]) == bits(want["act"]), where
    assert np.array_equal(got["idx"], plan["best_index"]), where
    assert bits(got["ret"]) == bits(np.asarray(plan["best_return"], dtype=np.float32)), where
    assert bits(got["mean"]) == bits(plan["icem_mean"]), where
    assert bits(got["std"]) == bits(plan["icem_std"]), where
    assert got["kept"].shape == plan["icem_elites"].shape and bits(got["kept"]) == bits(plan["icem_elites"]), where
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], plan["icem_elite_count"]), where
    trace = plan["icem_trace"]
    assert len(trace) == got["heads"].shape[0] == len(got["rets"]), where
    for it, step in enumerate(trace):
        head = got["heads"][it]
        as_int = lambda a: a.copy().view(np.int32).astype(np.int64)     # noqa: E731
        assert bits(head[:, A]) == bits(step["best_return"]), (where, it)
        assert np.array_equal(as_int(head[:, A + 1]), step["best_index"]), (where, it)
        assert np.array_equal(as_int(head[:, A + 2]), step["elites"]), (where, it)
        assert np.array_equal(as_int(head[:, A + 3]), step["valid"]), (where, it)
        assert got["rets"][it].shape == (got["act"].shape[0], step["n"]), (where, it)
        assert bits(got["rets"][it]) == bits(step["returns"]), (where, it)
    assert np.array_equal(as_int(got["heads"][-1][:, A + 3]), plan["icem_valid"]), where
    assert bits(got["heads"][-1][:, :A].astype(np.float64)) == bits(want["act"]), where
    assert bits(got["rets"][-1]) == bits(plan["returns"]), where


def same_snapshot(got, want, where):
    """Two C steps' snapshots (sharded against unsharded): everything, every iteration's gathered table included."""
    for key in ("act", "idx", "ret", "mean", "std", "kept", "counts", "heads"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and bits(got[key]) == bits(want[key]), (where, key)
    assert len(got["rets"]) == len(want["rets"]), where
    for it, (a, b) in enumerate(zip(got["rets"], want["rets"])):
        assert a.shape == b.shape and bits(a) == bits(b), (where, "rets", it)
