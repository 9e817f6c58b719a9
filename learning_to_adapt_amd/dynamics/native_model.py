"""Python handle on an ``l2a_model`` (C ABI: ``include/l2a.h``).

Holds no numerics of its own: it hands device pointers of PyTorch-ROCm tensors (storage only)
to ``libl2a_hip.so`` and launches the fused rollout / predict kernels on torch's current HIP
stream.  Raises ``L2AError`` on any failure - there is no CPU fallback.
"""

import ctypes

import numpy as np
import torch

from .. import _lib
from ..envs.reward_spec import RewardProgram, RewardSpec
from ..envs.termination import TerminationProgram


def _stream_ptr(device=None):
    """torch's current HIP stream on `device` (the model's GPU, not necessarily the process' current one)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dvec(x):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    return x, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class NativeModel(object):
    def __init__(self, obs_dim, act_dim, hidden_sizes, hidden_act, output_act, n_sets, mode, device=None):
        if not torch.cuda.is_available():
            raise _lib.L2AError("no MI355X visible to PyTorch-ROCm: the rollout path is HIP-only "
                                "(there is no CPU fallback)")
        if device is None:                  # one process per GPU: the process' current device (torch.cuda.set_device)
            device = torch.cuda.current_device()
        self.ctx = _lib.Context.get(device)
        self.lib = self.ctx.lib
        self.device = torch.device("cuda", device)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.n_sets, self.mode = int(n_sets), mode
        if hidden_act not in _lib.ACT_CODES or output_act not in _lib.ACT_CODES:
            raise _lib.L2AError("nonlinearity %r / %r is not supported by the HIP kernels"
                                % (hidden_act, output_act))
        hid = (ctypes.c_int * len(self.hidden_sizes))(*self.hidden_sizes)
        handle = ctypes.c_void_p()
        rc = self.lib.l2a_model_create(self.ctx.handle, self.obs_dim, self.act_dim, len(self.hidden_sizes),
                                       hid, _lib.ACT_CODES[hidden_act], _lib.ACT_CODES[output_act],
                                       self.n_sets, _lib.MODE_CODES[mode], ctypes.byref(handle))
        self.ctx.check(rc, "l2a_model_create")
        self.handle = handle
        self._keep = {}     # source tensors kept alive until the stream has consumed them
        self.program_plans = 0      # calls of plan_rs_program (diagnostics: which plan path a controller took)
        self.reward_model_plans = 0     # calls of plan_rs_reward_model
        self.value_plans = 0        # calls of plan_rs_value
        self.term_plans = 0         # calls of plan_rs_term
        self.policy_proposals = 0   # calls of policy_propose
        self._spec_programs = {}    # RewardSpec -> its RewardProgram.from_spec (plan_rs_term scores a spec as a program)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.l2a_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters ---------------------------------------------------------------------
    def set_weights(self, e, params):
        """``params``: [W0, b0, ..., Wout, bout] (torch tensors or arrays, kernels ``[in, out]``)."""
        dev = []
        for p in params:
            t = torch.as_tensor(p) if not torch.is_tensor(p) else p
            dev.append(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        sizes = (self.obs_dim + self.act_dim,) + self.hidden_sizes + (self.obs_dim,)
        assert len(dev) == 2 * (len(sizes) - 1), "expected %d parameter arrays" % (2 * (len(sizes) - 1))
        for li in range(len(sizes) - 1):
            assert tuple(dev[2 * li].shape) == (sizes[li], sizes[li + 1]), \
                "kernel %d has shape %s, expected %s" % (li, tuple(dev[2 * li].shape), (sizes[li], sizes[li + 1]))
            assert tuple(dev[2 * li + 1].shape) == (sizes[li + 1],)
        ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        rc = self.lib.l2a_model_set_weights(self.handle, int(e), ptrs, _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_set_weights")
        self._keep[("w", e)] = dev

    def set_weights_stacked(self, first_set, stacked):
        """``stacked``: [W0, b0, ..., Wout, bout] with a leading set axis (``[count, in, out]`` / ``[count, out]``
        CUDA tensors) - all ``count`` sets go up in one strided call (``l2a_model_set_weights_strided``)."""
        sizes = (self.obs_dim + self.act_dim,) + self.hidden_sizes + (self.obs_dim,)
        assert len(stacked) == 2 * (len(sizes) - 1)
        count = int(stacked[0].shape[0])
        dev = []
        for i, t in enumerate(stacked):
            t = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            li = i // 2
            expect = (count, sizes[li], sizes[li + 1]) if i % 2 == 0 else (count, sizes[li + 1])
            assert tuple(t.shape) == expect, "stacked parameter %d has shape %s, expected %s" % (i, tuple(t.shape), expect)
            dev.append(t)
        ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        strides = (ctypes.c_longlong * len(dev))(*[int(t.stride(0)) for t in dev])
        rc = self.lib.l2a_model_set_weights_strided(self.handle, int(first_set), count, ptrs, strides, _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_set_weights_strided")
        self._keep[("w_stacked", first_set)] = dev

    def adapt_sgd(self, base_params, x, y, lr):
        """One SGD step per task on the device, written straight into weight sets ``0 .. m-1``
        (``l2a_model_adapt_sgd``).  ``base_params``: pre-update [W0, b0, ...] CUDA tensors; ``x`` /
        ``y``: fp32 CUDA ``[m, rows, in_dim]`` / ``[m, rows, obs_dim]`` (normalised)."""
        m, rows = int(x.shape[0]), int(x.shape[1])
        assert x.is_cuda and y.is_cuda and x.dtype == torch.float32 and y.dtype == torch.float32
        assert tuple(x.shape) == (m, rows, self.obs_dim + self.act_dim) and tuple(y.shape) == (m, rows, self.obs_dim)
        base = [t.detach().to(device=self.device, dtype=torch.float32).contiguous() for t in base_params]
        ptrs = (ctypes.c_void_p * len(base))(*[t.data_ptr() for t in base])
        x, y = x.contiguous(), y.contiguous()
        rc = self.lib.l2a_model_adapt_sgd(self.handle, ptrs, _ptr(x), _ptr(y), m, rows, float(lr), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_adapt_sgd")
        self._keep["adapt"] = (base, x, y)

    def adapt_sgd_host(self, base_params, x, y, lr):
        """``adapt_sgd`` with the batches as HOST float32 arrays ``[m, rows, in_dim]`` / ``[m, rows, obs_dim]``
        (``l2a_model_adapt_sgd_host``: host-mapped staging, the launches replayed as one hipGraph)."""
        m, rows = int(x.shape[0]), int(x.shape[1])
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        assert x.shape == (m, rows, self.obs_dim + self.act_dim) and y.shape == (m, rows, self.obs_dim)
        base = self._keep.get("adapt_base")
        if base is None or base[0] is not base_params:       # same list object = same tensors: keep the graph valid
            dev = [t.detach().to(device=self.device, dtype=torch.float32).contiguous() for t in base_params]
            base = (base_params, dev, (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev]))
            self._keep["adapt_base"] = base
        rc = self.lib.l2a_model_adapt_sgd_host(self.handle, base[2], ctypes.c_void_p(x.ctypes.data),
                                               ctypes.c_void_p(y.ctypes.data), m, rows, float(lr),
                                               _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_adapt_sgd_host")

    raw_adapt_max_inputs = 128

    def adapt_sgd_raw(self, base_params, obs, act, obs_next, normalization, lr):
        """``adapt_sgd`` from the un-normalised float64 transitions ``[m, rows, dim]`` and ``normalization`` (the
        model's dict of (mean, std) pairs): the device normalises exactly as the host would
        (``l2a_model_adapt_sgd_raw``).  This wrapper sits in front of the GrBAL step's first launch: arrays and
        pointers it has seen before (the caller's stacking buffers, the normalisation vectors) are not converted again."""
        raw = self._keep.get("adapt_raw")
        if raw is None or raw[0] is not obs or raw[1] is not act or raw[2] is not obs_next:
            obs_c = np.ascontiguousarray(obs, dtype=np.float64)
            act_c = np.ascontiguousarray(act, dtype=np.float64)
            next_c = np.ascontiguousarray(obs_next, dtype=np.float64)
            m, rows = int(obs_c.shape[0]), int(obs_c.shape[1])
            assert obs_c.shape == (m, rows, self.obs_dim) and act_c.shape == (m, rows, self.act_dim) and next_c.shape == obs_c.shape
            # (identity of the CALLER's arrays is only remembered when they needed no conversion: the library copies out of
            #  them during the call, so the same buffers with new contents are fine)
            same = obs_c is obs and act_c is act and next_c is obs_next
            raw = (obs if same else None, act, obs_next, obs_c, act_c, next_c, m, rows,
                   ctypes.c_void_p(obs_c.ctypes.data), ctypes.c_void_p(act_c.ctypes.data), ctypes.c_void_p(next_c.ctypes.data))
            self._keep["adapt_raw"] = raw
        m, rows = raw[6], raw[7]
        base = self._keep.get("adapt_base")
        if base is None or base[0] is not base_params:
            dev = [t.detach().to(device=self.device, dtype=torch.float32).contiguous() for t in base_params]
            base = (base_params, dev, (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev]))
            self._keep["adapt_base"] = base
        nv = self._keep.get("adapt_norm")
        if nv is None or nv[0] is not normalization:
            vecs = [np.ascontiguousarray(normalization[k][j], dtype=np.float64) for k in ("obs", "act", "delta") for j in (0, 1)]
            assert vecs[0].shape == (self.obs_dim,) and vecs[2].shape == (self.act_dim,) and vecs[4].shape == (self.obs_dim,)
            nv = (normalization, vecs, [ctypes.c_void_p(v.ctypes.data) for v in vecs])
            self._keep["adapt_norm"] = nv
        p = nv[2]
        rc = self.lib.l2a_model_adapt_sgd_raw(self.handle, base[2], raw[8], raw[9], raw[10],
                                              p[0], p[1], p[2], p[3], p[4], p[5], m, rows, float(lr),
                                              _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_adapt_sgd_raw")

    def get_weights(self, e):
        """Weight set ``e`` as fresh CUDA tensors in the reference's order and layout."""
        sizes = (self.obs_dim + self.act_dim,) + self.hidden_sizes + (self.obs_dim,)
        out = []
        for li in range(len(sizes) - 1):
            out.append(torch.empty((sizes[li], sizes[li + 1]), dtype=torch.float32, device=self.device))
            out.append(torch.empty((sizes[li + 1],), dtype=torch.float32, device=self.device))
        ptrs = (ctypes.c_void_p * len(out))(*[t.data_ptr() for t in out])
        rc = self.lib.l2a_model_get_weights(self.handle, int(e), ptrs, _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_get_weights")
        return out

    def set_norm(self, e, norm):
        """``norm``: the reference's ``normalization`` dict (``'obs'/'act'/'delta' -> (mean, std)``)
        or ``None`` for identity."""
        if norm is None:
            null = ctypes.POINTER(ctypes.c_double)()
            rc = self.lib.l2a_model_set_norm(self.handle, int(e), null, null, null, null, null, null,
                                             _stream_ptr(self.device))
        else:
            keep, args = [], []
            for key in ("obs", "act", "delta"):
                for j in (0, 1):
                    arr, p = _dvec(norm[key][j])
                    expect = self.act_dim if key == "act" else self.obs_dim
                    assert arr.shape == (expect,), "normalization[%r] has shape %s" % (key, arr.shape)
                    keep.append(arr)
                    args.append(p)
            rc = self.lib.l2a_model_set_norm(self.handle, int(e), *args, _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_model_set_norm")

    # ---- launches -----------------------------------------------------------------------
    def plan_rs(self, obs0, actions, m, n, h, discount, reward, cand_offset=0, returns_out=None,
                best_key=None):
        """All tensor arguments are fp32 / int64 CUDA tensors; see ``l2a_plan_rs`` in include/l2a.h."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        assert isinstance(reward, RewardSpec)
        rc = self.lib.l2a_plan_rs(self.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h),
                                  float(discount), ctypes.byref(reward), int(cand_offset),
                                  _ptr(returns_out), _ptr(best_key), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_plan_rs")

    def rollout_traj(self, obs0, actions, m, n, h, cand_offset=0, traj_out=None):
        """The model's predicted trajectory of a plan (``l2a_rollout_traj``): fp32 CUDA ``[h, m * n, obs_dim]``, ``traj[t]`` = the
        observation after horizon step ``t``.  One launch of the trajectory-writing micro-tile kernel where the plan fits one
        (``_lib.mlp_traj_geometry``), else ``h`` one-step launches that hand the state on; the same bits either way."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if traj_out is None:
            traj_out = torch.empty((h, m * n, self.obs_dim), dtype=torch.float32, device=self.device)
        assert traj_out.is_cuda and traj_out.dtype == torch.float32 and traj_out.is_contiguous()
        assert traj_out.numel() == h * m * n * self.obs_dim
        rc = self.lib.l2a_rollout_traj(self.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h), int(cand_offset),
                                       _ptr(traj_out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_rollout_traj")
        return traj_out

    def plan_rs_program(self, obs0, actions, m, n, h, discount, program, cand_offset=0, returns_out=None, best_key=None,
                        traj_out=None):
        """Plan step of an env with a ``RewardProgram`` (``l2a_plan_rs_program``): the rollout of ``rollout_traj``, then the
        scoring kernel.  Arguments as ``plan_rs``; ``traj_out``: optional fp32 CUDA ``[h, m * n, obs_dim]`` that receives every
        candidate's states."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if traj_out is not None:
            assert traj_out.is_cuda and traj_out.dtype == torch.float32 and traj_out.is_contiguous()
            assert traj_out.numel() == h * m * n * self.obs_dim
        assert isinstance(program, RewardProgram)
        self.program_plans += 1
        rc = self.lib.l2a_plan_rs_program(self.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h), float(discount),
                                          ctypes.byref(program), int(cand_offset), _ptr(returns_out), _ptr(best_key),
                                          _ptr(traj_out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_plan_rs_program")

    def plan_rs_reward_model(self, obs0, actions, m, n, h, discount, reward_model, cand_offset=0, returns_out=None,
                             best_key=None, traj_out=None):
        """Plan step with a learned reward (``l2a_plan_rs_reward_model``): the rollout of ``rollout_traj``, then the
        matrix-core scorer of ``reward_model`` (a ``NativeRewardModel``).  Arguments as ``plan_rs_program``."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if traj_out is not None:
            assert traj_out.is_cuda and traj_out.dtype == torch.float32 and traj_out.is_contiguous()
            assert traj_out.numel() == h * m * n * self.obs_dim
        assert isinstance(reward_model, NativeRewardModel)
        self.reward_model_plans += 1
        rc = self.lib.l2a_plan_rs_reward_model(self.handle, reward_model.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h),
                                               float(discount), int(cand_offset), _ptr(returns_out), _ptr(best_key),
                                               _ptr(traj_out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_plan_rs_reward_model")

    def plan_rs_value(self, obs0, actions, m, n, h, discount, reward, value_model, value_coef=1.0, cand_offset=0,
                      returns_out=None, best_key=None, traj_out=None):
        """Plan step with a learned terminal value: ``R' = R + value_coef * discount ** h * V(s_h)`` (include/l2a.h, "plans with
        a learned terminal value").  ``reward``: a ``RewardSpec`` (``l2a_plan_rs_value``: the fused rollout hands out the last
        states), a ``RewardProgram`` (``l2a_plan_rs_program_value``) or a ``NativeRewardModel``
        (``l2a_plan_rs_reward_model_value``); ``value_model``: a ``NativeValueModel``.  Other arguments as ``plan_rs`` /
        ``plan_rs_program`` (``traj_out`` only with the latter two)."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if traj_out is not None:
            assert not isinstance(reward, RewardSpec), "the fused rollout writes no trajectory"
            assert traj_out.is_cuda and traj_out.dtype == torch.float32 and traj_out.is_contiguous()
            assert traj_out.numel() == h * m * n * self.obs_dim
        assert isinstance(value_model, NativeValueModel)
        self.value_plans += 1
        head = (_ptr(obs0), _ptr(actions), int(m), int(n), int(h), float(discount))
        outs = (int(cand_offset), _ptr(returns_out), _ptr(best_key))
        stream = _stream_ptr(self.device)
        if isinstance(reward, RewardSpec):
            what = "l2a_plan_rs_value"
            rc = self.lib.l2a_plan_rs_value(self.handle, value_model.handle, *(head + (ctypes.byref(reward), float(value_coef)) + outs +
                                                                               (stream,)))
        elif isinstance(reward, RewardProgram):
            what = "l2a_plan_rs_program_value"
            self.program_plans += 1
            rc = self.lib.l2a_plan_rs_program_value(self.handle, value_model.handle, *(head + (ctypes.byref(reward), float(value_coef)) +
                                                                                       outs + (_ptr(traj_out), stream)))
        elif isinstance(reward, NativeRewardModel):
            what = "l2a_plan_rs_reward_model_value"
            self.reward_model_plans += 1
            rc = self.lib.l2a_plan_rs_reward_model_value(self.handle, reward.handle, value_model.handle,
                                                         *(head + (float(value_coef),) + outs + (_ptr(traj_out), stream)))
        else:
            raise _lib.L2AError("plans with a terminal value take a RewardSpec, a RewardProgram or a NativeRewardModel, not %s"
                                % type(reward).__name__)
        self.ctx.check(rc, what)

    def policy_propose(self, policy_model, obs0, m, n, n_pi, h, seq, sigma, low, high, mirror=None, n_total=None, cand_offset=0, z=None,
                       seed=0, offset=0):
        """Overwrite the first ``n_pi`` (global index ``cand_offset + j``) candidates of every env in ``seq`` ``[h, m * n, act_dim]``
        - and in ``mirror`` ``[n_total, m, h * act_dim]`` when given - with ``policy_model`` (a ``NativePolicyModel``) rolled in
        closed loop through this model from ``obs0`` ``[m, obs_dim]`` (``l2a_policy_propose``; include/l2a.h, "policy priors").
        ``sigma`` / ``low`` / ``high``: fp32 CUDA ``[act_dim]``; ``z``: optional injected normals ``[h, m, n_pi, act_dim]``, else
        the Philox stream of (``seed``, ``offset``).  Stream-ordered."""
        if not hasattr(self.lib, "l2a_policy_propose"):
            raise _lib.L2AError("this libl2a_hip.so has no policy kernel (l2a_policy_propose): rebuild it")
        assert isinstance(policy_model, NativePolicyModel)
        n_total = int(n) if n_total is None else int(n_total)
        for t in (obs0, seq, sigma, low, high):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and seq.numel() == h * m * n * self.act_dim
        assert sigma.numel() == self.act_dim and low.numel() == self.act_dim and high.numel() == self.act_dim
        if mirror is not None:
            assert mirror.is_cuda and mirror.dtype == torch.float32 and mirror.is_contiguous()
            assert mirror.numel() == n_total * m * h * self.act_dim
        if z is not None:
            assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.numel() == h * m * n_pi * self.act_dim
        self.policy_proposals += 1
        rc = self.lib.l2a_policy_propose(self.handle, policy_model.handle, _ptr(obs0), int(m), int(n), int(n_pi), int(h),
                                         int(cand_offset), _ptr(z), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF,
                                         _ptr(sigma), _ptr(low), _ptr(high), _ptr(seq), _ptr(mirror), n_total,
                                         _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_policy_propose")

    def plan_rs_term(self, obs0, actions, m, n, h, discount, reward, termination, value_model=None, value_coef=1.0, cand_offset=0,
                     returns_out=None, steps_alive_out=None, best_key=None, traj_out=None):
        """Plan step of an env that terminates (``l2a_plan_rs_term``; include/l2a.h, "plans on envs that terminate"): every
        candidate's return stops at its first step whose next observation fails a guard of ``termination`` (a
        ``TerminationProgram``).  ``reward``: a ``RewardProgram``, a ``RewardSpec`` (scored as ``RewardProgram.from_spec``) or a
        ``NativeRewardModel``; ``value_model``: an optional ``NativeValueModel`` whose value of the last state is folded into the
        rows that survive.  ``steps_alive_out``: optional int32 CUDA ``[m, n]``.  Other arguments as ``plan_rs_program``."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if steps_alive_out is not None:
            assert steps_alive_out.is_cuda and steps_alive_out.dtype == torch.int32 and steps_alive_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if traj_out is not None:
            assert traj_out.is_cuda and traj_out.dtype == torch.float32 and traj_out.is_contiguous()
            assert traj_out.numel() == h * m * n * self.obs_dim
        assert isinstance(termination, TerminationProgram)
        assert value_model is None or isinstance(value_model, NativeValueModel)
        if not hasattr(self.lib, "l2a_plan_rs_term"):
            raise _lib.L2AError("this libl2a_hip.so has no termination kernel (l2a_plan_rs_term): rebuild it")
        rm, program = None, None
        if isinstance(reward, NativeRewardModel):
            rm = reward.handle
        elif isinstance(reward, RewardProgram):
            program = reward
        elif isinstance(reward, RewardSpec):
            program = self._spec_programs.get(id(reward))
            if program is None or program[0] is not reward:
                program = self._spec_programs[id(reward)] = (reward, RewardProgram.from_spec(reward, self.obs_dim, self.act_dim))
            program = program[1]
        else:
            raise _lib.L2AError("plans with a termination program take a RewardSpec, a RewardProgram or a NativeRewardModel, not %s"
                                % type(reward).__name__)
        self.term_plans += 1
        rc = self.lib.l2a_plan_rs_term(self.handle, rm, value_model.handle if value_model is not None else None, _ptr(obs0),
                                       _ptr(actions), int(m), int(n), int(h), float(discount),
                                       ctypes.byref(program) if program is not None else None, ctypes.byref(termination),
                                       float(value_coef), int(cand_offset), _ptr(returns_out), _ptr(steps_alive_out),
                                       _ptr(best_key), _ptr(traj_out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_plan_rs_term")

    def plan_rs_particles(self, obs0, actions, m, n, h, discount, reward, risk_coef=0.0, cand_offset=0, score_out=None,
                          spread_out=None, member_returns_out=None, best_key=None):
        """Plan step over the ensemble's particles (``l2a_plan_rs_particles`` and its two siblings): every member of this mean
        ensemble rolls every candidate out on its own, ``score_out [m, n]`` = mean of the ``n_sets`` member returns less
        ``risk_coef`` times their standard deviation (``spread_out [m, n]``); ``member_returns_out [m, n_sets, n]``.  ``reward``: a
        ``RewardSpec`` (the fused rollout), a ``RewardProgram`` or a ``NativeRewardModel`` (trajectory rollout + scoring launch).
        The other arguments as ``plan_rs``; ``best_key`` holds the arg-max of the score."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        for t, count in ((score_out, m * n), (spread_out, m * n), (member_returns_out, m * self.n_sets * n)):
            if t is not None:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == count
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if not hasattr(self.lib, "l2a_plan_rs_particles"):
            raise _lib.L2AError("this libl2a_hip.so has no particle plans (l2a_plan_rs_particles): rebuild it")
        tail = (ctypes.c_float(risk_coef), int(cand_offset), _ptr(score_out), _ptr(spread_out), _ptr(member_returns_out),
                _ptr(best_key), _stream_ptr(self.device))
        head = (self.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h), float(discount))
        if isinstance(reward, NativeRewardModel):
            self.reward_model_plans += 1
            rc = self.lib.l2a_plan_rs_particles_reward_model(self.handle, reward.handle, *(head[1:] + tail))
            what = "l2a_plan_rs_particles_reward_model"
        elif isinstance(reward, RewardProgram):
            self.program_plans += 1
            rc = self.lib.l2a_plan_rs_particles_program(*(head + (ctypes.byref(reward),) + tail))
            what = "l2a_plan_rs_particles_program"
        else:
            assert isinstance(reward, RewardSpec)
            rc = self.lib.l2a_plan_rs_particles(*(head + (ctypes.byref(reward),) + tail))
            what = "l2a_plan_rs_particles"
        self.particle_plans = getattr(self, "particle_plans", 0) + 1
        self.ctx.check(rc, what)

    def plan_rs_particles_ts1(self, obs0, actions, m, n, h, discount, reward, risk_coef=0.0, seed=0, offset=0, perm=None,
                              cand_offset=0, score_out=None, spread_out=None, particle_returns_out=None, best_key=None):
        """TS1 plan step over the ensemble's particles (``l2a_plan_rs_particles_ts1`` and its two siblings): as
        ``plan_rs_particles``, but between two horizon steps every candidate's particles are dealt anew over the members - the
        Philox permutations of ``(seed, offset)``, or ``perm``, a uint8 CUDA tensor ``[h - 1, m, n, n_sets]``.  ``reward``: a
        ``RewardSpec`` (fused into the rollout), a ``RewardProgram`` or a ``NativeRewardModel`` (scored step by step, where the
        particles are dealt).  ``particle_returns_out [m, n_sets, n]``: the returns of the particles that END in block e (row e
        is no longer member e's)."""
        assert obs0.is_cuda and actions.is_cuda and obs0.dtype == torch.float32 and actions.dtype == torch.float32
        assert obs0.is_contiguous() and actions.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and actions.numel() == h * m * n * self.act_dim
        for t, count in ((score_out, m * n), (spread_out, m * n), (particle_returns_out, m * self.n_sets * n)):
            if t is not None:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == count
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        if perm is not None:
            assert perm.is_cuda and perm.dtype == torch.uint8 and perm.is_contiguous() and perm.numel() == (h - 1) * m * n * self.n_sets
        if not hasattr(self.lib, "l2a_plan_rs_particles_ts1"):
            raise _lib.L2AError("this libl2a_hip.so has no TS1 particle plans (l2a_plan_rs_particles_ts1): rebuild it")
        head = (self.handle, _ptr(obs0), _ptr(actions), int(m), int(n), int(h), float(discount))
        tail = (ctypes.c_float(risk_coef), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), _ptr(perm), int(cand_offset), _ptr(score_out),
                _ptr(spread_out), _ptr(particle_returns_out), _ptr(best_key), _stream_ptr(self.device))
        if isinstance(reward, (NativeRewardModel, RewardProgram)):
            # the step's reward is taken at every boundary (``l2a_particle_step``), in the launch that deals the particles
            if not hasattr(self.lib, "l2a_particle_step"):
                raise _lib.L2AError("this libl2a_hip.so scores TS1 particle plans by the fused reward formula only "
                                    "(no l2a_particle_step): rebuild it")
            if isinstance(reward, NativeRewardModel):
                self.reward_model_plans += 1
                rc = self.lib.l2a_plan_rs_particles_ts1_reward_model(self.handle, reward.handle, *(head[1:] + tail))
                what = "l2a_plan_rs_particles_ts1_reward_model"
            else:
                self.program_plans += 1
                rc = self.lib.l2a_plan_rs_particles_ts1_program(*(head + (ctypes.byref(reward),) + tail))
                what = "l2a_plan_rs_particles_ts1_program"
        elif isinstance(reward, RewardSpec):
            rc = self.lib.l2a_plan_rs_particles_ts1(*(head + (ctypes.byref(reward),) + tail))
            what = "l2a_plan_rs_particles_ts1"
        else:
            raise _lib.L2AError("TS1 particle plans take a RewardSpec, a RewardProgram or a NativeRewardModel, not %s"
                                % type(reward).__name__)
        self.particle_plans = getattr(self, "particle_plans", 0) + 1
        self.ctx.check(rc, what)

    def particle_step(self, pre, post, actions, ret_out, m, n, disc_t=1.0, rewards=None, program=None, ret_in=None, state_out=None,
                      pre_per_row=True, act_env_stride=None, t=0, seed=0, offset=0, perm=None, cand_offset=0):
        """One TS1 step boundary alone (``l2a_particle_step``): the step reward of every particle - ``program`` on its ``pre``
        state, action and ``post`` state, or the given ``rewards [m, n_sets, n]`` - is added to ``ret_in`` (``None``: zero) times
        ``disc_t``, then returns and ``post`` states are dealt over the member blocks into ``ret_out`` / ``state_out`` (``None``:
        the last step, nothing is dealt).  ``pre``: ``[m, n_sets * n, obs_dim]``, or ``[m, n_sets, obs_dim]`` with
        ``pre_per_row=False``; ``actions``: env ``i``'s ``[n_sets * n, act_dim]`` at ``i * act_env_stride`` floats."""
        E = self.n_sets
        rows = m * E * n
        stride = E * n * self.act_dim if act_env_stride is None else int(act_env_stride)
        for x, count in ((pre, rows * self.obs_dim if pre_per_row else m * E * self.obs_dim), (post, rows * self.obs_dim),
                         (state_out, rows * self.obs_dim), (rewards, rows), (ret_in, rows), (ret_out, rows)):
            if x is not None:
                assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == count
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert actions.numel() >= (m - 1) * stride + E * n * self.act_dim
        if perm is not None:
            assert perm.is_cuda and perm.dtype == torch.uint8 and perm.is_contiguous() and perm.numel() == m * n * E
        assert program is None or isinstance(program, RewardProgram)
        if not hasattr(self.lib, "l2a_particle_step"):
            raise _lib.L2AError("this libl2a_hip.so has no TS1 step kernel (l2a_particle_step): rebuild it")
        rc = self.lib.l2a_particle_step(self.ctx.handle, _ptr(pre), 1 if pre_per_row else 0, _ptr(post), _ptr(actions), stride,
                                        _ptr(rewards), None if program is None else ctypes.byref(program), float(disc_t),
                                        _ptr(ret_in), _ptr(state_out), _ptr(ret_out), _ptr(perm), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        int(offset), int(t), int(m), E, int(n), self.obs_dim, self.act_dim, int(cand_offset),
                                        _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_particle_step")

    def particle_shuffle(self, state_in, ret_in, state_out, ret_out, m, n, t=0, seed=0, offset=0, perm=None, cand_offset=0):
        """The TS1 shuffle alone (``l2a_particle_shuffle``): fp32 CUDA states ``[m, n_sets * n, obs_dim]`` and returns
        ``[m, n_sets, n]``, out of place; ``perm``: uint8 CUDA ``[m, n, n_sets]`` or ``None`` (Philox of ``seed, offset, t``)."""
        E = self.n_sets
        for x, count in ((state_in, m * E * n * self.obs_dim), (state_out, m * E * n * self.obs_dim), (ret_in, m * E * n),
                         (ret_out, m * E * n)):
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == count
        if perm is not None:
            assert perm.is_cuda and perm.dtype == torch.uint8 and perm.is_contiguous() and perm.numel() == m * n * E
        if not hasattr(self.lib, "l2a_particle_shuffle"):
            raise _lib.L2AError("this libl2a_hip.so has no particle shuffle (l2a_particle_shuffle): rebuild it")
        rc = self.lib.l2a_particle_shuffle(self.ctx.handle, _ptr(state_in), _ptr(ret_in), _ptr(state_out), _ptr(ret_out), _ptr(perm),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), int(t), int(m), E, int(n), self.obs_dim,
                                           int(cand_offset), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_particle_shuffle")

    def particle_score(self, member_returns, m, n_members, n, risk_coef=0.0, cand_offset=0, score_out=None, spread_out=None,
                       best_key=None):
        """The particle scorer alone (``l2a_particle_score``) on fp32 CUDA ``member_returns [m, n_members, n]``."""
        assert member_returns.is_cuda and member_returns.dtype == torch.float32 and member_returns.is_contiguous()
        assert member_returns.numel() == m * n_members * n
        rc = self.lib.l2a_particle_score(self.ctx.handle, _ptr(member_returns), int(m), int(n_members), int(n),
                                         ctypes.c_float(risk_coef), int(cand_offset), _ptr(score_out), _ptr(spread_out),
                                         _ptr(best_key), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_particle_score")

    def plan_rs_sync(self, obs_host, actions, m, n, h, discount, reward, cand_offset=0, returns_out=None):
        """Blocking plan step (``l2a_plan_rs_sync``): ``obs_host`` is a HOST array ``[m, obs_dim]``; returns the
        arg-max keys as a NumPy uint64 array ``[m]``, or ``None`` when the launch was flagged invalid (tile-split
        partner missing) - the context has then been switched to the unsplit geometry and the caller repeats the
        call.  ctypes releases the GIL for the duration, so other Python threads run while the GPU plans."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert actions.numel() == h * m * n * self.act_dim
        obs = np.ascontiguousarray(obs_host, dtype=np.float32)
        assert obs.size == m * self.obs_dim
        keys = np.empty(m, dtype=np.uint64)
        rc = self.lib.l2a_plan_rs_sync(self.handle, ctypes.c_void_p(obs.ctypes.data), _ptr(actions), int(m), int(n),
                                       int(h), float(discount), ctypes.byref(reward), int(cand_offset),
                                       _ptr(returns_out), ctypes.c_void_p(keys.ctypes.data), _stream_ptr(self.device))
        if rc == _lib.L2A_ESPLIT:
            if getattr(self.ctx, "split_degraded", False):
                raise _lib.L2AError("rollout launch was flagged invalid with the tile split disabled")
            self.ctx.set_split(0)
            self.ctx.split_degraded = True
            return None
        self.ctx.check(rc, "l2a_plan_rs_sync")
        return keys

    sync_max_envs = 64

    def plan_payload(self, best_key, m, digest, payload):
        """Pack what a sharded plan all-reduces (``l2a_plan_payload``): keys, this rank's launch flag, the digest pair -
        on the device, in stream order behind the launch, no host synchronisation."""
        self.ctx.plan_payload(best_key, m, digest, payload, _stream_ptr(self.device))

    def plan_rs_chunk(self, state, state_per_row, actions, m, n, h_chunk, t0, discount, reward, cand_offset=0,
                      returns_in=None, returns_out=None, state_out=None, best_key=None):
        """Horizon steps ``t0 .. t0 + h_chunk - 1`` of a plan (``l2a_plan_rs_chunk``); all tensors fp32 CUDA."""
        assert state.is_cuda and actions.is_cuda and state.is_contiguous() and actions.is_contiguous()
        assert actions.numel() == h_chunk * m * n * self.act_dim
        assert state.numel() == (m * n if state_per_row else m) * self.obs_dim
        assert returns_out is not None and returns_out.numel() == m * n
        assert isinstance(reward, RewardSpec)
        rc = self.lib.l2a_plan_rs_chunk(self.handle, _ptr(state), 1 if state_per_row else 0, _ptr(actions), int(m), int(n),
                                        int(h_chunk), int(t0), float(discount), ctypes.byref(reward), int(cand_offset),
                                        _ptr(returns_in), _ptr(returns_out), _ptr(state_out), _ptr(best_key),
                                        _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_plan_rs_chunk")

    def predict(self, obs, act, n_blocks=1, out=None):
        assert obs.is_cuda and act.is_cuda and obs.dtype == torch.float32 and act.dtype == torch.float32
        rows = obs.shape[0]
        if out is None:
            out = torch.empty((rows, self.obs_dim), dtype=torch.float32, device=self.device)
        rc = self.lib.l2a_predict(self.handle, _ptr(obs.contiguous()), _ptr(act.contiguous()), int(rows),
                                  int(n_blocks), _ptr(out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_predict")
        return out


class _NativeHead(object):
    """What the handles on the three matrix-core MLP heads share (``csrc/l2a_rm_net.hip``): construction, ``close``, and the
    marshalling of ``set_weights`` and ``set_norm``.  A subclass names its C entry points (``_prefix`` + ``_create`` /
    ``_destroy`` / ``_set_weights`` / ``_set_norm``) and itself in messages (``_what``), and supplies ``_sizes()`` - the layer
    widths, input first - and ``_norm_spec()`` - the ``(key, length)`` pairs of its normalisation dict, in the C argument order."""

    _prefix = None
    _what = None

    def __init__(self, dims, hidden_sizes, hidden_act, device=None):
        if not torch.cuda.is_available():
            raise _lib.L2AError("no MI355X visible to PyTorch-ROCm: the %s is HIP-only (there is no CPU fallback)" % self._what)
        if device is None:
            device = torch.cuda.current_device()
        self.ctx = _lib.Context.get(device)
        self.lib = self.ctx.lib
        if not hasattr(self.lib, self._prefix + "_create"):
            raise _lib.L2AError("this libl2a_hip.so has no %s (%s_create): rebuild it" % (self._what, self._prefix))
        self.device = torch.device("cuda", device)
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        if hidden_act not in _lib.ACT_CODES:
            raise _lib.L2AError("nonlinearity %r is not supported by the HIP kernels" % (hidden_act,))
        hid = (ctypes.c_int * len(self.hidden_sizes))(*self.hidden_sizes)
        handle = ctypes.c_void_p()
        args = tuple(dims) + (len(self.hidden_sizes), hid, _lib.ACT_CODES[hidden_act], ctypes.byref(handle))
        self._call("_create", self.ctx.handle, *args)
        self.handle = handle
        self._keep = {}

    def _call(self, suffix, *args):
        """``l2a_<head>_model<suffix>(*args)``, checked."""
        self.ctx.check(getattr(self.lib, self._prefix + suffix)(*args), self._prefix + suffix)

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.lib, self._prefix + "_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, params):
        """``params``: [W0, b0, ..., Wout, bout], kernels ``[in, out]`` of the widths ``_sizes()``."""
        dev = []
        for p in params:
            t = torch.as_tensor(p) if not torch.is_tensor(p) else p
            dev.append(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        sizes = self._sizes()
        assert len(dev) == 2 * (len(sizes) - 1), "expected %d parameter arrays" % (2 * (len(sizes) - 1))
        for li in range(len(sizes) - 1):
            assert tuple(dev[2 * li].shape) == (sizes[li], sizes[li + 1]), \
                "kernel %d has shape %s, expected %s" % (li, tuple(dev[2 * li].shape), (sizes[li], sizes[li + 1]))
            assert tuple(dev[2 * li + 1].shape) == (sizes[li + 1],)
        ptrs = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        self._call("_set_weights", self.handle, ptrs, _stream_ptr(self.device))
        self._keep["w"] = dev

    def set_norm(self, norm):
        """``norm``: dict ``key -> (mean, std)`` over the keys of ``_norm_spec()``, or ``None`` for identity."""
        spec = self._norm_spec()
        if norm is None:
            args = [ctypes.POINTER(ctypes.c_double)()] * (2 * len(spec))
        else:
            keep, args = [], []
            for key, expect in spec:
                for j in (0, 1):
                    arr, p = _dvec(np.reshape(norm[key][j], -1))
                    assert arr.shape == (expect,), "normalization[%r] has shape %s" % (key, arr.shape)
                    keep.append(arr)
                    args.append(p)
        self._call("_set_norm", self.handle, *(args + [_stream_ptr(self.device)]))


class NativeRewardModel(_NativeHead):
    """Python handle on an ``l2a_reward_model``: a reward MLP over ``[obs | act | next_obs - obs]`` that the planner scores
    trajectories with on the matrix cores (``csrc/l2a_score_mlp.hip``).  Raises ``L2AError`` on any failure.  ``set_weights``:
    the first ``in`` is ``2 * obs_dim + act_dim``, the last ``out`` is 1.  ``set_norm``: ``'obs' / 'act' / 'delta' / 'reward' ->
    (mean, std)`` (reward: scalars)."""

    _prefix, _what = "l2a_reward_model", "reward scorer"

    def __init__(self, obs_dim, act_dim, hidden_sizes, hidden_act, device=None):
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        _NativeHead.__init__(self, (self.obs_dim, self.act_dim), hidden_sizes, hidden_act, device)

    def _sizes(self):
        return (2 * self.obs_dim + self.act_dim,) + self.hidden_sizes + (1,)

    def _norm_spec(self):
        return (("obs", self.obs_dim), ("act", self.act_dim), ("delta", self.obs_dim), ("reward", 1))

    def predict(self, obs, act, next_obs, out=None):
        """fp32 CUDA ``[rows, obs_dim]``, ``[rows, act_dim]``, ``[rows, obs_dim]`` -> fp32 CUDA ``[rows]``."""
        for t in (obs, act, next_obs):
            assert t.is_cuda and t.dtype == torch.float32
        rows = int(obs.shape[0])
        assert tuple(obs.shape) == (rows, self.obs_dim) == tuple(next_obs.shape) and tuple(act.shape) == (rows, self.act_dim)
        if out is None:
            out = torch.empty((rows,), dtype=torch.float32, device=self.device)
        rc = self.lib.l2a_reward_model_predict(self.handle, _ptr(obs.contiguous()), _ptr(act.contiguous()),
                                               _ptr(next_obs.contiguous()), rows, _ptr(out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_reward_model_predict")
        return out

    def score_trajectory(self, obs0, traj, actions, m, n, h, discount, cand_offset=0, returns_out=None, best_key=None):
        """The scorer alone (``l2a_score_trajectory_model``) on trajectories that are already on the device: ``obs0``
        ``[m, obs_dim]``, ``traj`` ``[h, m * n, obs_dim]``, ``actions`` ``[h, m * n, act_dim]`` fp32 CUDA tensors."""
        for t in (obs0, traj, actions):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert obs0.numel() == m * self.obs_dim and traj.numel() == h * m * n * self.obs_dim
        assert actions.numel() == h * m * n * self.act_dim
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        rc = self.lib.l2a_score_trajectory_model(self.handle, _ptr(obs0), _ptr(traj), _ptr(actions), int(m), int(n), int(h),
                                                 float(discount), int(cand_offset), _ptr(returns_out), _ptr(best_key),
                                                 _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_score_trajectory_model")


class NativePolicyModel(_NativeHead):
    """Python handle on an ``l2a_policy_model``: a policy MLP over the observation that proposes planning candidates, evaluated
    on the matrix cores (``csrc/l2a_policy.hip``).  Raises ``L2AError`` on any failure.  ``set_weights``: the first ``in`` is
    ``obs_dim``, the last ``out`` is ``act_dim``.  ``set_norm``: ``'obs' / 'act' -> (mean, std)``."""

    _prefix, _what = "l2a_policy_model", "policy kernel"

    def __init__(self, obs_dim, act_dim, hidden_sizes, hidden_act, device=None):
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        _NativeHead.__init__(self, (self.obs_dim, self.act_dim), hidden_sizes, hidden_act, device)

    def _sizes(self):
        return (self.obs_dim,) + self.hidden_sizes + (self.act_dim,)

    def _norm_spec(self):
        return (("obs", self.obs_dim), ("act", self.act_dim))

    def act(self, states, sigma, low, high, z=None, seed=0, offset=0, out=None):
        """The kernel alone (``l2a_policy_act``): fp32 CUDA ``[rows, obs_dim]`` -> fp32 CUDA ``[rows, act_dim]``.  ``sigma`` /
        ``low`` / ``high``: fp32 CUDA ``[act_dim]``; ``z``: optional normals ``[rows, act_dim]``, else the Philox stream."""
        rows = int(states.shape[0])
        for t in (states, sigma, low, high):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert tuple(states.shape) == (rows, self.obs_dim)
        assert sigma.numel() == self.act_dim and low.numel() == self.act_dim and high.numel() == self.act_dim
        if z is not None:
            assert z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and z.numel() == rows * self.act_dim
        if out is None:
            out = torch.empty((rows, self.act_dim), dtype=torch.float32, device=self.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == rows * self.act_dim
        rc = self.lib.l2a_policy_act(self.handle, _ptr(states), rows, _ptr(z), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     int(offset) & 0xFFFFFFFFFFFFFFFF, _ptr(sigma), _ptr(low), _ptr(high), _ptr(out),
                                     _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_policy_act")
        return out


class NativeValueModel(_NativeHead):
    """Python handle on an ``l2a_value_model``: a value MLP over the observation that the planner adds, evaluated on every
    candidate's last predicted state, to the returns on the matrix cores (``csrc/l2a_value.hip``).  Raises ``L2AError`` on any
    failure.  ``set_weights``: the first ``in`` is ``obs_dim``, the last ``out`` is 1.  ``set_norm``: ``'obs' / 'value' ->
    (mean, std)`` (value: scalars)."""

    _prefix, _what = "l2a_value_model", "value kernel"

    def __init__(self, obs_dim, hidden_sizes, hidden_act, device=None):
        self.obs_dim = int(obs_dim)
        _NativeHead.__init__(self, (self.obs_dim,), hidden_sizes, hidden_act, device)

    def _sizes(self):
        return (self.obs_dim,) + self.hidden_sizes + (1,)

    def _norm_spec(self):
        return (("obs", self.obs_dim), ("value", 1))

    def predict(self, states, out=None):
        """fp32 CUDA ``[rows, obs_dim]`` -> fp32 CUDA ``[rows]``."""
        assert states.is_cuda and states.dtype == torch.float32
        rows = int(states.shape[0])
        assert tuple(states.shape) == (rows, self.obs_dim)
        if out is None:
            out = torch.empty((rows,), dtype=torch.float32, device=self.device)
        rc = self.lib.l2a_value_model_predict(self.handle, _ptr(states.contiguous()), rows, _ptr(out), _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_value_model_predict")
        return out

    def terminal(self, final_state, returns_in, m, n, h, discount, value_coef=1.0, cand_offset=0, returns_out=None, best_key=None):
        """The fold alone (``l2a_value_terminal``): ``final_state`` ``[m * n, obs_dim]`` and ``returns_in`` ``[m, n]`` fp32 CUDA
        tensors -> ``returns_out`` (may be ``returns_in``) and / or ``best_key``."""
        for t in (final_state, returns_in):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert final_state.numel() == m * n * self.obs_dim and returns_in.numel() == m * n
        if returns_out is not None:
            assert returns_out.is_cuda and returns_out.dtype == torch.float32 and returns_out.numel() == m * n
        if best_key is not None:
            assert best_key.is_cuda and best_key.dtype == torch.int64 and best_key.numel() == m
        rc = self.lib.l2a_value_terminal(self.handle, _ptr(final_state), _ptr(returns_in), int(m), int(n), int(h), float(discount),
                                         float(value_coef), int(cand_offset), _ptr(returns_out), _ptr(best_key),
                                         _stream_ptr(self.device))
        self.ctx.check(rc, "l2a_value_terminal")
