"""``MLPPolicyModel`` - a learned policy prior for ``MPCController(policy_model=..., policy_candidates=..., policy_noise=...)``.

TD-MPC (Hansen et al. 2022), LOOP (Sikchi et al. 2021) and POPLIN (Wang & Ba 2020) draw a small share of every planning
population from a learned policy rolled in closed loop through the dynamics model,

    a_t = pi(s_t) + sigma * eps,        s_{t+1} = f(s_t, a_t),

instead of from noise around the plan mean.  The reference has no such class; this one follows ``MLPValueModel``'s conventions
(constructor keywords, nonlinearities as strings, ``fit`` / ``predict`` / ``normalization``, pickling), and its semantics are
the ones DESIGN section 4.16 fixes:

    x = (obs - mu_obs) / (sd_obs + 1e-10)
    a = MLP(x) * (sd_act + 1e-10) + mu_act              (linear output layer of act_dim units)

* ``predict`` (float64 ``[rows, act_dim]``) is the host restatement of those two lines; it needs no GPU.
* The planner does not call ``predict``: ``MPCController`` asks for the native handle (``planner_policy_model()``) and has the
  library roll the policy through the dynamics model on the GPU (``l2a_policy_propose``).
* ``fit`` is stock PyTorch behaviour cloning (Adam on the MSE of the normalised action); training is not part of the hot path.
"""

from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from ..utils.serializable import Serializable
from . import core


class MLPPolicyModel(Serializable):
    """Feed-forward model of the normalised action for an observation."""

    _activations = core.ACTIVATION_NAMES

    def __init__(self,
                 name,
                 env,
                 hidden_sizes=(256, 256),
                 hidden_nonlinearity="relu",
                 batch_size=500,
                 learning_rate=0.001,
                 normalize_input=True,
                 valid_split_ratio=0.2,
                 init_seed=None,
                 ):
        Serializable.quick_init(self, locals())

        self.name = name
        self.normalization = None
        self.normalize_input = normalize_input
        self.valid_split_ratio = valid_split_ratio
        self.batch_size = batch_size
        self.learning_rate = learning_rate

        self.obs_space_dims = int(env.observation_space.shape[0])
        self.action_space_dims = int(env.action_space.shape[0])

        hidden_nonlinearity = core.nonlinearity_name(hidden_nonlinearity)
        if hidden_nonlinearity not in self._activations:
            raise ValueError("unsupported nonlinearity %r (supported: %s)" % (hidden_nonlinearity, self._activations))
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity

        sizes = (self.obs_space_dims,) + self.hidden_sizes + (self.action_space_dims,)
        self._params = core.xavier_params(sizes, np.random.RandomState(init_seed))
        self._native = None
        self._native_dirty = True

    # ------------------------------------------------------------------ parameters
    def get_param_values(self):
        names = core.param_names(len(self.hidden_sizes))
        return OrderedDict((k, p.numpy().copy()) for k, p in zip(names, self._params))

    def set_params(self, params):
        """``params``: OrderedDict name -> array (``hidden_0/kernel`` ... ``output/bias``) or flat list."""
        self._params = core.as_param_list(params, len(self.hidden_sizes))
        self._native_dirty = True

    def set_normalization(self, normalization):
        """``normalization``: dict ``'obs' / 'act' -> (mean, std)``."""
        self.normalization = normalization
        self._native_dirty = True

    def _norm(self):
        if not self.normalize_input:
            return None
        assert self.normalization is not None, "policy model has no normalization yet (call fit first)"
        return self.normalization

    def native_eligible(self):
        """``None`` when the policy kernel takes this network (``l2a_policy_model_check``, host only), else the reason."""
        return _lib.policy_model_check(self.obs_space_dims, self.action_space_dims, self.hidden_sizes,
                                       _lib.ACT_CODES.get(self.hidden_nonlinearity, -1))

    def planner_policy_model(self):
        """Return the up-to-date ``NativePolicyModel`` (creates / refreshes the HBM copy lazily)."""
        from .native_model import NativePolicyModel
        if self._native is None:
            self._native = NativePolicyModel(self.obs_space_dims, self.action_space_dims, self.hidden_sizes, self.hidden_nonlinearity)
            self._native_dirty = True
        if self._native_dirty:
            self._native.set_weights(self._params)
            self._native.set_norm(self._norm())
            self._native_dirty = False
        return self._native

    # ------------------------------------------------------------------ predict
    def predict(self, obs):
        """float64 ``[rows, act_dim]``: the formulas above on the host (no noise, no clipping)."""
        obs = np.asarray(obs, dtype=np.float64)
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims
        norm = self._norm()
        x = obs if norm is None else (obs - np.asarray(norm["obs"][0], np.float64)) / (np.asarray(norm["obs"][1], np.float64) + 1e-10)
        params = [p.detach().to(torch.float64) for p in self._params]
        y = core.mlp_forward(torch.from_numpy(np.ascontiguousarray(x)), params, self.hidden_nonlinearity, None).numpy()
        if norm is None:
            return y
        return y * (np.asarray(norm["act"][1], np.float64) + 1e-10) + np.asarray(norm["act"][0], np.float64)

    # ------------------------------------------------------------------ fit
    def compute_normalization(self, obs, act):
        """``MLPDynamicsModel.compute_normalization``'s recipe for the observation and the action."""
        assert obs.shape[0] == act.shape[0]
        norm = OrderedDict()
        norm["obs"] = (np.mean(obs, axis=0), np.std(obs, axis=0))
        norm["act"] = (np.mean(act, axis=0), np.std(act, axis=0))
        self.set_normalization(norm)

    def _features(self, obs):
        if not self.normalize_input:
            return np.asarray(obs, dtype=np.float64)
        return core.normalize(obs, *self.normalization["obs"])

    def _targets(self, act):
        if not self.normalize_input:
            return np.asarray(act, dtype=np.float64)
        return core.normalize(np.asarray(act, dtype=np.float64), *self.normalization["act"])

    def fit(self, obs, act, epochs=100, compute_normalization=True, valid_split_ratio=None, verbose=False):
        """Behaviour cloning: Adam on the mean squared error of the normalised action, shuffled mini-batches of ``batch_size``;
        returns the last epoch's training and validation losses."""
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims
        assert act.ndim == 2 and act.shape == (obs.shape[0], self.action_space_dims)
        if valid_split_ratio is None:
            valid_split_ratio = self.valid_split_ratio
        assert 1 > valid_split_ratio >= 0
        if (self.normalization is None or compute_normalization) and self.normalize_input:
            self.compute_normalization(obs, act)
        x, y = self._features(obs), self._targets(act)

        perm = np.arange(x.shape[0])
        np.random.shuffle(perm)
        split = int(x.shape[0] * (1 - valid_split_ratio))
        tr, te = perm[:split], perm[split:]
        dev = core.training_device()
        x_tr = torch.as_tensor(x[tr], dtype=torch.float32, device=dev)
        y_tr = torch.as_tensor(y[tr], dtype=torch.float32, device=dev)
        x_te = torch.as_tensor(x[te], dtype=torch.float32, device=dev)
        y_te = torch.as_tensor(y[te], dtype=torch.float32, device=dev)

        params = [p.to(dev).requires_grad_(True) for p in self._params]
        opt = core.TFAdam(params, lr=self.learning_rate)
        train_loss, valid_loss = float("nan"), float("nan")
        for epoch in range(epochs):
            order = torch.randperm(x_tr.shape[0], device=dev)
            losses = []
            for s in range(0, x_tr.shape[0], self.batch_size):
                idx = order[s:s + self.batch_size]
                pred = core.mlp_forward(x_tr[idx], params, self.hidden_nonlinearity, None)
                loss = torch.mean((y_tr[idx] - pred) ** 2)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            train_loss = float(np.mean(losses)) if losses else float("nan")
            with torch.no_grad():
                if x_te.shape[0] > 0:
                    valid_loss = float(torch.mean((y_te - core.mlp_forward(x_te, params, self.hidden_nonlinearity, None)) ** 2))
                else:
                    valid_loss = train_loss
            if verbose:
                print("Training PolicyModel - epoch %i -- train loss: %.5f  valid loss: %.5f" % (epoch, train_loss, valid_loss))
        self._params = [p.detach().to("cpu").contiguous() for p in params]
        self._native_dirty = True
        self.fit_stats = dict(TrainLoss=train_loss, ValidLoss=valid_loss, Epochs=epochs)
        return self.fit_stats

    # ------------------------------------------------------------------ pickling
    def __getstate__(self):
        state = dict()
        state["init_args"] = Serializable.__getstate__(self)
        state["normalization"] = self.normalization
        state["network_params"] = self.get_param_values()
        return state

    def __setstate__(self, state):
        Serializable.__setstate__(self, state["init_args"])
        self.normalization = state["normalization"]
        self.set_params(state["network_params"])
