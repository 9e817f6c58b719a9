"""``MLPValueModel`` - a learned terminal value for ``MPCController(value_model=..., terminal_value_coef=...)``.

A planner stops counting reward at the last horizon step; the usual remedy for a short horizon is a learned value of the last
predicted state added to the return (POLO, Lowrey et al. 2019; TD-MPC, Hansen et al. 2022):

    R' = R + terminal_value_coef * discount ** h * V(s_h)

The reference has no such class; this one follows ``MLPRewardModel``'s conventions (constructor keywords, nonlinearities as
strings, ``fit`` / ``predict`` / ``normalization``, pickling), and its semantics are the ones DESIGN section 2 fixes:

    x = (obs - mu_obs) / (sd_obs + 1e-10)
    v = MLP(x) * (sd_v + 1e-10) + mu_v                  (linear scalar output layer)

* ``predict`` (float64 ``[rows]``) runs on the MI355X through ``l2a_value_model_predict``.
* The planner does not call ``predict``: ``MPCController`` asks for the native handle (``planner_value_model()``) and folds the
  value of every candidate's last predicted state into the returns with it (``l2a_plan_rs_value`` and its siblings).
* ``fit`` is stock PyTorch (Adam on the MSE of the normalised target); training is not part of the hot path.  The targets are
  the caller's: ``returns_to_go`` turns one path's rewards into Monte-Carlo targets.
"""

from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from ..utils.serializable import Serializable
from . import core


class MLPValueModel(Serializable):
    """Feed-forward model of the normalised value of an observation."""

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

        hidden_nonlinearity = core.nonlinearity_name(hidden_nonlinearity)
        if hidden_nonlinearity not in self._activations:
            raise ValueError("unsupported nonlinearity %r (supported: %s)" % (hidden_nonlinearity, self._activations))
        self.hidden_sizes = tuple(int(h) for h in hidden_sizes)
        self.hidden_nonlinearity = hidden_nonlinearity

        sizes = (self.obs_space_dims,) + self.hidden_sizes + (1,)
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
        """``normalization``: dict ``'obs' / 'value' -> (mean, std)`` (value: scalars)."""
        self.normalization = normalization
        self._native_dirty = True

    def _norm(self):
        if not self.normalize_input:
            return None
        assert self.normalization is not None, "value model has no normalization yet (call fit first)"
        return self.normalization

    def native_eligible(self):
        """``None`` when the terminal-value kernel takes this network (``l2a_value_model_check``, host only), else the reason."""
        return _lib.value_model_check(self.obs_space_dims, self.hidden_sizes, _lib.ACT_CODES.get(self.hidden_nonlinearity, -1))

    def planner_value_model(self):
        """Return the up-to-date ``NativeValueModel`` (creates / refreshes the HBM copy lazily)."""
        from .native_model import NativeValueModel
        if self._native is None:
            self._native = NativeValueModel(self.obs_space_dims, self.hidden_sizes, self.hidden_nonlinearity)
            self._native_dirty = True
        if self._native_dirty:
            self._native.set_weights(self._params)
            self._native.set_norm(self._norm())
            self._native_dirty = False
        return self._native

    # ------------------------------------------------------------------ predict
    def predict(self, obs):
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims
        native = self.planner_value_model()
        o = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(native.device)
        values = native.predict(o).cpu().numpy().astype(np.float64)
        assert values.ndim == 1
        return values

    # ------------------------------------------------------------------ fit
    @staticmethod
    def returns_to_go(rewards, discount):
        """One path's Monte-Carlo targets: ``G[t] = sum_{k >= t} discount ** (k - t) * rewards[k]`` (float64)."""
        rewards = np.asarray(rewards, dtype=np.float64).reshape(-1)
        out = np.zeros_like(rewards)
        acc = 0.0
        for t in range(rewards.shape[0] - 1, -1, -1):
            acc = rewards[t] + float(discount) * acc
            out[t] = acc
        return out

    def compute_normalization(self, obs, targets):
        """``MLPDynamicsModel.compute_normalization``'s recipe for the observation, plus the target's mean and standard deviation."""
        assert obs.shape[0] == targets.shape[0]
        norm = OrderedDict()
        norm["obs"] = (np.mean(obs, axis=0), np.std(obs, axis=0))
        norm["value"] = (float(np.mean(targets)), float(np.std(targets)))
        self.set_normalization(norm)

    def _features(self, obs):
        if not self.normalize_input:
            return np.asarray(obs, dtype=np.float64)
        return core.normalize(obs, *self.normalization["obs"])

    def _targets(self, targets):
        if not self.normalize_input:
            return np.asarray(targets, dtype=np.float64)
        return core.normalize(np.asarray(targets, dtype=np.float64), *self.normalization["value"])

    def fit(self, obs, targets, epochs=100, compute_normalization=True, valid_split_ratio=None, verbose=False):
        """Adam on the mean squared error of the normalised target, shuffled mini-batches of ``batch_size``; returns the last
        epoch's training and validation losses."""
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims
        targets = np.asarray(targets, dtype=np.float64).reshape(-1)
        assert targets.shape[0] == obs.shape[0]
        if valid_split_ratio is None:
            valid_split_ratio = self.valid_split_ratio
        assert 1 > valid_split_ratio >= 0
        if (self.normalization is None or compute_normalization) and self.normalize_input:
            self.compute_normalization(obs, targets)
        x, y = self._features(obs), self._targets(targets)

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
                pred = core.mlp_forward(x_tr[idx], params, self.hidden_nonlinearity, None)[:, 0]
                loss = torch.mean((y_tr[idx] - pred) ** 2)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            train_loss = float(np.mean(losses)) if losses else float("nan")
            with torch.no_grad():
                if x_te.shape[0] > 0:
                    valid_loss = float(torch.mean((y_te - core.mlp_forward(x_te, params, self.hidden_nonlinearity, None)[:, 0]) ** 2))
                else:
                    valid_loss = train_loss
            if verbose:
                print("Training ValueModel - epoch %i -- train loss: %.5f  valid loss: %.5f" % (epoch, train_loss, valid_loss))
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
