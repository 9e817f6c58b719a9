"""``MLPRewardModel`` - a learned reward for ``MPCController(reward_model=..., use_reward_model=True)``.

The reference's controller keeps the two keywords and calls ``self.reward_model.predict(obs, act, next_obs)`` in its
horizon loop (``policies/mpc_controller.py:121-123``) but ships no class to pass; this is one.  It follows
``MLPDynamicsModel``'s conventions (constructor keywords, nonlinearities as strings, ``fit`` / ``predict`` /
``normalization``, pickling), and its semantics are the ones DESIGN section 2 fixes:

    x = [ (obs - mu_obs) / (sd_obs + 1e-10) | (act - mu_act) / (sd_act + 1e-10) | ((next_obs - obs) - mu_d) / (sd_d + 1e-10) ]
    r = MLP(x) * (sd_r + 1e-10) + mu_r                  (linear scalar output layer)

* ``predict`` (the reference's contract: float64 ``[rows]``) runs on the MI355X through ``l2a_reward_model_predict``.
* The planner does not call ``predict`` per horizon step: ``MPCController`` asks for the native handle
  (``planner_reward_model()``) and scores whole trajectories with it (``l2a_plan_rs_reward_model``).
* ``fit`` is stock PyTorch (Adam on the MSE of the normalised reward); training is not part of the hot path.
"""

from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from ..utils.serializable import Serializable
from . import core


class MLPRewardModel(Serializable):
    """Feed-forward model of the normalised reward of a transition."""

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

        sizes = (2 * self.obs_space_dims + self.action_space_dims,) + self.hidden_sizes + (1,)
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
        """``normalization``: dict ``'obs' / 'act' / 'delta' / 'reward' -> (mean, std)`` (reward: scalars)."""
        self.normalization = normalization
        self._native_dirty = True

    def _norm(self):
        if not self.normalize_input:
            return None
        assert self.normalization is not None, "reward model has no normalization yet (call fit first)"
        return self.normalization

    def native_eligible(self):
        """``None`` when the matrix-core scorer takes this network (``l2a_reward_model_check``, host only), else the reason."""
        return _lib.reward_model_check(self.obs_space_dims, self.action_space_dims, self.hidden_sizes,
                                       _lib.ACT_CODES.get(self.hidden_nonlinearity, -1))

    def planner_reward_model(self):
        """Return the up-to-date ``NativeRewardModel`` (creates / refreshes the HBM copy lazily)."""
        from .native_model import NativeRewardModel
        if self._native is None:
            self._native = NativeRewardModel(self.obs_space_dims, self.action_space_dims, self.hidden_sizes,
                                             self.hidden_nonlinearity)
            self._native_dirty = True
        if self._native_dirty:
            self._native.set_weights(self._params)
            self._native.set_norm(self._norm())
            self._native_dirty = False
        return self._native

    # ------------------------------------------------------------------ predict (reference mpc_controller.py:123)
    def predict(self, obs, act, next_obs):
        assert obs.shape[0] == act.shape[0] == next_obs.shape[0]
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims and next_obs.shape == obs.shape
        assert act.ndim == 2 and act.shape[1] == self.action_space_dims
        native = self.planner_reward_model()
        o = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(native.device)
        a = torch.from_numpy(np.ascontiguousarray(act, dtype=np.float32)).to(native.device)
        nx = torch.from_numpy(np.ascontiguousarray(next_obs, dtype=np.float32)).to(native.device)
        rewards = native.predict(o, a, nx).cpu().numpy().astype(np.float64)
        assert rewards.ndim == 1
        return rewards

    # ------------------------------------------------------------------ fit
    def compute_normalization(self, obs, act, obs_next, rewards):
        """``MLPDynamicsModel.compute_normalization``'s recipe, plus the reward's mean and standard deviation."""
        assert obs.shape[0] == obs_next.shape[0] == act.shape[0] == rewards.shape[0]
        delta = obs_next - obs
        norm = OrderedDict()
        norm["obs"] = (np.mean(obs, axis=0), np.std(obs, axis=0))
        norm["delta"] = (np.mean(delta, axis=0), np.std(delta, axis=0))
        norm["act"] = (np.mean(act, axis=0), np.std(act, axis=0))
        norm["reward"] = (float(np.mean(rewards)), float(np.std(rewards)))
        self.set_normalization(norm)

    def _features(self, obs, act, obs_next):
        if not self.normalize_input:
            return np.concatenate([obs, act, obs_next - obs], axis=1)
        nm = self.normalization
        return np.concatenate([core.normalize(obs, *nm["obs"]), core.normalize(act, *nm["act"]),
                               core.normalize(obs_next - obs, *nm["delta"])], axis=1)

    def _targets(self, rewards):
        if not self.normalize_input:
            return np.asarray(rewards, dtype=np.float64)
        return core.normalize(np.asarray(rewards, dtype=np.float64), *self.normalization["reward"])

    def fit(self, obs, act, obs_next, rewards, epochs=100, compute_normalization=True, valid_split_ratio=None, verbose=False):
        """Adam on the mean squared error of the normalised reward, shuffled mini-batches of ``batch_size``; returns the
        last epoch's training and validation losses."""
        assert obs.ndim == 2 and obs.shape[1] == self.obs_space_dims and obs_next.shape == obs.shape
        assert act.ndim == 2 and act.shape[1] == self.action_space_dims
        rewards = np.asarray(rewards, dtype=np.float64).reshape(-1)
        assert rewards.shape[0] == obs.shape[0]
        if valid_split_ratio is None:
            valid_split_ratio = self.valid_split_ratio
        assert 1 > valid_split_ratio >= 0
        if (self.normalization is None or compute_normalization) and self.normalize_input:
            self.compute_normalization(obs, act, obs_next, rewards)
        x, y = self._features(obs, act, obs_next), self._targets(rewards)

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
                print("Training RewardModel - epoch %i -- train loss: %.5f  valid loss: %.5f" % (epoch, train_loss, valid_loss))
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
