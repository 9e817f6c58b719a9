"""``MPCController`` - drop-in for ``learning_to_adapt/policies/mpc_controller.py:6-135``.

Same constructor, ``get_action`` / ``get_actions`` / ``reset`` / ``vectorized`` surface and the
same consumption of NumPy's legacy global RNG (``np.random.uniform`` for random shooting,
``:67-69``; ``np.random.normal`` for CEM, ``:85``) as the reference, so that with a fixed seed
the chosen action matches the reference's bit for bit (modulo declared near-ties).

What changed underneath: the horizon loop (``:116-127`` / ``:92-99``) - ``dynamics_model.predict``
+ ``env.reward`` + return accumulation, h sequential host<->device round trips in the
reference - is ONE launch of the fused HIP rollout kernel (``l2a_plan_rs``), and the arg-max
(``:128-129``) comes back as 8 bytes per env.  With ``torch.distributed`` initialised the
candidates are sharded over the ranks (one process per GPU) and the per-rank best keys are
combined by a single max all-reduce (RCCL over xGMI); CEM all-gathers the returns instead,
because its elite rule (``:101``) needs every candidate's rank.

Extra keyword arguments (all optional, defaults reproduce the reference):
``rng`` (``'numpy'`` = parity mode, host MT19937 as in the reference; ``'device'`` = candidates
drawn on the GPU - the library's counter-based Philox stream under ``torch.initial_seed()`` on one GPU, torch's generator
when sharded - statistically equivalent, not bit-identical),
``cem_mode`` (``'reference'`` keeps the reference's three CEM quirks, SURVEY.md section 3.3;
``'fixed'`` = clipped rollouts, true top-k elites, env-consistent row order),
``shard_candidates`` (use torch.distributed when initialised), ``pipeline_chunks`` (parity mode: the
plan step is cut into this many horizon chunks so that the host draws / uploads chunk k + 1 while the
GPU rolls out chunk k - same RNG stream, bit-identical result; 1 = one launch), ``draw_ahead`` (parity
mode: the NEXT controller step's candidates are drawn on a private copy of the generator state while the
GPU runs the current plan and adopted only if the global generator is still in exactly that state -
``policies/draw_ahead.py``; numbers, order and the state left behind are the reference's), ``native_step`` (parity-mode
random shooting on one GPU: the whole step - adopt the block drawn ahead by a C thread, launch, wait, decode, gather - is ONE
C call, ``l2a_controller_step``, ``policies/native_step.py``; a step that finds no valid block falls back to the path above),
``native_cem_step`` (off by default: ``rng="device"`` CEM through the C controller, ``l2a_cem_controller_create_device`` -
sharded over torch.distributed ranks: ``l2a_cem_controller_create_sharded_device``, one rank each - bit-identical to
``get_cem_action_device``, ``policies/native_cem_step.py``; every other case keeps the Python path),
``use_mppi`` (the reward-weighted planner of PDDM, Nagabandi et al. 2019 - not in the reference: a plan mean per env persists on
the device from one controller step to the next, is moved on one step, sampled with time-correlated noise and replaced by the
return-weighted mean of the clipped candidates, ``get_mppi_action``; needs ``rng="device"``; ``mppi_kappa`` the weights'
temperature ``exp(kappa (R - Rmax))``, ``mppi_sigma`` the noise scale per action dimension - ``None``: a quarter of the action
range -, ``mppi_beta`` the noise filter ``n_t = beta u_t + (1 - beta) n_(t-1)``, ``mppi_iters`` refinements per step;
``reset(dones)`` restarts the marked envs' plans from zero), ``native_mppi_step`` (off by default: the MPPI plan step through the C
controller, ``l2a_mppi_controller_create_device`` - the only way to shard an MPPI plan over torch.distributed ranks:
``l2a_mppi_controller_create_sharded_device``, one rank each - bit-identical to ``get_mppi_action``, ``policies/native_mppi_step.py``;
reward programs, reward models and recurrent models keep the Python path),
``use_icem`` (iCEM, Pinneri et al. 2020 - not in the reference: per env a plan mean, a spread and kept elites persist on the device;
a step moves mean and kept elites on one horizon step and re-opens the spread to ``icem_sigma`` - ``None``: a quarter of the action
range -, an iteration places the kept elites first and draws the rest with AR(1) noise ``n_t = rho n_(t-1) + sqrt(1 - rho^2) z_t``
(``icem_rho``) or, with ``icem_noise="powerlaw"``, with the paper's coloured noise of power spectral density ``f^-icem_beta``
(``l2a_icem_noise_matrix`` / ``l2a_icem_sample_noise``, horizons up to 128; ``icem_rho`` is ignored then; ``icem_beta = 0`` is white
noise, the default 2 a lag-1 correlation of 0.88 at ``horizon = 30``), the population shrinks by ``icem_decay`` per iteration down
to twice the elites, ``percent_elites`` and ``alpha`` refit
mean and spread, ``icem_keep`` of the elites are kept, ``icem_add_mean`` adds the mean itself to the last of the ``icem_iters``
iterations, and the best candidate's first action is returned, ``get_icem_action``; needs ``rng="device"``; ``reset(dones)`` restarts
the marked envs' plans), ``native_icem_step`` (off by default: the iCEM plan step through the C controller,
``l2a_icem_controller_create_device`` - the only way to shard an iCEM plan over torch.distributed ranks:
``l2a_icem_controller_create_sharded_device``, one rank each - bit-identical to ``get_icem_action``, ``policies/native_icem_step.py``;
reward programs, reward models and particle plans keep the Python loop),
``ensemble_planning`` (``"mean"``, the default: the members of an ``MLPDynamicsModel(ensemble_size=E)`` share one state, their
deltas averaged at every horizon step; ``"particles"``: PETS-style trajectory sampling - every member rolls every candidate out as a
trajectory of its own and a candidate's score is the mean of its E returns less ``risk_coef`` times their standard deviation,
``l2a_plan_rs_particles``; random shooting, CEM and MPPI all plan on that score, ``particle_diagnostics()`` reads the winner's
member returns back; the C controller steps do not apply: the default ``native_step`` steps aside, an explicit ``native_cem_step``
/ ``native_mppi_step`` raises),
``particle_sampling`` (with ``ensemble_planning="particles"``: ``"tsinf"``, the default - a particle stays on one member for the
whole horizon - or ``"ts1"``: between two horizon steps every candidate's particles are dealt anew over the members by a random
permutation, ``l2a_plan_rs_particles_ts1``; seeded by ``torch.initial_seed()`` under either ``rng``, every rollout takes the next
``horizon * m`` permutation slots; one rank only, and the fused reward formula only unless the next keyword is set),
``ts1_step_rewards`` (off by default: ``particle_sampling="ts1"`` refuses an env with a ``RewardProgram`` and ``use_reward_model``
at construction; on: such a plan takes every step's reward where the particles are dealt, ``l2a_plan_rs_particles_ts1_program`` /
``_reward_model`` - random shooting, CEM, MPPI and iCEM alike; with a ``RewardSpec`` env the keyword changes nothing),
``value_model`` / ``terminal_value_coef`` (a learned terminal value, ``MLPValueModel``: every planner scores
``R' = R + terminal_value_coef * discount ** h * V(s_h)``, the value of each candidate's last predicted state folded into returns and
keys by one launch behind the rollout - ``l2a_plan_rs_value`` / ``_program_value`` / ``_reward_model_value``; no host fallback, not
with ``ensemble_planning="particles"`` or an explicit C controller step, which raise at construction),
``termination`` (a ``TerminationProgram``; default: the env's ``termination_spec``: every candidate's return stops at its first step
whose next observation leaves a guarded range, and a ``value_model`` is folded into the surviving candidates only - one scoring
launch behind the trajectory rollout, ``l2a_plan_rs_term``; random shooting, CEM, MPPI and iCEM alike; no host fallback, not with
``ensemble_planning="particles"``, an explicit C controller step or the recurrent planner, which raise at construction;
``termination_diagnostics()`` copies the winner's ``steps_alive`` and the terminated share back on demand),
``policy_model`` / ``policy_candidates`` / ``policy_fraction`` / ``policy_noise`` (a learned policy prior, ``MLPPolicyModel``: the first
``n_pi = policy_candidates or max(1, round(policy_fraction * n))`` candidates of every env are the policy rolled in closed loop through
the dynamics model, ``a_t = pi(s_t) + policy_noise * eps``, clipped to the action box - ``l2a_policy_propose``, written into the
candidate tensor (and CEM's / MPPI's sample memory) in front of the unchanged rollout, so it composes with every scoring path;
random shooting under ``rng="device"``, CEM in ``cem_mode="fixed"`` and MPPI; ``last_plan["policy_candidates"]`` is ``n_pi``, so
``best_index < n_pi`` says the policy's proposal won; no host fallback, not with ``use_icem``, ``cem_mode="reference"``,
``rng="numpy"``, an explicit C controller step or more than one rank, which raise).

A tile-split launch whose exchange partner was not co-resident (another process on the GPU) flags a status
word instead of hanging; the controller then switches the context to the unsplit geometry (bit-identical
results) and relaunches the plan - it never raises mid-rollout for that.
"""

import os

import numpy as np
import torch

from .. import _lib
from ..envs.reward_spec import RewardProgram, reward_spec_for_env
from ..envs.termination import TerminationProgram, termination_spec_for_env
from ..utils import fast_rng
from ..utils.serializable import Serializable
from .draw_ahead import DrawAhead
from .policy import Policy, innermost_env


class MPCController(Policy, Serializable):
    def __init__(
            self,
            name,
            env,
            dynamics_model,
            reward_model=None,
            discount=1,
            use_cem=False,
            n_candidates=1024,
            horizon=10,
            num_cem_iters=8,
            percent_elites=0.1,
            use_reward_model=False,
            alpha=0.1,
            rng="numpy",
            cem_mode="reference",
            shard_candidates=True,
            pipeline_chunks=5,
            draw_ahead=True,
            native_step=True,
            native_cem_step=False,
            use_mppi=False,
            mppi_kappa=1.0,
            mppi_sigma=None,
            mppi_beta=0.6,
            mppi_iters=1,
            native_mppi_step=False,
            ensemble_planning="mean",
            risk_coef=0.0,
            use_icem=False,
            icem_iters=3,
            icem_keep=0.3,
            icem_decay=1.25,
            icem_rho=0.5,
            icem_sigma=None,
            icem_add_mean=True,
            native_icem_step=False,
            icem_noise="ar1",
            icem_beta=2.0,
            particle_sampling="tsinf",
            ts1_step_rewards=False,
            value_model=None,
            terminal_value_coef=1.0,
            termination=None,
            policy_model=None,
            policy_candidates=None,
            policy_fraction=0.05,
            policy_noise=0.0,
    ):
        self.dynamics_model = dynamics_model
        self.value_model = value_model
        self.policy_model = policy_model
        self.policy_candidates = policy_candidates
        self.policy_fraction = float(policy_fraction)
        self.policy_noise = policy_noise
        self.terminal_value_coef = float(terminal_value_coef)
        self.reward_model = reward_model
        self.discount = discount
        self.n_candidates = n_candidates
        self.horizon = horizon
        self.use_cem = use_cem
        self.num_cem_iters = num_cem_iters
        self.percent_elites = percent_elites
        self.env = env
        self.use_reward_model = use_reward_model
        self.alpha = alpha
        assert rng in ("numpy", "device")
        assert cem_mode in ("reference", "fixed")
        self.rng = rng
        self.cem_mode = cem_mode
        self.shard_candidates = shard_candidates
        self.pipeline_chunks = int(pipeline_chunks)
        self.draw_ahead = bool(draw_ahead)
        self.native_step = bool(native_step)
        self.native_cem_step = bool(native_cem_step)
        self.use_mppi = bool(use_mppi)
        self.mppi_kappa = float(mppi_kappa)
        self.mppi_sigma = mppi_sigma
        self.mppi_beta = float(mppi_beta)
        self.mppi_iters = int(mppi_iters)
        self.native_mppi_step = bool(native_mppi_step)
        if self.use_mppi:
            if use_cem:
                raise ValueError("use_mppi and use_cem are two planners: choose one")
            if rng != "device":
                raise ValueError("use_mppi draws its normals on the device: pass rng='device'")
            if not (self.mppi_kappa > 0.0 and np.isfinite(self.mppi_kappa)):
                raise ValueError("mppi_kappa must be positive and finite")
            if not 0.0 < self.mppi_beta <= 1.0:
                raise ValueError("mppi_beta must lie in (0, 1]")
            if self.mppi_iters < 1:
                raise ValueError("mppi_iters must be at least 1")
        self.use_icem = bool(use_icem)
        self.icem_iters = int(icem_iters)
        self.icem_keep = float(icem_keep)
        self.icem_decay = float(icem_decay)
        self.icem_rho = float(icem_rho)
        self.icem_sigma = icem_sigma
        self.icem_add_mean = bool(icem_add_mean)
        self.native_icem_step = bool(native_icem_step)
        self.icem_noise = icem_noise
        self.icem_beta = float(icem_beta)
        if self.native_icem_step and (use_cem or self.use_mppi):
            raise _lib.L2AError("native_icem_step is the iCEM planner's C controller step (use_icem=True): with use_cem it is "
                                "native_cem_step, with use_mppi native_mppi_step")
        if self.use_icem:
            if use_cem or self.use_mppi:
                raise ValueError("use_icem, use_cem and use_mppi are three planners: choose one")
            if rng != "device":
                raise ValueError("use_icem draws its normals on the device: pass rng='device'")
            if self.icem_iters < 1:
                raise ValueError("icem_iters must be at least 1")
            if not 0.0 <= self.icem_keep <= 1.0:
                raise ValueError("icem_keep must lie in [0, 1]")
            if not (self.icem_decay >= 1.0 and np.isfinite(self.icem_decay)):
                raise ValueError("icem_decay must be finite and at least 1")
            if not 0.0 <= self.icem_rho < 1.0:
                raise ValueError("icem_rho must lie in [0, 1)")
            if self.icem_noise not in ("ar1", "powerlaw"):
                raise ValueError("icem_noise is 'ar1' or 'powerlaw', not %r" % (icem_noise,))
            if not (np.isfinite(self.icem_beta) and 0.0 <= self.icem_beta <= 8.0):
                raise ValueError("icem_beta must be finite and lie in [0, 8]")
            if not 0.0 <= float(alpha) < 1.0:
                raise ValueError("use_icem needs alpha in [0, 1)")
            if not percent_elites > 0:
                raise ValueError("use_icem needs percent_elites > 0")

        if ensemble_planning not in ("mean", "particles"):
            raise ValueError("ensemble_planning is 'mean' or 'particles', not %r" % (ensemble_planning,))
        self.ensemble_planning = ensemble_planning
        self.risk_coef = float(risk_coef)
        if not np.isfinite(self.risk_coef):
            raise ValueError("risk_coef must be finite")
        if particle_sampling not in ("tsinf", "ts1"):
            raise ValueError("particle_sampling is 'tsinf' or 'ts1', not %r" % (particle_sampling,))
        if particle_sampling == "ts1" and ensemble_planning != "particles":
            raise ValueError("particle_sampling='ts1' deals an ensemble's particles anew at every horizon step: it needs "
                             "ensemble_planning='particles'")
        self.particle_sampling = particle_sampling
        self.ts1_step_rewards = bool(ts1_step_rewards)
        if ensemble_planning == "particles":
            self._check_particles()

        self.unwrapped_env = innermost_env(env)

        # make sure that env has reward function (reference :39)
        assert hasattr(self.unwrapped_env, 'reward'), "env must have a reward function"

        Serializable.quick_init(self, locals())
        super(MPCController, self).__init__(env=env)

        self._reward_spec = None if use_reward_model else reward_spec_for_env(env)
        if particle_sampling == "ts1" and not self.ts1_step_rewards and \
                (use_reward_model or isinstance(self._reward_spec, RewardProgram)):
            raise _lib.L2AError("particle_sampling='ts1' scores the fused reward formula only: a reward program or a reward model "
                                "reads a step's two states from one trajectory row, which the shuffle between steps breaks")
        if value_model is not None:
            self._check_value_model()
        self._termination = termination if termination is not None else termination_spec_for_env(env)
        if self._termination is not None:
            self._check_termination()
        if policy_model is not None:
            self._check_policy_model()
        self._pol_calls = 0         # `_policy_fill` calls since the seed below was first seen
        self._pol_seed = None       # torch.initial_seed() the count belongs to: a changed seed restarts it
        self._term = None           # device tensors of the latest plan under a termination program (`termination_diagnostics`)
        self._ts1_calls = 0         # `_rollout` calls under particle_sampling="ts1" since the seed below was first seen
        self._ts1_seed = None       # torch.initial_seed() the count belongs to: a changed seed restarts it
        self._bufs = {}
        if self.use_mppi:
            self._mppi_sigma_vector()       # (a bad mppi_sigma fails here, not on the first step)
        if self.use_icem:
            self._icem_sigma_vector()
        self._ahead = None          # DrawAhead chain (parity mode), created on first use
        self._cstep = None          # NativeStep (l2a_controller): the whole parity-mode step in one C call
        self._cstep_no = None       # request key the C controller was found ineligible for
        self._cemstep = None        # NativeCemStep (CEM l2a_controller, rng="device"): the whole CEM plan step in one C call
        self._cemstep_no = None     # key of a sharded CEM controller that could not be built (the collective's dry run failed)
        self._mppistep = None       # NativeMppiStep (MPPI l2a_controller): the whole MPPI plan step in one C call
        self._mppi_side = None      # which side plans (and holds the persistent mean): None until the first MPPI step, then "c" / "python"
        self._icemstep = None       # NativeIcemStep (iCEM l2a_controller): the whole iCEM plan step in one C call
        self._icem_side = None      # which side plans (and holds mean, spread and kept elites): None until the first iCEM step, then "c" / "python"
        self._cem_first_chunk = 4   # horizon steps of the first chunk of a pipelined CEM rollout (0: equal chunks)
        self.last_plan = None       # diagnostics of the latest fused plan (returns, keys, ...)
        self._particles = None      # device tensors of the latest particle rollout (`particle_diagnostics`)

    @property
    def vectorized(self):
        return True

    def _check_particles(self):
        """``ensemble_planning="particles"``: the members must be there to be rolled out one by one - a mean ensemble of at least
        two weight sets - and the plan goes through ``_rollout``, which the C controller steps bypass."""
        model = self.dynamics_model
        if getattr(model, "mode", None) != "mean" or int(getattr(model, "ensemble_size", 1)) < 2:
            raise _lib.L2AError("ensemble_planning='particles' needs a mean ensemble: MLPDynamicsModel(ensemble_size >= 2)")
        if self.native_cem_step or self.native_mppi_step:
            raise _lib.L2AError("ensemble_planning='particles' plans through the Python loop: the C controller steps "
                                "(native_cem_step, native_mppi_step) roll the mean ensemble out - leave them off")

    def _check_value_model(self):
        """``value_model=...``: the plan is scored on ``R' = R + terminal_value_coef * discount ** h * V(s_h)`` by a launch of its
        own behind the rollout (``l2a_value_terminal``) - there is no host fallback, and the plan goes through ``_rollout``, which
        the C controller steps bypass."""
        vm = self.value_model
        if not np.isfinite(self.terminal_value_coef):
            raise ValueError("terminal_value_coef must be finite")
        if not hasattr(vm, "planner_value_model"):
            raise _lib.L2AError("value_model must be a value model the library evaluates on the GPU (MLPValueModel): there is no "
                                "host fallback")
        why = vm.native_eligible() if hasattr(vm, "native_eligible") else None
        if why is not None:
            raise _lib.L2AError("value_model is not eligible for the terminal-value kernel (there is no host fallback): %s" % why)
        if self.ensemble_planning == "particles":
            raise _lib.L2AError("ensemble_planning='particles' with a value_model is not built: a particle plan scores every "
                                "member's rollout, the terminal value is folded into the mean ensemble's plan only")
        if self.native_cem_step or self.native_mppi_step or self.native_icem_step:
            raise _lib.L2AError("a value_model plans through the Python loop: the C controller steps (native_cem_step, "
                                "native_mppi_step, native_icem_step) score the plain return - leave them off")
        if self._reward_spec is None and self._native_reward_model() is None:
            raise _lib.L2AError("a value_model needs a plan the library scores: an env reward it knows (a RewardSpec or a "
                                "RewardProgram) or, with use_reward_model, a reward model it scores (MLPRewardModel)")
        if not hasattr(self.dynamics_model, "planner_model"):
            raise _lib.L2AError("a value_model needs a dynamics model with a native planner (MLPDynamicsModel)")

    def _check_policy_model(self):
        """``policy_model=...``: the first ``n_pi`` candidates of every env are the policy rolled in closed loop through the
        dynamics model on the GPU (``l2a_policy_propose``), written into the tensors the planner already holds directly in front
        of ``_rollout`` - there is no host fallback, and the C controller steps, which draw and score in one call, do not apply."""
        pm = self.policy_model
        n = int(self.n_candidates)
        if self.policy_candidates is not None:
            n_pi = int(self.policy_candidates)
        else:
            if not (np.isfinite(self.policy_fraction) and 0.0 <= self.policy_fraction <= 1.0):
                raise ValueError("policy_fraction must lie in [0, 1]")
            n_pi = max(1, int(round(self.policy_fraction * n)))
        if n_pi < 1:
            raise ValueError("policy_candidates must be at least 1")
        if n_pi > n:
            raise _lib.L2AError("policy_candidates %d exceeds n_candidates %d" % (n_pi, n))
        self._n_pi = n_pi
        self._policy_sigma = self._sigma_vector(self.policy_noise, "policy_noise")
        if self.rng != "device":
            raise _lib.L2AError("a policy_model proposes its candidates on the device: pass rng='device' (the parity path returns "
                                "the winner's action from the host copy of the candidates, which the proposal never reaches)")
        if self.use_icem:
            raise _lib.L2AError("a policy_model with use_icem is not built: the kept elites and the added mean own candidate slots")
        if self.use_cem and self.cem_mode == "reference":
            raise _lib.L2AError("a policy_model needs cem_mode='fixed': cem_mode='reference' rolls out the unclipped samples in "
                                "candidate-major rows, which the proposal does not write")
        if self.native_cem_step or self.native_mppi_step or self.native_icem_step:
            raise _lib.L2AError("a policy_model plans through the Python loop: the C controller steps (native_cem_step, "
                                "native_mppi_step, native_icem_step) draw and score in one call - leave them off")
        if not hasattr(pm, "planner_policy_model"):
            raise _lib.L2AError("policy_model must be a policy the library evaluates on the GPU (MLPPolicyModel): there is no "
                                "host fallback")
        why = pm.native_eligible() if hasattr(pm, "native_eligible") else None
        if why is not None:
            raise _lib.L2AError("policy_model is not eligible for the policy kernel (there is no host fallback): %s" % why)
        if not self._fusable():
            raise _lib.L2AError("a policy_model needs a plan the library scores: an env reward it knows (a RewardSpec or a "
                                "RewardProgram) or, with use_reward_model, a reward model it scores (MLPRewardModel), and a "
                                "dynamics model with a native planner (MLPDynamicsModel)")

    def _policy_fill(self, obs_dev, seq, mirror, n_local, cand_offset):
        """Overwrite candidates ``cand_offset + j < n_pi`` of every env in ``seq`` ``[h, m * n_local, act_dim]`` (and in ``mirror``,
        the planner's ``a_clip`` ``[n, m, h * act_dim]``) with the policy's closed-loop proposal (``l2a_policy_propose``, 2 h - 1
        launches, stream-ordered).  Every call - an RS step, a CEM / MPPI iteration, a relaunch after a flagged tile split - takes
        the next ``h * m * n_pi * act_dim`` counters of a Philox stream of its own under ``torch.initial_seed()``."""
        if self._dist()[1] > 1:
            raise _lib.L2AError("a policy_model is not sharded at the controller level (the sharded CEM keeps a full a_clip on every "
                                "rank): plan on one rank (shard_candidates=False), or call l2a_policy_propose per shard")
        native = self.dynamics_model.planner_model()
        dev = native.device
        m, h, act_dim = int(obs_dev.shape[0]), self.horizon, self.action_space.shape[0]
        const = self._bufs.get("pol_const")
        if const is None or const[0].device != dev:
            up = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)  # noqa: E731
            const = self._bufs["pol_const"] = (up(self._policy_sigma), up(self.action_space.low), up(self.action_space.high))
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        if seed != self._pol_seed:
            self._pol_seed, self._pol_calls = seed, 0
        offset = self._pol_calls * h * m * self._n_pi * act_dim
        self._pol_calls += 1
        native.policy_propose(self.policy_model.planner_policy_model(), obs_dev, m, n_local, self._n_pi, h, seq, const[0], const[1],
                              const[2], mirror=mirror, n_total=self.n_candidates, cand_offset=cand_offset, seed=seed, offset=offset)

    _takes_termination = True       # (RNNMPCController: False - the recurrent planner scores no termination program)

    def _check_termination(self):
        """``termination=...`` (or the env's ``termination_spec``): every candidate's return stops at its first step whose next
        observation fails a guard (``l2a_plan_rs_term``) - there is no host fallback, and the plan goes through ``_rollout``,
        which the C controller steps bypass."""
        term = self._termination
        if not isinstance(term, TerminationProgram):
            raise _lib.L2AError("termination must be a TerminationProgram (envs/termination.py), not %s" % type(term).__name__)
        try:
            term.check(int(self.env.observation_space.shape[0]))
        except ValueError as e:
            raise _lib.L2AError(str(e))
        if not self._takes_termination:
            raise _lib.L2AError("the recurrent planner scores no termination program: plan this env with an MLPDynamicsModel "
                                "(MPCController)")
        if self.ensemble_planning == "particles":
            raise _lib.L2AError("ensemble_planning='particles' with a termination program is not built (either particle_sampling): "
                                "a particle plan scores every member's rollout on the whole horizon")
        if self.native_cem_step or self.native_mppi_step or self.native_icem_step:
            raise _lib.L2AError("a termination program plans through the Python loop: the C controller steps (native_cem_step, "
                                "native_mppi_step, native_icem_step) score the whole horizon - leave them off")
        if self._reward_spec is None and self._native_reward_model() is None:
            raise _lib.L2AError("a termination program needs a plan the library scores: an env reward it knows (a RewardSpec or a "
                                "RewardProgram) or, with use_reward_model, a reward model it scores (MLPRewardModel)")
        if not hasattr(self.dynamics_model, "planner_model"):
            raise _lib.L2AError("a termination program needs a dynamics model with a native planner (MLPDynamicsModel)")

    # ------------------------------------------------------------------ reference API
    def get_action(self, observation):
        if observation.ndim == 1:
            observation = observation[None]
        if self.use_icem:
            action = self.get_icem_action(observation)
        elif self.use_mppi:
            action = self.get_mppi_action(observation)
        elif self.use_cem:
            action = self.get_cem_action(observation)
        else:
            action = self.get_rs_action(observation)
        return action, dict()

    def get_actions(self, observations):
        if self.use_icem:
            actions = self.get_icem_action(observations)
        elif self.use_mppi:
            actions = self.get_mppi_action(observations)
        elif self.use_cem:
            actions = self.get_cem_action(observations)
        else:
            actions = self.get_rs_action(observations)
        return actions, dict()

    _fast_uniform = None        # class-wide: does the vectorised draw reproduce np.random.uniform bit for bit here?

    def get_random_action(self, n):
        """``np.random.uniform(low, high, (n, act_dim))`` (reference ``:67-69``) - same values, same
        consumption of the global MT19937 stream.  NumPy's legacy ``uniform`` with array bounds walks a
        broadcast iterator per element (measured 2.6x the cost of the raw doubles); ``low + (high - low) *
        random_sample()`` is the same arithmetic (``random_uniform``: ``lower + range * next_double``, two
        roundings) vectorised.  Verified once per process against the real call on a saved RNG state; if
        the platform's NumPy ever differed, the reference call is used."""
        low, high = self.action_space.low, self.action_space.high
        shape = (n,) + low.shape
        cls = MPCController
        if cls._fast_uniform is None:
            state = np.random.get_state()
            want = np.random.uniform(low=low, high=high, size=(257,) + low.shape)
            np.random.set_state(state)
            got = np.random.random_sample((257,) + low.shape)
            got *= (high - low)
            got += low
            np.random.set_state(state)
            cls._fast_uniform = bool(np.array_equal(want, got))
        if not cls._fast_uniform:
            return np.random.uniform(low=low, high=high, size=shape)
        u = fast_rng.random_sample(shape)            # same stream, vectorised generator (utils/fast_rng.py)
        # full-size (contiguous) scale / offset arrays: broadcasting a length-act_dim vector over the last
        # axis makes NumPy run act_dim-element inner loops, slower than the draw itself
        key = ("uniform_affine", shape)
        aff = self._bufs.get(key)
        if aff is None:
            aff = (np.ascontiguousarray(np.broadcast_to(high - low, shape)),
                   np.ascontiguousarray(np.broadcast_to(low, shape)))
            self._bufs[key] = aff
        u *= aff[0]
        u += aff[1]
        return u

    def get_params_internal(self, **tags):
        return []

    def reset(self, dones=None):
        self._mppi_reset(dones)
        self._icem_reset(dones)

    # ------------------------------------------------------------------ sharding helpers
    def _dist(self):
        """(rank, world) when candidates are sharded over torch.distributed ranks."""
        if self.shard_candidates and torch.distributed.is_available() and torch.distributed.is_initialized():
            return torch.distributed.get_rank(), torch.distributed.get_world_size()
        return 0, 1

    @staticmethod
    def _shard_range(n, rank, world):
        return (rank * n) // world, ((rank + 1) * n) // world

    DIGEST_MASK = 0x7FFFFFFFFFFF          # include/l2a.h: L2A_DIGEST_MASK

    def _rank_digest(self):
        """Fingerprint of what this rank's candidates were drawn from.  Sharded planning lets every rank draw the SAME
        candidate tensor and keep its slice (parity mode), or the same CEM normals (device mode).  Ranks seeded
        differently (the common ``seed + rank``) - or one rank whose generator was consumed by something else between
        two plans (an in-process env reset, a logger) - would combine keys and returns that refer to different
        actions, silently.  Parity mode: the global MT19937 state as this step's draw left it (~1 us); device mode:
        ``torch.initial_seed()``.  Travels with EVERY collective of a plan step (two more words), so a disagreement is
        caught on the step it happens, on all ranks at once."""
        if self.rng == "numpy":
            return fast_rng.global_digest(with_gauss=bool(self.use_cem)) & self.DIGEST_MASK
        return int(torch.initial_seed()) & self.DIGEST_MASK

    def _digest_error(self):
        what = "np.random global state" if self.rng == "numpy" else "torch.initial_seed()"
        return _lib.L2AError("candidate sharding needs identical %s on every rank (seed all ranks alike and keep other "
                             "consumers of the generator off the planning process; the shards themselves are disjoint)"
                             % what)

    def _agree(self, flag, world):
        """Host-side facts every rank must share before a collective whose inputs depend on them (CEM: the all-gather
        of the returns): MAX all-reduce of ``[flag, digest, MASK - digest]``.  Returns ``any rank's flag``; raises - on
        every rank - when the digests differ."""
        if world == 1:
            return bool(flag)
        d = self._rank_digest()
        t = torch.tensor([1 if flag else 0, d, self.DIGEST_MASK - d], dtype=torch.int64, device=self._device())
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        v = t.cpu().numpy()
        if int(v[1]) + int(v[2]) != self.DIGEST_MASK:
            raise self._digest_error()
        return bool(int(v[0]))

    @staticmethod
    def _all_gather(mine, world):
        """``all_gather`` of equally shaped tensors.  RCCL gathers device tensors; gloo implements the collective for host
        tensors only, so a GPU tensor goes through the host there."""
        if mine.is_cuda and torch.distributed.get_backend() == "gloo":
            mine = mine.cpu()
        parts = [torch.empty_like(mine) for _ in range(world)]
        torch.distributed.all_gather(parts, mine)
        return parts

    def _force_unsplit(self):
        """Every rank of a sharded plan switches to the unsplit launch geometry (some rank's launch lost its tile-split
        partner)."""
        self.dynamics_model.planner_model().ctx.force_unsplit()

    def _pack_payload(self, best, m):
        """``[keys (m), launch flag, digest, MASK - digest]`` as an int64 tensor on the planning device - packed ON the
        device behind the launch (``l2a_plan_payload`` reads the status word there), so nothing on the host waits
        between the launch and the collective."""
        dev = best.device
        payload = self._buf("payload", (m + 3,), torch.int64, dev)
        self.dynamics_model.planner_model().plan_payload(best, m, self._rank_digest(), payload)
        return payload

    _takes_reward_models = True     # (RNNMPCController: False unless built with `native_reward_model=True`; programs route there too)

    def _fusable(self):
        return ((self._reward_spec is not None or self._native_reward_model() is not None)
                and hasattr(self.dynamics_model, "planner_model"))

    def _native_reward_model(self):
        """``use_reward_model=True`` with a reward model the library scores on the GPU: one that offers
        ``planner_reward_model()`` and passes ``l2a_reward_model_check`` (``MLPRewardModel``).  ``None`` for every other
        object with a ``predict``: those keep the reference's loop (``_get_rs_action_unfused``).  The check is host only and
        made once."""
        if not (self.use_reward_model and self._takes_reward_models):
            return None
        ok = self.__dict__.get("_reward_model_ok")
        if ok is None or ok[0] is not self.reward_model:
            rm = self.reward_model
            good = rm is not None and hasattr(rm, "planner_reward_model") and \
                (not hasattr(rm, "native_eligible") or rm.native_eligible() is None)
            ok = self._reward_model_ok = (rm, bool(good))
        return self.reward_model if ok[1] else None

    def _program(self):
        """The plan is scored by a launch of its own behind the trajectory rollout (``l2a_rollout_traj``) - the env's reward is a
        ``RewardProgram`` (``l2a_plan_rs_program``) or a native reward model stands in for it (``l2a_plan_rs_reward_model``) -
        through ``_rollout``, and every path that would hand the spec to an entry point taking ``l2a_reward`` - the blocking
        launch, the horizon-chunked pipelines, the C controllers - declines.  A particle plan (``ensemble_planning="particles"``)
        is scored behind its rollouts too, whatever its reward, and stays on ``_rollout`` the same way; so does a plan with a
        ``value_model``: its terminal value is folded in by a launch behind the rollout (``l2a_plan_rs_value`` and its siblings);
        and so does a plan under a termination program, scored by ``l2a_plan_rs_term`` behind the trajectory rollout; and so does a
        plan with a ``policy_model``, whose proposal is written into the candidate tensor in front of ``_rollout``."""
        return (self.ensemble_planning == "particles" or isinstance(self._reward_spec, RewardProgram)
                or self._native_reward_model() is not None or self.__dict__.get("value_model") is not None
                or self.__dict__.get("_termination") is not None or self.__dict__.get("policy_model") is not None)

    def _buf(self, key, shape, dtype, device):
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device:
            t = torch.empty(shape, dtype=dtype, device=device)
            self._bufs[key] = t
        return t

    def _pinned(self, key, shape, dev=None):
        """fp32 host staging tensor (page-locked when the planner runs on a GPU)."""
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            dev = dev if dev is not None else self._device()
            t = torch.empty(tuple(shape), dtype=torch.float32, pin_memory=(dev.type == "cuda"))
            self._bufs[key] = t
        return t

    def _host64(self, key, shape):
        a = self._bufs.get(key)
        if a is None or a.shape != tuple(shape):
            a = np.empty(tuple(shape), dtype=np.float64)
            self._bufs[key] = a
        return a

    # ------------------------------------------------------------------ fused rollout of a candidate batch
    def _device(self):
        return self.dynamics_model.planner_model().device

    def _upload(self, actions_local):
        """Host ``[h, m * n_local, act_dim]`` (any float dtype) -> fp32 device tensor: cast straight into a
        pinned staging buffer, one asynchronous H2D copy per plan step (the caller reads the plan's result
        back before it can call again, so the staging buffer is never overwritten in flight)."""
        dev = self._device()
        shape = tuple(actions_local.shape)
        pin = self._bufs.get("a_pin")
        if pin is None or tuple(pin.shape) != shape:
            pin = torch.empty(shape, dtype=torch.float32, pin_memory=True)
            self._bufs["a_pin"] = pin
        np.copyto(pin.numpy(), actions_local, casting="same_kind")
        a_dev = self._buf("a_up", shape, torch.float32, dev)
        a_dev.copy_(pin, non_blocking=True)
        return a_dev

    def _to_device(self, pin, key):
        """Staging tensor -> device tensor ``key`` on the current stream (asynchronous)."""
        dev = self._device()
        if dev.type != "cuda":
            return pin
        a_dev = self._buf(key, tuple(pin.shape), torch.float32, dev)
        a_dev.copy_(pin, non_blocking=True)
        return a_dev

    def _to_device_side(self, pin, key, dev):
        """As ``_to_device`` but on a private copy stream (the draw-ahead worker's upload must not queue behind
        the rollout that is running on the main stream).  Returns ``(tensor, None)``: the copy has completed.  Runs on
        the worker thread: it must not touch the dynamics model (``dev`` is captured by the caller)."""
        if dev.type != "cuda":
            return pin, None
        side = self._bufs.get("side_stream")
        if side is None:
            side = torch.cuda.Stream(device=dev)
            self._bufs["side_stream"] = side
        a_dev = self._buf(key, tuple(pin.shape), torch.float32, dev)
        with torch.cuda.stream(side):
            a_dev.copy_(pin, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        # The worker has a whole plan's duration to spare: it waits for its copy here (GIL released), so that the
        # consumer neither has to make its stream wait for the event (2-45 us on the step's critical path, measured)
        # nor launches behind an unfinished copy.
        ev.synchronize()
        return a_dev, None

    def _sync(self):
        dev = self._device()
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()

    def _check_status(self):
        """After a device->host read-back (= stream sync).  ``False``: a launch since the last check was invalid
        (its tile-split partner was not co-resident); the context has been switched to the unsplit launch
        geometry and the caller must relaunch.  Raises only if launches fail with the split already off."""
        return self.dynamics_model.planner_model().ctx.check_or_degrade()

    def _status_flag(self):
        """After a stream sync: was a launch since the last read flagged invalid?  Reads and clears the status word
        WITHOUT switching the geometry (the ranks of a sharded plan decide that together, ``_agree``)."""
        return self.dynamics_model.planner_model().ctx.launch_status_value() != 0

    def _check_blocks(self, m):
        blocks = self.dynamics_model.planner_blocks(m)
        if blocks != 1 and blocks != m:
            raise _lib.L2AError("the dynamics model holds %d adapted weight sets but %d observations "
                                "were passed" % (blocks, m))

    def _upload_obs(self, observations):
        """``[m, obs_dim]`` host observations -> the fp32 device buffer the rollout reads."""
        native = self.dynamics_model.planner_model()
        shape = (len(observations), native.obs_dim)
        obs0 = self._buf("obs0", shape, torch.float32, native.device)
        # through page-locked staging: an asynchronous copy instead of a pageable one that synchronises the stream
        # (every caller reads the plan's result back before it uploads the next observation)
        pin = self._pinned("obs0_pin", shape, native.device)
        np.copyto(pin.numpy(), np.asarray(observations).reshape(shape), casting="same_kind")
        obs0.copy_(pin, non_blocking=True)
        return obs0

    def _rollout(self, observations, actions_local, n_local, cand_offset, want_returns, obs_dev=None):
        """Launch the fused kernel on this rank's shard.

        ``actions_local``: fp32 CUDA tensor ``[h, m * n_local, act_dim]`` (row = env * n_local + j).
        Returns ``(best_key int64 CUDA [m], returns fp32 CUDA [m, n_local] or None)``.
        """
        native = self.dynamics_model.planner_model()
        m = len(observations)
        self._check_blocks(m)
        dev = native.device
        obs0 = obs_dev if obs_dev is not None else self._upload_obs(observations)
        best = self._buf("best", (m,), torch.int64, dev)
        rets = self._buf("rets", (m, n_local), torch.float32, dev) if want_returns else None
        rm = self._native_reward_model()
        if self.ensemble_planning == "particles":
            # every member's rollout of every candidate, then mean - risk_coef * std: the score table and its keys stand where the
            # returns do; the member returns and the spread stay on the device (`particle_diagnostics`)
            members = self._buf("p_members", (m, native.n_sets, n_local), torch.float32, dev)
            spread = self._buf("p_spread", (m, n_local), torch.float32, dev)
            if self.particle_sampling == "ts1":
                # the permutations are positional in (seed, offset, step, env, candidate): every `_rollout` call - an RS step, a
                # CEM / MPPI / iCEM iteration, a relaunch after a flagged tile split - takes the next h * m slots
                if self._dist()[1] > 1:
                    raise _lib.L2AError("particle_sampling='ts1' is not sharded at the controller level: plan on one rank "
                                        "(shard_candidates=False), or call l2a_plan_rs_particles_ts1 per shard")
                seed = int(torch.initial_seed())
                if seed != self._ts1_seed:
                    self._ts1_seed, self._ts1_calls = seed, 0
                offset = self._ts1_calls * self.horizon * m
                self._ts1_calls += 1
                native.plan_rs_particles_ts1(obs0, actions_local, m, n_local, self.horizon, self.discount,
                                             rm.planner_reward_model() if rm is not None else self._reward_spec,
                                             risk_coef=self.risk_coef, seed=seed, offset=offset, cand_offset=cand_offset,
                                             score_out=rets, spread_out=spread, particle_returns_out=members, best_key=best)
                self._particles = dict(members=members, spread=spread, score=rets, best=best, cand_offset=cand_offset,
                                       ts1_offset=offset)
                return best, rets
            native.plan_rs_particles(obs0, actions_local, m, n_local, self.horizon, self.discount,
                                     rm.planner_reward_model() if rm is not None else self._reward_spec, risk_coef=self.risk_coef,
                                     cand_offset=cand_offset, score_out=rets, spread_out=spread, member_returns_out=members,
                                     best_key=best)
            self._particles = dict(members=members, spread=spread, score=rets, best=best, cand_offset=cand_offset)
            return best, rets
        if self.__dict__.get("_termination") is not None:
            # the return stops at a candidate's terminal step; a value model's V(s_h) is folded into the rows that survive
            steps = self._buf("t_steps", (m, n_local), torch.int32, dev)
            vm = self.__dict__.get("value_model")
            native.plan_rs_term(obs0, actions_local, m, n_local, self.horizon, self.discount,
                                rm.planner_reward_model() if rm is not None else self._reward_spec, self._termination,
                                value_model=vm.planner_value_model() if vm is not None else None,
                                value_coef=self.terminal_value_coef, cand_offset=cand_offset, returns_out=rets,
                                steps_alive_out=steps, best_key=best)
            self._term = dict(steps=steps, best=best, cand_offset=cand_offset, horizon=self.horizon)
            return best, rets
        if self.__dict__.get("value_model") is not None:
            # R' = R + terminal_value_coef * discount ** h * V(s_h): one branch per reward kind, the planners see R' only
            native.plan_rs_value(obs0, actions_local, m, n_local, self.horizon, self.discount,
                                 rm.planner_reward_model() if rm is not None else self._reward_spec,
                                 self.value_model.planner_value_model(), value_coef=self.terminal_value_coef,
                                 cand_offset=cand_offset, returns_out=rets, best_key=best)
            return best, rets
        if rm is not None:
            native.plan_rs_reward_model(obs0, actions_local, m, n_local, self.horizon, self.discount, rm.planner_reward_model(),
                                        cand_offset=cand_offset, returns_out=rets, best_key=best)
            return best, rets
        # (a policy prior holds `_program()` with any reward kind: the fused formula keeps its own entry)
        plan = native.plan_rs_program if isinstance(self._reward_spec, RewardProgram) else native.plan_rs
        plan(obs0, actions_local, m, n_local, self.horizon, self.discount, self._reward_spec,
             cand_offset=cand_offset, returns_out=rets, best_key=best)
        return best, rets

    def termination_diagnostics(self):
        """What the latest plan under a termination program on this rank knew, copied back on demand (nothing of it is on the plan
        step's own read-back): per env ``index`` (global candidate index of the best return in this rank's shard),
        ``steps_alive [m]`` of that winner (``horizon``: it survived) and ``terminated [m]``, the share of this rank's candidates
        that terminated before the horizon's end.  Under CEM, MPPI and iCEM it is the last iteration's rollout; ``None`` before
        the first such plan."""
        st = self._term
        if st is None:
            return None
        keys = st["best"].cpu().numpy()
        m = len(keys)
        index = np.empty(m, dtype=np.int64)
        for i in range(m):
            _, index[i] = _lib.key_decode(keys[i])
        steps = st["steps"].cpu().numpy()
        return dict(index=index, steps_alive=steps[np.arange(m), index - st["cand_offset"]].astype(np.int32),
                    terminated=(steps < st["horizon"]).mean(axis=1))

    def particle_diagnostics(self, tables=False):
        """What the latest particle rollout on this rank knew of its winner, copied back on demand (nothing of it is on the plan
        step's own read-back): per env ``index`` (global candidate index of the best score in this rank's shard), ``score``, the
        winner's ``member_returns [m, E]`` and their ``std [m]``.  ``tables=True`` adds the whole ``member_returns_table
        [m, E, n_local]``, ``spread_table`` and - where the planner asked for the scores - ``score_table [m, n_local]``.  Under CEM
        and MPPI it is the last iteration's rollout; ``None`` before the first particle plan.  Under ``particle_sampling="ts1"`` row
        ``e`` of the member returns is the return of the particle that ENDED in block ``e`` - every step of it predicted by the
        member the particle sat on then - not member ``e``'s own; score and ``std`` are taken over those E returns."""
        st = self._particles
        if st is None:
            return None
        keys = st["best"].cpu().numpy()
        m = len(keys)
        index = np.empty(m, dtype=np.int64)
        score = np.empty(m, dtype=np.float32)
        for i in range(m):
            score[i], index[i] = _lib.key_decode(keys[i])
        dev = st["members"].device
        env = torch.arange(m, device=dev)
        loc = torch.as_tensor(index - st["cand_offset"], device=dev)
        out = dict(index=index, score=score, member_returns=st["members"][env, :, loc].cpu().numpy(),     # the winners' columns only
                   std=st["spread"][env, loc].cpu().numpy())
        if tables:
            out.update(member_returns_table=st["members"].cpu().numpy(), spread_table=st["spread"].cpu().numpy(),
                       score_table=st["score"].cpu().numpy() if st["score"] is not None else None)
        return out

    def _plan_keys(self, observations, a_dev, n_local, lo, world):
        """Roll out ``a_dev`` and return the arg-max keys: as a NumPy uint64 array when the blocking single-GPU
        launch is available (``l2a_plan_rs_sync``: observations staged in host-mapped memory, keys published to a
        host-mapped mailbox by the last tile - no copies, no stream synchronisation; a launch flagged invalid is
        repeated unsplit right here), else as the device tensor ``_rollout`` fills (sharded plans, recurrent
        model, CPU test harness)."""
        m = len(observations)
        stock = getattr(self._rollout, "__func__", None) is MPCController._rollout      # not overridden / replaced
        native = self.dynamics_model.planner_model() if (stock and world == 1 and n_local > 0 and not self._program()) else None
        if native is not None and getattr(native, "sync_max_envs", 0) >= m:
            self._check_blocks(m)
            for _ in range(2):
                keys = native.plan_rs_sync(observations, a_dev, m, n_local, self.horizon, self.discount,
                                           self._reward_spec, cand_offset=lo)
                if keys is not None:
                    return keys.view(np.int64)
            raise _lib.L2AError("rollout launch failed twice")
        if n_local > 0:
            return self._rollout(observations, a_dev, n_local, lo, want_returns=False)[0]
        return torch.zeros((m,), dtype=torch.int64, device=self._device())       # more ranks than candidates

    # ------------------------------------------------------------------ parity-mode draws
    def _draw_rows(self, rows, n, lo, hi, out_f32, rows64=0, out_f64=None):
        """``rows`` rows of the reference's draw (``get_random_action``, ``:67-69``) from the GLOBAL generator:
        candidates ``lo <= row % n < hi`` of every block of n rows as fp32 into ``out_f32`` (this rank's shard, the
        layout ``l2a_plan_rs`` reads), the first ``rows64`` rows as float64 into ``out_f64``.  One threaded pass of
        ``csrc/l2a_rng.c`` when the helper has proven itself on this machine, NumPy otherwise."""
        low, high = self.action_space.low, self.action_space.high
        if fast_rng.available("uniform"):
            st = fast_rng.State.from_global()
            if st is not None:
                st.uniform_rows(rows, low, high, n, lo, hi, out_f32, rows64, out_f64)
                st.to_global()
                return
        a = self.get_random_action(rows)
        act_dim = a.shape[-1]
        if out_f64 is not None and rows64:
            out_f64.reshape(-1, act_dim)[:rows64] = a[:rows64]
        if out_f32 is not None and hi > lo:
            np.copyto(out_f32.reshape(-1, hi - lo, act_dim), a.reshape(-1, n, act_dim)[:, lo:hi, :], casting="same_kind")

    def _use_draw_ahead(self, kind="uniform"):
        return self.draw_ahead and self.rng == "numpy" and fast_rng.available(kind)

    def _ahead_chain(self):
        if self._ahead is None:
            self._ahead = DrawAhead(depth=1)
        return self._ahead

    def _rs_producer(self, n, m, h, lo, hi):
        """Producer of one controller step's candidates for the draw-ahead chain (runs on its worker thread)."""
        low = np.array(self.action_space.low, dtype=np.float64)
        high = np.array(self.action_space.high, dtype=np.float64)
        act_dim = low.shape[0]
        n_local = hi - lo
        dev = self._device()

        def produce(state, slot):
            c64 = self._host64(("ahead_c64", slot), (m * n, act_dim))
            if n_local > 0:
                pin = self._pinned(("ahead_pin", slot), (h, m * n_local, act_dim), dev)
                state.uniform_rows(h * n * m, low, high, n, lo, hi, pin.numpy(), n * m, c64)
                a_dev, ev = self._to_device_side(pin, ("ahead_dev", slot), dev)
            else:
                state.uniform_rows(h * n * m, low, high, n, lo, hi, None, n * m, c64)
                a_dev, ev = None, None
            return dict(a_dev=a_dev, event=ev, cand_a=c64.reshape(m, n, act_dim))
        return produce

    # ------------------------------------------------------------------ the whole step in one C call
    def _native_step_stock(self):
        """The launch path is the product's own (a test harness that replaces it must not be bypassed)."""
        return (getattr(self._rollout, "__func__", None) is MPCController._rollout
                and getattr(self._plan_keys, "__func__", None) is MPCController._plan_keys)

    def _native_step_state(self, native, m):
        """Recurrent planners: ``((c0, h0, c_next, h_next) device pointers, what to keep)``; None here."""
        return None, None

    def _native_step_done(self, keep):
        pass

    @staticmethod
    def _reduce_payload(payload):
        """The sharded C step's one collective through torch.distributed: int64 MAX all-reduce of ``[keys, flag, digest pair]``
        in place (``backend="nccl"`` is RCCL over xGMI; gloo reduces host tensors only, so the words go through the host)."""
        if torch.distributed.get_backend() == "gloo":
            host = payload.cpu()
            torch.distributed.all_reduce(host, op=torch.distributed.ReduceOp.MAX)
            payload.copy_(host)
        else:
            torch.distributed.all_reduce(payload, op=torch.distributed.ReduceOp.MAX)

    @staticmethod
    def _native_comm(native, rank, world):
        """``L2A_NATIVE_COMM=1``: the library's OWN RCCL communicator (``l2a_comm_init``) carries the step's collective
        (``l2a_allreduce_best`` on m + 3 words) instead of torch.distributed; its id travels through torch.distributed once."""
        import ctypes
        ctx = native.ctx
        if getattr(ctx, "native_comm", None) == (rank, world):
            return True
        ids = [None]
        if rank == 0:
            buf = ctypes.create_string_buffer(128)
            ctx.check(native.lib.l2a_comm_unique_id(buf), "l2a_comm_unique_id")
            ids[0] = buf.raw
        torch.distributed.broadcast_object_list(ids, src=0)
        ctx.check(native.lib.l2a_comm_init(ctx.handle, int(rank), int(world), ids[0]), "l2a_comm_init")
        ctx.native_comm = (rank, world)
        return True

    def _native_shard(self, native, rank, world, words):
        """The ``shard`` tuple of a sharded C step (``NativeStep`` / ``NativeCemStep``) whose collective reduces ``words`` int64 words:
        over the library's own communicator (``L2A_NATIVE_COMM=1``), else through ``_reduce_payload`` - after a dry run of that
        collective (every rank builds its controller in the same step, so the call is symmetric).  None: the backend cannot
        MAX-reduce int64 words on this device, and the plan keeps the Python path."""
        if os.environ.get("L2A_NATIVE_COMM", "0") == "1" and torch.distributed.get_backend() != "gloo":
            self._native_comm(native, rank, world)
            return (rank, world, None)
        try:
            self._reduce_payload(torch.zeros((words,), dtype=torch.int64, device=native.device))
        except Exception:
            return None
        return (rank, world, self._reduce_payload)

    def _native_step_build(self, native, m, key, rank=0, world=1):
        from .native_step import NativeStep
        if self._cstep is not None:
            self._cstep.close()
            self._cstep = None
        if os.environ.get("L2A_NATIVE_STEP", "1") == "0" or not hasattr(native.lib, "l2a_controller_step"):
            return None
        if getattr(native, "sync_max_envs", 0) < m or m * native.obs_dim > 4096 or native.act_dim > 16:
            return None
        device = self.rng == "device"
        if not device and (not (fast_rng.available("uniform") and fast_rng.available("direct")) or fast_rng._global_addr() is None):
            return None
        shard = None
        if world > 1:
            # the sharded step in one C call: launch, payload, the ONE collective, read-back - the ~80 us of Python glue per step
            # of `_rs_parity_plan` / `_combine_keys` gone.  The collective: torch.distributed behind a callback (default), or the
            # library's own RCCL communicator (L2A_NATIVE_COMM=1).
            # (rng="device": every rank fills its slice of the SAME Philox stream - the plan does not depend on the world size -
            #  and recomputes the winner's action from the stream: no second collective)
            # (recurrent models: `l2a_lstm_controller_create_sharded[_device]` - the hidden state moves on with the GLOBAL winner's
            #  first action on the device, behind the collective)
            if not hasattr(native.lib, "l2a_lstm_controller_create_sharded" if hasattr(native, "units")
                           else "l2a_controller_create_sharded_device"):
                return None
            shard = self._native_shard(native, rank, world, m + 3)
            if shard is None:
                return None
        st = NativeStep(native, hasattr(native, "units"), m, self.n_candidates, self.horizon, self.action_space.low,
                        self.action_space.high, self.discount, self._reward_spec,
                        device_seed=(int(torch.initial_seed()) if device else None), shard=shard)
        st.key = key
        self._cstep = st
        return st

    def _native_rs_step(self, observations, m):
        """Parity-mode random shooting on one GPU through ``l2a_controller_step`` (``policies/native_step.py``).  Returns the
        actions, or None when the C controller does not apply (sharded plan, test harness, no helper library, a forked child):
        the caller then takes the ordinary path.  A step that finds no valid block of candidates (first call, a foreign draw
        from ``np.random`` since the last step) draws them itself inside the C call - the reference's draw from the global
        generator - and re-arms the chain behind it."""
        self._cstep_missed = False
        if self.use_cem or self._program() or not self._native_step_stock():
            if self._cstep is not None:     # built earlier, bypassed now (a harness replaced the launch path): no idle C chain
                self._cstep.close()
                self._cstep = None
            return None
        rank, world = self._dist()
        native = self.dynamics_model.planner_model()
        # (device mode: the library's counter-based stream (seed, steps so far) restarts whenever torch's seed VALUE changes, like
        #  the device CEM's.  Calling torch.manual_seed(s) again with the same s does NOT rewind it - build a new controller, or
        #  seed with another value in between, to replay a run.  Since round 6 a sharded MLP plan draws its slices from the SAME
        #  Philox stream (`l2a_controller_create_sharded_device`, recurrent: `l2a_lstm_controller_create_sharded_device`):
        #  device-mode plans do not depend on the world size)
        # (parity mode: the address of the global generator's state - the C controller caches it; a generator object that was
        #  replaced, np.random.set_bit_generator, must not leave it reading and writing the old, possibly freed one: ADVICE r5)
        key = (os.getpid(), id(native), native.handle.value, world, m, self.n_candidates, self.horizon, float(self.discount),
               int(torch.initial_seed()) if self.rng == "device" else fast_rng._global_addr())
        st = self._cstep
        if st is None or st.key != key:
            if self._cstep_no == key:
                return None
            st = self._native_step_build(native, m, key, rank, world)
            if st is None:
                self._cstep_no = key
                return None
            self._cstep_no = None
        self._check_blocks(m)
        state, keep = self._native_step_state(native, m)
        if not st.step(observations, torch.cuda.current_stream(native.device).cuda_stream, state):
            self._cstep_missed = True       # (a forked child): this call's fallback plan re-arms the C chain instead of a Python one
            return None
        self._native_step_done(keep)
        lo, hi = self._shard_range(self.n_candidates, rank, world)
        self.last_plan = dict(best_index=st.idx.copy(), best_return=st.ret.copy(), n_local=hi - lo, shard=(lo, hi))
        return st.act.copy()

    def draw_ahead_stats(self):
        """``dict(hits=, misses=)`` of the candidate blocks drawn ahead of time (C controller and Python chain together)."""
        hits = misses = 0
        if self._cstep is not None:
            s = self._cstep.stats()
            hits, misses = hits + s["hits"], misses + s["misses"]
        if self._ahead is not None:
            hits, misses = hits + self._ahead.hits, misses + self._ahead.misses
        return dict(hits=hits, misses=misses)

    # ------------------------------------------------------------------ random shooting (reference :108-129)
    def get_rs_action(self, observations):
        n = self.n_candidates
        m = len(observations)
        h = self.horizon

        if not self._fusable():
            return self._get_rs_action_unfused(observations)

        if self.native_step and (self.draw_ahead or self.rng == "device"):
            out = self._native_rs_step(observations, m)
            if out is not None:
                return out

        rank, world = self._dist()
        lo, hi = self._shard_range(n, rank, world)
        n_local = hi - lo
        act_dim = self.action_space.shape[0]
        dev = self._device()
        a_dev = None

        if self.rng == "numpy":
            best, cand_a, relaunch = self._rs_parity_plan(observations, n, m, h, lo, hi, world)
        else:
            cand_a = None
            a_dev = self._buf("a_dev", (h, m * n_local, act_dim), torch.float32, dev)
            gen = self._bufs.get("rs_gen")
            if gen is None or gen.device != dev:
                # every rank must draw DIFFERENT candidates for its shard
                gen = torch.Generator(device=dev)
                gen.manual_seed((int(torch.initial_seed()) + 7919 * rank) & 0x7FFFFFFF)
                self._bufs["rs_gen"] = gen
            lo_np, hi_np = np.asarray(self.action_space.low), np.asarray(self.action_space.high)
            if np.all(lo_np == lo_np[0]) and np.all(hi_np == hi_np[0]):
                a_dev.uniform_(float(lo_np[0]), float(hi_np[0]), generator=gen)     # one launch (the usual +-bound box)
            else:
                low = torch.as_tensor(lo_np, dtype=torch.float32, device=dev)
                high = torch.as_tensor(hi_np, dtype=torch.float32, device=dev)
                a_dev.uniform_(0.0, 1.0, generator=gen)
                a_dev.mul_(high - low).add_(low)

            def relaunch():
                if self.__dict__.get("policy_model") is not None and n_local > 0:
                    self._policy_fill(self._upload_obs(observations), a_dev, None, n_local, lo)
                return self._plan_keys(observations, a_dev, n_local, lo, world)
            best = relaunch()

        keys = self._combine_keys(best, relaunch, world)
        idx = np.empty(m, dtype=np.int64)
        best_ret = np.empty(m, dtype=np.float32)
        for i in range(m):
            best_ret[i], idx[i] = _lib.key_decode(keys[i])
        self.last_plan = dict(best_index=idx, best_return=best_ret, n_local=n_local, shard=(lo, hi))
        if self.__dict__.get("policy_model") is not None:
            self.last_plan["policy_candidates"] = self._n_pi

        if cand_a is not None:
            return cand_a[range(m), idx]
        # device RNG: the winning first action lives on the rank that owns the candidate
        if world == 1:
            rows = torch.from_numpy(np.arange(m, dtype=np.int64) * n_local + (idx - lo)).to(a_dev.device)
            return a_dev[0].index_select(0, rows).cpu().numpy().astype(np.float64)
        first = a_dev[0].reshape(m, n_local, act_dim)
        gidx = torch.from_numpy(idx).to(a_dev.device)
        own = ((gidx >= lo) & (gidx < hi)).to(torch.float32).unsqueeze(1)
        loc = (gidx - lo).clamp(0, max(n_local - 1, 0))
        out = first[torch.arange(m, device=a_dev.device), loc] * own if n_local > 0 else \
            torch.zeros((m, act_dim), dtype=torch.float32, device=a_dev.device)
        torch.distributed.all_reduce(out, op=torch.distributed.ReduceOp.SUM)
        return out.cpu().numpy().astype(np.float64)

    def _combine_keys(self, best, relaunch, world):
        """Read the arg-max keys back.  Sharded plan: ONE max all-reduce of ``[keys, launch flag, digest pair]`` enqueued
        right behind the launch (no host synchronisation, no status read before the collective), then ONE device-to-host
        copy of ``m + 3`` words.  A set flag means some rank's launch lost its tile-split partner: ALL ranks switch to
        the unsplit geometry (bit-identical results) and repeat their launch and the collective together, so no rank is
        ever out of step and a stale key never decides anything."""
        if isinstance(best, np.ndarray):        # blocking launch: keys already on the host, status already handled
            return best
        if world > 1:
            m = best.numel()
            for attempt in (0, 1):
                payload = self._pack_payload(best, m)
                torch.distributed.all_reduce(payload, op=torch.distributed.ReduceOp.MAX)
                host = payload.cpu().numpy()
                if int(host[m + 1]) + int(host[m + 2]) != self.DIGEST_MASK:
                    raise self._digest_error()
                if int(host[m]) == 0:
                    return host[:m].copy()
                if attempt == 1:
                    raise _lib.L2AError("rollout launch failed twice")
                self._force_unsplit()           # every rank: the reduced flag is the same everywhere
                best = relaunch()
        keys = best.cpu().numpy()
        if self._check_status() is False:
            keys = relaunch().cpu().numpy()
            if self._check_status() is False:
                raise _lib.L2AError("rollout launch failed twice")
        return keys

    def _rs_parity_plan(self, observations, n, m, h, lo, hi, world):
        """Parity mode: candidates from NumPy's global generator exactly as the reference draws them (``:114``:
        ``[h, n*m, act_dim]``, row = i*n + j).  Returns ``(best_key, cand_a float64 [m, n, act], relaunch)``.

        Three ways to the same bits, fastest first: (1) the block the draw-ahead chain prepared while the
        previous plan ran (already in HBM); (2) the draw pipelined over horizon chunks under the rollout;
        (3) one draw, one upload, one launch."""
        n_local = hi - lo
        act_dim = self.action_space.shape[0]
        dev = self._device()
        # the C controller's chain serves the fallback only when the native step was tried in THIS call and could not serve it;
        # a controller that is bypassed for good keeps the Python chain (a silent loss of the draw-ahead otherwise)
        cstep = self._cstep if (self._cstep is not None and self._cstep_no is None and getattr(self, "_cstep_missed", False)) else None
        ahead = self._use_draw_ahead("uniform") and cstep is None      # one chain at a time: the C controller's, if it applies
        sig = ("rs", n, m, h, lo, hi)
        chain = self._ahead_chain() if ahead else None
        blk = chain.take(sig) if ahead else None

        def kick():     # the next controller step's candidates are drawn while this plan runs on the GPU
            if cstep is not None:
                cstep.rearm()
            elif ahead and not chain.active_for(sig):
                chain.start(sig, self._rs_producer(n, m, h, lo, hi), depth=1, words_only=True)

        if blk is not None:
            cand_a, a_dev = blk["cand_a"], blk["a_dev"]
            if blk["event"] is not None:
                torch.cuda.current_stream(dev).wait_event(blk["event"])

            def relaunch():
                return self._plan_keys(observations, a_dev, n_local, lo, world)
            kick()
            best = relaunch()
        elif n_local > 0 and self._can_pipeline(h, n_local):
            best, cand_a = self._plan_pipelined(observations, n, m, h, lo, hi, world)

            def relaunch():
                return self._plan_pipelined(observations, n, m, h, lo, hi, world, redraw=False)[0]
            kick()
        else:
            c64 = self._host64("rs_c64", (m * n, act_dim))
            if n_local > 0:
                pin = self._pinned("rs_pin", (h, m * n_local, act_dim))
                self._draw_rows(h * n * m, n, lo, hi, pin.numpy(), n * m, c64)
                a_dev = self._to_device(pin, "rs_dev")
            else:
                self._draw_rows(h * n * m, n, lo, hi, None, n * m, c64)
                a_dev = None
            cand_a = c64.reshape(m, n, act_dim)

            def relaunch():
                return self._plan_keys(observations, a_dev, n_local, lo, world)
            kick()
            best = relaunch()
        return best, cand_a, relaunch

    # ------------------------------------------------------------------ parity mode, pipelined over the horizon
    def _can_pipeline(self, h, n_local):
        return (self.pipeline_chunks > 1 and h >= 6 and n_local > 0 and not self._program()
                and hasattr(self.dynamics_model.planner_model(), "plan_rs_chunk"))

    def _plan_pipelined(self, observations, n, m, h, lo, hi, world, redraw=True):
        """The reference draws its ``h*n*m`` candidate rows horizon-major (``:114``), so the first rows of the
        stream are the first horizon steps: draw chunk k + 1 on the host while the GPU rolls out chunk k
        (``l2a_plan_rs_chunk`` carries per-candidate state and returns between launches).  Same RNG
        consumption, bit-identical returns and arg-max as the single launch.  ``redraw=False`` relaunches the
        chunks already in HBM (after a launch was flagged invalid)."""
        native = self.dynamics_model.planner_model()
        dev = native.device
        self._check_blocks(m)
        act_dim = self.action_space.shape[0]
        n_local = hi - lo
        K = max(2, min(self.pipeline_chunks, h // 2))      # at least two horizon steps per launch
        bounds = [(h * c) // K for c in range(K + 1)]
        obs0 = self._upload_obs(observations)
        best = self._buf("best", (m,), torch.int64, dev)
        c64 = self._host64("pipe_c64", (m * n, act_dim))
        for c in range(K):
            t0, hc = bounds[c], bounds[c + 1] - bounds[c]
            shape = (hc, m * n_local, act_dim)
            if redraw:
                pin = self._pinned(("pipe_pin", c), shape)
                self._draw_rows(hc * n * m, n, lo, hi, pin.numpy(), n * m if c == 0 else 0, c64 if c == 0 else None)
                a_dev = self._to_device(pin, ("pipe_dev", c))
            else:
                a_dev = self._bufs[("pipe_dev", c)]
            self._launch_chunk(native, c, c == K - 1, obs0, a_dev, m, n_local, hc, t0, lo, best)
        return best, c64.reshape(m, n, act_dim)

    def _launch_chunk(self, native, c, last, obs0, a_dev, m, n_local, hc, t0, lo, best):
        """Chunk ``c`` of a pipelined plan: state and returns ping-pong between two buffer pairs."""
        dev = native.device
        rets = [self._buf("pipe_ret%d" % i, (m, n_local), torch.float32, dev) for i in (0, 1)]
        state = [self._buf("pipe_state%d" % i, (m * n_local, native.obs_dim), torch.float32, dev) for i in (0, 1)]
        native.plan_rs_chunk(obs0 if c == 0 else state[(c + 1) % 2], c > 0, a_dev, m, n_local, hc, t0,
                             self.discount, self._reward_spec, cand_offset=lo,
                             returns_in=rets[(c + 1) % 2] if c > 0 else None, returns_out=rets[c % 2],
                             state_out=None if last else state[c % 2], best_key=best if last else None)

    def _get_rs_action_unfused(self, observations):
        """No closed-form reward available (custom env reward or ``use_reward_model``): keep the
        reference's loop shape; the MLP still runs on the GPU through ``dynamics_model.predict``."""
        n = self.n_candidates
        m = len(observations)
        h = self.horizon
        returns = np.zeros((n * m,))
        a = self.get_random_action(h * n * m).reshape((h, n * m, -1))
        cand_a = a[0].reshape((m, n, -1))
        observation = np.repeat(observations, n, axis=0)
        for t in range(h):
            next_observation = self.dynamics_model.predict(observation, a[t])
            if self.use_reward_model:
                assert self.reward_model is not None
                rewards = self.reward_model.predict(observation, a[t], next_observation)
            else:
                rewards = self.unwrapped_env.reward(observation, a[t], next_observation)
            returns += self.discount ** t * rewards
            observation = next_observation
        returns = returns.reshape(m, n)
        return cand_a[range(m), np.argmax(returns, axis=1)]

    def _cem_draw(self, n, m, D):
        """The iteration's standard normals ``np.random.normal(size=(n, m, D))`` (``:85``) as a ``[n * m, D]``
        float64 array (flat row g = j * m + i): from the draw-ahead chain when it is valid (the z of upcoming
        iterations - and of the next controller step - do not depend on mean / std, so they are drawn while
        the GPU rolls out), else synchronously from the global generator (threaded helper or NumPy)."""
        sig = ("cem", n, m, D)
        if self._use_draw_ahead("normal"):
            chain = self._ahead_chain()
            z = chain.take(sig)
            if z is None:
                z = self._host64("cem_z_sync", (n * m, D))
                st = fast_rng.State.from_global()
                if st is not None:
                    st.standard_normal(n * m * D, out=z.reshape(-1))
                    st.to_global()
                else:
                    z[...] = np.random.normal(size=(n * m, D))

                def produce(state, slot):
                    buf = self._host64(("cem_z", slot), (n * m, D))
                    state.standard_normal(n * m * D, out=buf.reshape(-1))
                    return buf
                chain.start(sig, produce, depth=max(1, int(self.num_cem_iters)))
            return z
        return fast_rng.standard_normal((n * m, D))

    def _cem_iteration(self, observations, mean, std, num_elites, clip_low, clip_high, lo, hi, world):
        """One CEM iteration (reference ``:85-104``): sample, roll out on the GPU, refit mean/std.
        Consumes ``n * m * h * act_dim`` normals of the global NumPy stream."""
        n = self.n_candidates
        m = len(observations)
        h = self.horizon
        act_dim = self.action_space.shape[0]
        D = h * act_dim
        n_local = hi - lo
        reference = (self.cem_mode == "reference")
        z = self._cem_draw(n, m, D)                                         # [n*m, D], row g = j*m + i
        mean2 = np.ascontiguousarray(np.broadcast_to(mean, (m, D)), dtype=np.float64)
        std2 = np.ascontiguousarray(np.broadcast_to(std, (m, D)), dtype=np.float64)
        a = self._host64("cem_a", (n * m, D))                               # :86 (unclipped)
        a_st = self._host64("cem_clip", (n * m, D))                         # :87
        low, high = self.action_space.low, self.action_space.high
        fused = fast_rng.available("double")        # helper library present and trusted
        if fused and n_local > 0 and self._can_pipeline_cem(m, world, n):
            returns = self._cem_rollout_pipelined(observations, z, a, a_st, mean2, std2, reference)
        else:
            if fused and n_local > 0 and D <= 4096:
                pin = self._pinned("cem_pin_all", (h, m * n_local, act_dim))
                fast_rng.cem_samples(z, 0, h, act_dim, mean2, std2, low, high, a, a_st, pin.numpy(), n, lo, hi,
                                     env_major=not reference, use_clipped=not reference)
                a_dev = self._to_device(pin, "cem_dev_all")
            else:
                a3 = mean2 + z.reshape(n, m, D) * std2
                a[...] = a3.reshape(n * m, D)
                a_st[...] = np.clip(a3, clip_low, clip_high).reshape(n * m, D)
                if reference:
                    # reference quirks: rollouts use the UNCLIPPED samples, and the flat row order is
                    # candidate-major (row = j*m + i) while observations are env-major (row // n).
                    seq = np.transpose(a.reshape((n * m, h, act_dim)), (1, 0, 2))          # [h, n*m, act]
                else:
                    seq = np.transpose(a_st.reshape(n, m, D).transpose(1, 0, 2).reshape((m * n, h, act_dim)), (1, 0, 2))
                seq_loc = seq.reshape(h, m, n, act_dim)[:, :, lo:hi, :].astype(np.float32)
                a_dev = self._upload(seq_loc.reshape(h, m * n_local, act_dim))
            if n_local > 0:
                _, rets = self._rollout(observations, a_dev, n_local, lo, want_returns=True)
            else:               # more ranks than candidates: an empty shard still joins the collective
                rets = torch.zeros((m, 0), dtype=torch.float32, device=self._device())
            if world > 1:
                # every rank must gather VALID returns drawn from the SAME normals: the ranks agree on (any launch
                # flagged?, generator digests equal?) first - one more 3-word collective per iteration beside a 2.8 ms
                # rollout - and repeat the rollout unsplit TOGETHER when any of them lost a tile-split partner
                bad = False
                if n_local > 0:
                    self._sync()
                    bad = self._status_flag()
                if self._agree(bad, world):
                    self._force_unsplit()
                    bad = False
                    if n_local > 0:
                        _, rets = self._rollout(observations, a_dev, n_local, lo, want_returns=True)
                        self._sync()
                        bad = self._status_flag()
                    if self._agree(bad, world):
                        raise _lib.L2AError("rollout launch failed twice")
                # all-gather needs equal shapes: shards are padded to the widest one (they differ by at most one
                # candidate) and cut back to their own width afterwards
                widths = [self._shard_range(n, r, world)[1] - self._shard_range(n, r, world)[0] for r in range(world)]
                wmax = max(widths)
                mine = rets if n_local == wmax else torch.cat(
                    [rets, torch.zeros((m, wmax - n_local), dtype=rets.dtype, device=rets.device)], dim=1)
                parts = self._all_gather(mine.contiguous(), world)
                rets = torch.cat([part[:, :w] for part, w in zip(parts, widths)], dim=1)
            returns = rets.cpu().numpy().astype(np.float64).reshape(m, n)
            if world == 1 and self._check_status() is False:
                _, rets = self._rollout(observations, a_dev, n_local, lo, want_returns=True)
                returns = rets.cpu().numpy().astype(np.float64).reshape(m, n)
                if self._check_status() is False:
                    raise _lib.L2AError("rollout launch failed twice")
        if reference:
            cand_a = a[:, :act_dim].reshape(m, n, act_dim)                  # = seq[0].reshape(m, n, -1)
        else:
            cand_a = a_st.reshape(n, m, D)[:, :, :act_dim].transpose(1, 0, 2)
        mean, std = self._cem_refit(mean, a_st.reshape(n, m, D), returns, num_elites, reference)
        return mean, std, returns, np.array(cand_a)

    def _cem_refit(self, mean, a_stacked, returns, num_elites, reference):
        """Elite statistics of one iteration (reference ``:101-104``)."""
        m = returns.shape[0]
        if reference:
            elites_idx = ((-returns).argsort(axis=-1) < num_elites).T                # :101
            # np.mean / np.std of `a_stacked[elites_idx]` (:102-104) without the gather and the temporaries - the same row-after-row
            # float64 sums, verified against NumPy on this machine (csrc/l2a_rng.c: l2a_cem_elite_stats); NumPy itself otherwise
            n_, m_, D_ = a_stacked.shape
            st = fast_rng.elite_stats(a_stacked.reshape(n_ * m_, D_), elites_idx.reshape(-1)) if a_stacked.flags.c_contiguous else None
            if st is not None:
                mu, std = st
            else:
                elites = a_stacked[elites_idx]
                mu, std = np.mean(elites, axis=0), np.std(elites, axis=0)
            mean = mean * self.alpha + (1 - self.alpha) * mu
        else:
            order = np.argsort(-returns, axis=1)[:, :num_elites]                      # [m, k]
            elites = np.stack([a_stacked[order[i], i] for i in range(m)], axis=0)     # [m, k, h*act]
            mean = mean * self.alpha + (1 - self.alpha) * np.mean(elites, axis=1)
            std = np.std(elites, axis=1)
        return mean, std

    def _cem_chunks(self, h):
        """Horizon chunks of a pipelined CEM iteration: two or three (measured on config 5: 1 chunk 16.8 ms per plan
        step, 2 or 3 chunks 16.35, 5 chunks 16.5; cutting the candidates instead: 18.1)."""
        return max(1, min(self.pipeline_chunks, 3, h // 4))

    def _can_pipeline_cem(self, m, world, n):
        """Single env, single rank: the host prepares horizon chunk k + 1 (``a = mean + z * std``, clip, cast,
        transpose of its steps) while the GPU rolls out chunk k."""
        return (m == 1 and world == 1 and self._cem_chunks(self.horizon) > 1 and not self._program()
                and hasattr(self.dynamics_model.planner_model(), "plan_rs_chunk"))

    def _cem_rollout_pipelined(self, observations, z, a, a_st, mean2, std2, reference, relaunch=False):
        """One CEM iteration's rollout for m == 1, pipelined ALONG THE HORIZON: ``a = mean + z * std``, the clip, the
        fp32 cast and the ``[h, rows, act]`` transposition are elementwise in the horizon step, so the steps of chunk
        k + 1 are prepared on the host (``l2a_cem_samples_steps``, threaded) and uploaded while the GPU rolls out chunk k
        of ALL candidates (``l2a_plan_rs_chunk`` hands state and returns from launch to launch, bit-identical to one
        launch).  Every launch keeps the full candidate count - the chip stays as full as with a single launch
        (cutting the candidates instead made two half-empty launches of one full one: 2 x 1.52 ms against 2.77 ms for
        config 5's 4000).  Fills ``a`` / ``a_st`` ``[n, D]``; returns ``returns [1, n]`` float64."""
        native = self.dynamics_model.planner_model()
        dev = native.device
        n, h = self.n_candidates, self.horizon
        act_dim = self.action_space.shape[0]
        self._check_blocks(1)
        K = self._cem_chunks(h)
        # a short first chunk - its samples are the only ones the GPU has to wait for - but long enough for the next
        # chunk's samples to be ready when it ends (host: ~15-30 us per step of 4000 candidates, GPU: ~90 us)
        h0 = max(2, min(self._cem_first_chunk, h // K)) if self._cem_first_chunk else h // K
        bounds = [0] + [h0 + ((h - h0) * c) // (K - 1) for c in range(K)]
        obs0 = self._upload_obs(observations)
        low, high = self.action_space.low, self.action_space.high
        pin = self._pinned("cem_pin_h", (h, n, act_dim))
        a_dev = self._buf("cem_dev_h", (h, n, act_dim), torch.float32, dev)
        rets = [self._buf("cem_ret%d" % i, (1, n), torch.float32, dev) for i in (0, 1)]
        state = [self._buf("cem_state%d" % i, (n, native.obs_dim), torch.float32, dev) for i in (0, 1)]
        for c in range(K):
            t0, t1 = bounds[c], bounds[c + 1]
            if not relaunch:
                fast_rng.cem_samples(z, 0, h, act_dim, mean2, std2, low, high, a, a_st, pin.numpy(), n, 0, n,
                                     env_major=False, use_clipped=not reference, steps=(t0, t1))
                side = self._bufs.get("side_stream")
                if side is None:
                    side = self._bufs["side_stream"] = torch.cuda.Stream(device=dev)
                with torch.cuda.stream(side):           # the upload of chunk k + 1 overlaps the rollout of chunk k
                    a_dev[t0:t1].copy_(pin[t0:t1], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(side)
                torch.cuda.current_stream(dev).wait_event(ev)
            last = (c == K - 1)
            src, dst = (c + 1) % 2, c % 2
            native.plan_rs_chunk(obs0 if c == 0 else state[src], c > 0, a_dev[t0:t1], 1, n, t1 - t0, t0, self.discount,
                                 self._reward_spec, cand_offset=0, returns_in=rets[src] if c > 0 else None,
                                 returns_out=rets[dst], state_out=None if last else state[dst])
        returns = rets[(K - 1) % 2].cpu().numpy().astype(np.float64).reshape(1, n)
        if self._check_status() is False:
            if relaunch:
                raise _lib.L2AError("rollout launch failed twice")
            return self._cem_rollout_pipelined(observations, z, a, a_st, mean2, std2, reference, relaunch=True)
        return returns

    # ------------------------------------------------------------------ CEM (reference :71-106)
    def _cem_normal_device(self, shape, device):
        """Hook for tests: return the iteration's standard normals ``[n, m, D]`` as a CUDA fp32 tensor to inject them;
        ``None`` (the default) lets ``l2a_cem_sample`` draw them on the device (Philox4x32-10 + Box-Muller - every
        rank generates the same numbers: each one keeps all samples and rolls out only its shard)."""
        return None

    def get_cem_action_device(self, observations, retry=False):
        """CEM with sampling, clipping, elite selection and refit on the GPU: the five
        host synchronisations and 5 x n*m*h*act_dim host normals per plan step of the reference loop (``:84-104``)
        disappear; only the chosen action comes back.  Per iteration three hand-written launches around the fused
        rollout (``csrc/l2a_cem.hip``: ``l2a_cem_sample`` - draw, ``a = mean + z * std``, clip, the rollout's
        candidate tensor in one pass; ``l2a_cem_refit`` - elite rows by rank counting instead of a sort, then their
        mean / std).  ``cem_mode='reference'`` keeps the reference's semantics on the device - rollouts on the
        UNCLIPPED samples, candidate-major rows (row = j*m + i read as env row // n), the rank-mask "elites" of
        ``:101`` pooled over the envs; ``cem_mode='fixed'`` uses clipped rollouts, env-major rows and true top-k
        elites per env.  The numbers are the library's own Philox stream, so both modes are validated against the
        host loops with injected normals, not bit-for-bit against NumPy."""
        import ctypes
        from ..dynamics.native_model import _ptr, _stream_ptr
        reference = (self.cem_mode == "reference")
        n, m, h = self.n_candidates, len(observations), self.horizon
        act_dim = self.action_space.shape[0]
        D = h * act_dim
        dev = self._device()
        native = self.dynamics_model.planner_model()
        ctx, lib = native.ctx, native.lib
        num_elites = max(int(n * self.percent_elites), 1)
        low = self._bufs.get("cem_low")
        if low is None or low.device != dev:
            low = self._bufs["cem_low"] = torch.as_tensor(np.asarray(self.action_space.low), dtype=torch.float32, device=dev)
            self._bufs["cem_high"] = torch.as_tensor(np.asarray(self.action_space.high), dtype=torch.float32, device=dev)
        high = self._bufs["cem_high"]
        mean = self._buf("cem_mean", (m, D), torch.float32, dev).zero_()
        std = self._buf("cem_std", (m, D), torch.float32, dev).fill_(1.0)
        rank, world = self._dist()
        lo, hi = self._shard_range(n, rank, world)
        n_local = hi - lo
        widths = [self._shard_range(n, r, world)[1] - self._shard_range(n, r, world)[0] for r in range(world)]
        wmax = max(widths)
        a_clip = self._buf("cem_a_clip", (n, m, D), torch.float32, dev)
        a_raw = self._buf("cem_a_raw", (n, m, D), torch.float32, dev) if reference else None
        seq = self._buf("cem_seq", (h, m * max(n_local, 1), act_dim), torch.float32, dev)
        elite_rows = self._buf("cem_rows", (m * num_elites,), torch.int32, dev)
        rets = None
        obs_dev = self._upload_obs(observations)             # once per plan step, not once per CEM iteration
        # counter-based stream: (seed, calls so far) - identical on every rank; restarts when torch's seed VALUE changes (seeding
        # again with the same value does not rewind it)
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        if self._bufs.get("cem_seed") != seed:
            self._bufs["cem_seed"], self._bufs["cem_calls"] = seed, 0
        call0 = self._bufs["cem_calls"]
        for it in range(self.num_cem_iters):
            z = self._cem_normal_device((n, m, D), dev)
            if z is not None:
                z = z.to(device=dev, dtype=torch.float32).contiguous()
            offset = (call0 + it) * n * m * D
            ctx.check(lib.l2a_cem_sample(ctx.handle, _ptr(z), ctypes.c_ulonglong(seed), ctypes.c_ulonglong(offset),
                                         _ptr(mean), _ptr(std), _ptr(low), _ptr(high), n, m, h, act_dim,
                                         1 if reference else 0, lo, hi, _ptr(a_clip), _ptr(a_raw),
                                         _ptr(seq) if n_local > 0 else None, _stream_ptr(dev)), "l2a_cem_sample")
            if n_local > 0:
                if self.__dict__.get("policy_model") is not None:
                    self._policy_fill(obs_dev, seq, a_clip, n_local, lo)
                _, r_loc = self._rollout(observations, seq, n_local, lo, want_returns=True, obs_dev=obs_dev)
            else:
                r_loc = torch.zeros((m, 0), dtype=torch.float32, device=dev)
            if world > 1:       # shards differ by at most one candidate: pad to the widest for the all-gather
                mine = r_loc if n_local == wmax else torch.cat(
                    [r_loc, torch.zeros((m, wmax - n_local), dtype=r_loc.dtype, device=dev)], dim=1)
                parts = self._all_gather(mine.contiguous(), world)
                rets = torch.cat([part[:, :w] for part, w in zip(parts, widths)], dim=1).to(dev).contiguous()
            else:
                rets = r_loc
            ctx.check(lib.l2a_cem_refit(ctx.handle, _ptr(rets), _ptr(a_clip), n, m, D, num_elites,
                                        1 if reference else 0, float(self.alpha), _ptr(elite_rows), _ptr(mean),
                                        _ptr(std), _stream_ptr(dev)), "l2a_cem_refit")
        # candidates as the rollout saw them: the reference reads the sample memory as [m, n, D] (:92-96) and returns
        # the UNCLIPPED first action (:106); the fixed mode's candidate (i, j) is clipped sample row j * m + i.  ONE launch packs
        # arg-max, that candidate's first action, its return and the final mean / std (`l2a_cem_pick`), one copy brings them back
        # (until round 4: five stock launches and five copies, ~1 % of a config-5 plan step)
        width = act_dim + 2
        packed = self._buf("cem_packed", (m * width + 2 * m * D,), torch.float32, dev)
        ctx.check(lib.l2a_cem_pick(ctx.handle, _ptr(rets), _ptr(a_raw if reference else a_clip), _ptr(mean), _ptr(std), n, m, D,
                                   act_dim, 1 if reference else 0, _ptr(packed), _stream_ptr(dev)), "l2a_cem_pick")
        host = packed.cpu().numpy()
        head = host[:m * width].reshape(m, width)
        out = head[:, :act_dim].astype(np.float64)
        best_return = head[:, act_dim].copy()
        best_index = head[:, act_dim + 1].copy().view(np.int32).astype(np.int64)
        mean_h = host[m * width:m * width + m * D].reshape(m, D).copy()
        std_h = host[m * width + m * D:].reshape(m, D).copy()
        if world > 1:
            # every rank gathered every rank's returns: all of them replay when any launch lost its tile-split partner;
            # the same collective carries the seed digests (ranks seeded differently sampled different normals)
            if self._agree(self._status_flag(), world):
                bad = True
                if not retry:
                    self._force_unsplit()
            else:
                bad = False
        else:
            bad = self._check_status() is False     # a launch lost its tile-split partner: the context is unsplit now
        if bad:
            if retry:
                raise _lib.L2AError("rollout launch failed twice")
            return self.get_cem_action_device(observations, retry=True)      # same counters: the same normals again
        self._bufs["cem_calls"] = call0 + self.num_cem_iters
        self.last_plan = dict(best_index=best_index, best_return=best_return, cem_mean=mean_h, cem_std=std_h)
        if self.__dict__.get("policy_model") is not None:
            self.last_plan["policy_candidates"] = self._n_pi
        return out

    def _native_cem_step(self, observations):
        """``rng="device"`` CEM through the C controller (``l2a_cem_controller_create_device``; at ``world > 1`` this rank's
        ``l2a_cem_controller_create_sharded_device``, whose per-iteration gather of the returns is the int64 MAX all-reduce of
        ``m * n + 3`` words through ``_reduce_payload`` - or the library's communicator, ``L2A_NATIVE_COMM=1``): the same Philox
        offsets as ``get_cem_action_device``, so the two paths can take turns only while they agree on the stream position - the C
        controller is built where the Python path's counter is 0 for this seed and dropped when the Python path has planned since.
        A recurrent planner (``RNNMPCController``) takes ``l2a_lstm_cem_controller_create_device`` / ``_sharded_device``: the
        rollouts start from the controller's hidden state and the state advance with the chosen actions runs inside the same call
        (``_native_step_state`` / ``_native_step_done``, as the random-shooting C step does).
        Returns the actions, or None when the C controller does not apply (parity mode, a library without the recurrent entry
        points, a test hook replaced the normals or the launch path, a backend that cannot reduce the words, a forked child)."""
        self._native_step_done(None)        # (recurrent: no advanced state is pending whenever this call falls back)
        if self.rng != "device" or self._program() or not self._native_step_stock():
            return None
        if getattr(self._cem_normal_device, "__func__", None) is not MPCController._cem_normal_device:
            return None
        rank, world = self._dist()
        native = self.dynamics_model.planner_model()
        recurrent = hasattr(native, "units")
        if not hasattr(native.lib, "l2a_lstm_cem_controller_create_device" if recurrent else "l2a_cem_controller_create_device"):
            return None
        if world > 1 and not hasattr(native.lib, "l2a_lstm_cem_controller_create_sharded_device" if recurrent
                                     else "l2a_cem_controller_create_sharded_device"):
            return None
        n, m, h = self.n_candidates, len(observations), self.horizon
        if m > 64 or m * native.obs_dim > 4096 or native.act_dim > 16:
            return None
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        if self._bufs.get("cem_seed") != seed:
            self._bufs["cem_seed"], self._bufs["cem_calls"] = seed, 0
        num_elites = max(int(n * self.percent_elites), 1)
        key = (id(native), native.handle.value, m, n, h, float(self.discount), seed, self.cem_mode, int(self.num_cem_iters),
               num_elites, float(self.alpha), rank, world)
        st = self._cemstep
        if st is not None and (st.pid != os.getpid() or st.key != key or st.calls != self._bufs["cem_calls"]):
            if st.pid != os.getpid():
                return None                 # (a forked child: the parent's HIP objects did not come along)
            st.close()
            st = self._cemstep = None
        if st is None:
            if self._bufs["cem_calls"] != 0:
                return None                 # the Python path has planned with this seed: its stream position is not the C one's
            from .native_cem_step import NativeCemStep
            shard = None
            if world > 1:
                if self._cemstep_no == key:
                    return None
                shard = self._native_shard(native, rank, world, m * n + 3)
                if shard is None:
                    self._cemstep_no = key
                    return None
            st = NativeCemStep(native, m, n, h, self.action_space.low, self.action_space.high, self.discount, self._reward_spec,
                               self.num_cem_iters, num_elites, self.alpha, self.cem_mode == "reference", seed, shard=shard)
            st.key, st.calls = key, 0
            self._cemstep = st
        self._check_blocks(m)
        state, keep = self._native_step_state(native, m)
        st.step(observations, torch.cuda.current_stream(native.device).cuda_stream, state)
        self._native_step_done(keep)
        st.calls += int(self.num_cem_iters)
        self._bufs["cem_calls"] = st.calls
        mean, std, rets = st.result()
        self.last_plan = dict(best_index=st.idx.copy(), best_return=st.ret.copy(), cem_mean=mean, cem_std=std,
                              cem_trace=[dict(returns=rets[it]) for it in range(rets.shape[0])])
        if world > 1:
            self.last_plan["shard"] = self._shard_range(n, rank, world)
        return st.act.copy()

    def get_cem_action(self, observations):
        if not self._fusable():
            raise _lib.L2AError("CEM planning needs a fusable closed-form reward (env.reward_spec: a RewardSpec or a RewardProgram) "
                                "or, with use_reward_model, a reward model the library scores (MLPRewardModel)")
        if self.native_cem_step:
            out = self._native_cem_step(observations)
            if out is not None:
                return out
        if self.rng == "device":
            return self.get_cem_action_device(observations)
        n = self.n_candidates
        m = len(observations)
        h = self.horizon
        act_dim = self.action_space.shape[0]
        num_elites = max(int(self.n_candidates * self.percent_elites), 1)
        mean = np.zeros((m, h * act_dim))
        std = np.ones((m, h * act_dim))
        clip_low = np.concatenate([self.action_space.low] * h)
        clip_high = np.concatenate([self.action_space.high] * h)

        rank, world = self._dist()
        lo, hi = self._shard_range(n, rank, world)
        trace = []
        cand_a = None
        returns = None

        for it in range(self.num_cem_iters):
            mean, std, returns, cand_a = self._cem_iteration(observations, mean, std, num_elites,
                                                             clip_low, clip_high, lo, hi, world)
            trace.append(dict(mean=np.array(mean), std=np.array(std), returns=returns))

        idx = np.argmax(returns, axis=1)
        self.last_plan = dict(best_index=idx, best_return=returns[range(m), idx], cem_trace=trace)
        return cand_a[range(m), idx]

    # ------------------------------------------------------------------ what MPPI and iCEM share: a plan that persists from step to step
    # `prefix` ("mppi" / "icem") names the planner's `_bufs` keys, its `_<prefix>step` / `_<prefix>_side` attributes and its hooks.
    def _warm_reset(self, prefix, step, dones):
        """``reset(dones)`` for a planner whose plan persists: the marked envs' next step starts afresh; ``None``, or a number of envs
        other than the plan's, starts all of them afresh.  ``step``: the planner's C controller, or None."""
        if step is not None and step.pid == os.getpid():    # the C controller holds the plan: the marks go to it
            step.reset(None if dones is None or len(dones) != step.m else dones)
        fresh = self._bufs.get(prefix + "_fresh")
        if dones is None or fresh is None or len(fresh) != len(dones):
            self._bufs[prefix + "_fresh"] = None
        else:
            fresh |= np.asarray(dones, dtype=bool)

    def _warm_open(self, prefix, m, dev):
        """Opens a plan step of the planner's Python loop: ``(low, high, sigma, shifts, first, cur, seed, call0)`` - the constants
        on the device, the shift table ``[+1 | 0 | -1][m]``, iteration 0's shift vector (a fresh start for an env that is new or was
        reset, one step on for the others), the committed copy of the three rotating copies of the plan - a step reads ``cur`` and
        commits its last outputs only when it succeeded (``_warm_commit``), so a replay starts from the same plan -, and the
        counter-based stream ``(seed, iterations so far)``, which restarts when torch's seed VALUE changes, as CEM's does."""
        bufs = self._bufs
        const = bufs.get(prefix + "_const")
        if const is None or const[0].device != dev:
            up = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=dev)  # noqa: E731
            sigma = getattr(self, "_%s_sigma_vector" % prefix)()
            const = bufs[prefix + "_const"] = (up(self.action_space.low), up(self.action_space.high), up(sigma))
        shifts = bufs.get(prefix + "_shifts")
        if shifts is None or shifts.device != dev or shifts.shape[1] != m:
            shifts = bufs[prefix + "_shifts"] = torch.as_tensor(np.array([[1] * m, [0] * m, [-1] * m], dtype=np.int32), device=dev)
            bufs[prefix + "_fresh"], bufs[prefix + "_cur"] = None, 0
        fresh = bufs.get(prefix + "_fresh")
        if fresh is None:
            first = shifts[2]                                   # every env starts afresh
        elif fresh.any():
            first = torch.as_tensor(np.where(fresh, -1, 1).astype(np.int32), device=dev)
        else:
            first = shifts[0]
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        if bufs.get(prefix + "_seed") != seed:
            bufs[prefix + "_seed"], bufs[prefix + "_calls"] = seed, 0
        return const + (shifts, first, bufs[prefix + "_cur"], seed, bufs[prefix + "_calls"])

    @staticmethod
    def _spare_copy(src, cur):
        """The copy of the plan an iteration writes: neither the one it reads nor the committed one."""
        return [b for b in range(3) if b != src and b != cur][0]

    def _flagged(self, retry):
        """True when a launch of this step lost its tile-split partner - the context is unsplit now, and the caller plans the same
        step again (same counters, same starting plan) with ``retry=True``; a second flag raises."""
        if self._check_status() is not False:
            return False
        if retry:
            raise _lib.L2AError("rollout launch failed twice")
        return True

    def _warm_commit(self, prefix, m, calls, cur):
        """A step that succeeded moves the planner on: the stream position, the committed copy, and no env is new any more."""
        self._bufs[prefix + "_calls"] = calls
        self._bufs[prefix + "_cur"] = cur
        self._bufs[prefix + "_fresh"] = np.zeros(m, dtype=bool)

    def _native_warm_step(self, prefix, observations, plan):
        """One plan step through the planner's C controller (``_native_mppi_step`` / ``_native_icem_step``), up to and including the
        step call.  The plan persists on the side that planned, so the choice is made on the controller's first step of this kind
        and kept; ``reset(dones)`` is forwarded to the C controller (``_warm_reset``), and a changed ``torch.initial_seed()`` value
        reseeds it (the stream restarts, the plan is kept - as the Python loop does).  ``plan(native, m, n, h)`` returns ``(facts,
        eligible, make)``: the planner's own part of the key a C controller is kept under (a controller under another key is
        dropped: another plan starts afresh, as the Python loop's), what of its own keeps the C controller from planning, and
        ``make(seed, shard)``, which builds it.  Returns ``(step, n, rank, world)``, or None: the Python loop plans, now and later."""
        side, attr = "_%s_side" % prefix, "_%sstep" % prefix
        if getattr(self, side) == "python":
            return None
        st = getattr(self, attr)
        if st is not None and st.pid != os.getpid():
            setattr(self, attr, None)       # (a forked child: the parent's HIP objects did not come along)
            setattr(self, side, "python")
            return None
        rank, world = self._dist()
        n, m, h = self.n_candidates, len(observations), self.horizon
        seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        native = self.dynamics_model.planner_model()
        facts, eligible, make = plan(native, m, n, h)
        key = (id(native), native.handle.value, m, n, h, float(self.discount)) + facts + (rank, world)
        if st is not None and st.key != key:
            st.close()
            st = None
            setattr(self, attr, None)
        if st is None:
            ok = eligible and not (self.use_reward_model or self._program() or hasattr(native, "units") or not self._native_step_stock()
                                   or not hasattr(native.lib, "l2a_%s_controller_create_sharded_device" % prefix)
                                   or m > 64 or m * native.obs_dim > 4096 or native.act_dim > 16)
            shard = self._native_shard(native, rank, world, m * n + 3) if ok and world > 1 else None    # (the shard dry run)
            if not ok or (world > 1 and shard is None):
                setattr(self, side, "python")
                return None
            st = make(seed, shard)
            st.key, st.seed = key, seed
            setattr(self, attr, st)
            setattr(self, side, "c")
        if st.seed != seed:
            st.reseed(seed)
            st.seed = seed
        self._check_blocks(m)
        st.step(observations, torch.cuda.current_stream(native.device).cuda_stream)
        return st, n, rank, world

    # ------------------------------------------------------------------ MPPI (PDDM's filtered, reward-weighted refinement)
    def _mppi_sigma_vector(self):
        """``mppi_sigma`` as an fp32 ``[act_dim]`` array: ``None`` = a quarter of each dimension's action range, a scalar = that
        value for every dimension, or one value per dimension; finite and non-negative."""
        return self._sigma_vector(self.mppi_sigma, "mppi_sigma")

    def _sigma_vector(self, value, name):
        low = np.asarray(self.action_space.low, dtype=np.float64)
        high = np.asarray(self.action_space.high, dtype=np.float64)
        if value is None:
            sigma = 0.25 * (high - low)
        else:
            sigma = np.asarray(value, dtype=np.float64)
            if sigma.ndim == 0:
                sigma = np.full(low.shape, float(sigma))
        if sigma.shape != low.shape:
            raise ValueError("%s must be None, a scalar or one value per action dimension %s, got shape %s"
                             % (name, low.shape, sigma.shape))
        if not (np.isfinite(sigma).all() and (sigma >= 0).all()):
            raise ValueError("%s must be finite and non-negative" % name)
        return sigma.astype(np.float32)

    def _mppi_reset(self, dones):
        """``reset(dones)`` for the MPPI planner: the marked envs' next step starts from a zero mean; ``None``, or a number of envs
        other than the plan's, starts all of them afresh.  Without ``use_mppi`` nothing happens."""
        if self.use_mppi:
            self._warm_reset("mppi", self._mppistep, dones)

    def _mppi_normal_device(self, shape, device):
        """Hook for tests: return the iteration's standard normals ``[n, m, D]`` as a CUDA fp32 tensor to inject them; ``None``
        (the default) lets ``l2a_mppi_sample`` draw them on the device (Philox4x32-10 + Box-Muller, CEM's stream)."""
        return None

    mppi_fetch_returns = True       # `_native_mppi_step`: copy the last iteration's returns [m, n] into `last_plan` on every step

    def _native_mppi_step(self, observations):
        """The MPPI plan step through the C controller (``l2a_mppi_controller_create_device``; at ``world > 1`` this rank's
        ``l2a_mppi_controller_create_sharded_device``, whose per-iteration gather of the returns is the int64 MAX all-reduce of
        ``m * n + 3`` words through ``_reduce_payload`` - or the library's communicator, ``L2A_NATIVE_COMM=1``): the Philox offsets,
        the shift rule and the bits of ``get_mppi_action``.  None (``_native_warm_step``: the Python loop plans, now and later) for
        a reward program, a reward model, a recurrent model, a test hook that replaced the normals or the launch path, a library
        without the entry points, a backend that cannot reduce the words, a forked child.  ``last_plan`` gets
        ``get_mppi_action``'s keys; the step itself reads back ``m * (act_dim + 4)`` floats only, the mean and the returns are
        copies of their own afterwards: ``returns`` is fetched eagerly by default, and the class or instance attribute
        ``mppi_fetch_returns = False`` leaves the key out and the ``m * n`` floats on the device (``self._mppistep.result()`` still
        returns every iteration's table on request)."""
        def plan(native, m, n, h):
            sigma = self._mppi_sigma_vector()
            hooked = getattr(self._mppi_normal_device, "__func__", None) is not MPCController._mppi_normal_device

            def make(seed, shard):
                from .native_mppi_step import NativeMppiStep
                return NativeMppiStep(native, m, n, h, self.action_space.low, self.action_space.high, self.discount, self._reward_spec,
                                      self.mppi_iters, self.mppi_kappa, self.mppi_beta, sigma, seed, shard=shard)
            return (int(self.mppi_iters), self.mppi_kappa, self.mppi_beta, sigma.tobytes()), not hooked, make

        stepped = self._native_warm_step("mppi", observations, plan)
        if stepped is None:
            return None
        st, n, rank, world = stepped
        mean, ess, valid, rets = st.result(with_returns=bool(self.mppi_fetch_returns))
        self.last_plan = dict(best_index=st.idx.copy(), best_return=st.ret.copy(), mppi_mean=mean, mppi_ess=ess, mppi_valid=valid)
        if rets is not None:
            self.last_plan["returns"] = rets[-1]
        if world > 1:
            self.last_plan["shard"] = self._shard_range(n, rank, world)
        return st.act.copy()

    def get_mppi_action(self, observations, retry=False):
        """One MPPI plan step on the GPU (``csrc/l2a_mppi.hip``; semantics in ``include/l2a.h``).  The plan mean ``[m, h * act_dim]``
        stays on the device between controller steps.  Per iteration: ``l2a_mppi_sample`` (shift - zeros for an env that is new
        or was reset, one step on for the first iteration of a later step, none for further iterations -, filtered noise, clip,
        the rollout's candidate tensor), the fused rollout for the returns (``_rollout``: closed-form reward, reward program or
        reward model alike), ``l2a_mppi_update`` (weights ``exp(kappa (R - Rmax))`` over the candidates whose return is neither NaN
        nor ``-inf``, the weighted mean of the clipped samples).  The observations go up once, one copy brings the packed result
        back.  The action returned is the new mean's first step.  The normals of iteration ``it`` of the s-th step are the Philox
        stream under ``torch.initial_seed()`` at offset ``(s * mppi_iters + it) * n * m * D`` (its own counter, not CEM's)."""
        import ctypes
        from ..dynamics.native_model import _ptr, _stream_ptr
        if not self._fusable():
            raise _lib.L2AError("MPPI planning needs a fusable closed-form reward (env.reward_spec: a RewardSpec or a RewardProgram) "
                                "or, with use_reward_model, a reward model the library scores (MLPRewardModel)")
        if self.rng != "device":
            raise _lib.L2AError("MPPI planning draws its normals on the device (rng='device'); NumPy normals are not supported")
        if self.native_cem_step:
            raise _lib.L2AError("an MPPI step as one C controller call is native_mppi_step=True: leave native_cem_step off with use_mppi")
        if self.native_mppi_step and not retry:
            out = self._native_mppi_step(observations)
            if out is not None:
                return out
        if self._dist()[1] > 1:
            raise _lib.L2AError("MPPI planning does not shard its candidates over torch.distributed ranks in this Python loop: pass "
                                "shard_candidates=False (every rank then plans on its own), or native_mppi_step=True (the C controller "
                                "shards a plan with a closed-form reward spec and an MLP model)")
        n, m, h = self.n_candidates, len(observations), self.horizon
        act_dim = self.action_space.shape[0]
        D = h * act_dim
        dev = self._device()
        native = self.dynamics_model.planner_model()
        ctx, lib = native.ctx, native.lib
        if not hasattr(lib, "l2a_mppi_sample"):
            raise _lib.L2AError("this libl2a_hip.so has no MPPI kernels (l2a_mppi_sample): rebuild it")
        low, high, sigma, shifts, first, cur, seed, call0 = self._warm_open("mppi", m, dev)
        means = self._buf("mppi_means", (3, m, D), torch.float32, dev)      # the persistent mean and two scratch means
        a_clip = self._buf("mppi_a_clip", (n, m, D), torch.float32, dev)
        seq = self._buf("mppi_seq", (h, m * n, act_dim), torch.float32, dev)
        width = act_dim + 4
        packed = self._buf("mppi_packed", (m * width + m * D + m * n,), torch.float32, dev)
        obs_dev = self._upload_obs(observations)                # once per plan step
        src = cur
        rets = None
        for it in range(self.mppi_iters):
            dst = self._spare_copy(src, cur)
            z = self._mppi_normal_device((n, m, D), dev)
            if z is not None:
                z = z.to(device=dev, dtype=torch.float32).contiguous()
            offset = (call0 + it) * n * m * D
            ctx.check(lib.l2a_mppi_sample(ctx.handle, _ptr(z), ctypes.c_ulonglong(seed), ctypes.c_ulonglong(offset & 0xFFFFFFFFFFFFFFFF),
                                          _ptr(means[src]), _ptr(first if it == 0 else shifts[1]), _ptr(sigma), self.mppi_beta,
                                          _ptr(low), _ptr(high), n, m, h, act_dim, _ptr(means[dst]), _ptr(a_clip), _ptr(seq),
                                          _stream_ptr(dev)), "l2a_mppi_sample")
            if self.__dict__.get("policy_model") is not None:
                self._policy_fill(obs_dev, seq, a_clip, n, 0)
            _, rets = self._rollout(observations, seq, n, 0, want_returns=True, obs_dev=obs_dev)
            ctx.check(lib.l2a_mppi_update(ctx.handle, _ptr(rets), _ptr(a_clip), n, m, h, act_dim, self.mppi_kappa, _ptr(means[dst]),
                                          _ptr(packed), _stream_ptr(dev)), "l2a_mppi_update")
            src = dst
        packed[m * width:m * width + m * D].view(m, D).copy_(means[src])
        packed[m * width + m * D:].view(m, n).copy_(rets)
        host = packed.cpu().numpy()
        if self._flagged(retry):
            return self.get_mppi_action(observations, retry=True)       # same counters, same starting mean: the same step again
        self._warm_commit("mppi", m, call0 + self.mppi_iters, src)
        head = host[:m * width].reshape(m, width)
        self.last_plan = dict(best_index=head[:, act_dim + 1].copy().view(np.int32).astype(np.int64),
                              best_return=head[:, act_dim].copy(),
                              returns=host[m * width + m * D:].reshape(m, n).copy(),
                              mppi_mean=host[m * width:m * width + m * D].reshape(m, D).copy(),
                              mppi_ess=head[:, act_dim + 2].copy(),
                              mppi_valid=head[:, act_dim + 3].copy().view(np.int32).astype(np.int64))
        if self.__dict__.get("policy_model") is not None:
            self.last_plan["policy_candidates"] = self._n_pi
        return head[:, :act_dim].astype(np.float64)

    # ------------------------------------------------------------------ iCEM (Pinneri et al. 2020: CEM with memory and coloured noise)
    def _icem_sigma_vector(self):
        """``icem_sigma`` (the spread a plan starts from, and re-opens to at every step) as an fp32 ``[act_dim]`` array, resolved as
        ``mppi_sigma`` is."""
        return self._sigma_vector(self.icem_sigma, "icem_sigma")

    def _icem_sizes(self):
        """``(K, Kk, [n_it per iteration])``: elites ``K = max(int(n * percent_elites), 1)``, kept elites ``Kk = int(icem_keep * K)``
        (0 is allowed), populations ``n_it = min(n, max(int(n / icem_decay ** it), 2 K))`` - in double precision, on the host."""
        n = int(self.n_candidates)
        K = max(int(n * self.percent_elites), 1)
        Kk = int(self.icem_keep * K)
        return K, Kk, [min(n, max(int(n / self.icem_decay ** it), 2 * K)) for it in range(self.icem_iters)]

    def _icem_noise_matrix(self, h):
        """The power-law matrix ``M [h, h]`` (host fp32) of ``icem_beta``: ``l2a_icem_noise_matrix`` (``include/l2a.h``), built on
        the host in double precision.  ``L2AError`` for a horizon above 128 or a library without the entry point."""
        lib = _lib.load()
        if not hasattr(lib, "l2a_icem_noise_matrix"):
            raise _lib.L2AError("this libl2a_hip.so has no power-law iCEM noise (l2a_icem_sample_noise): rebuild it")
        M = np.empty((int(h), int(h)), dtype=np.float32)
        if lib.l2a_icem_noise_matrix(int(h), float(self.icem_beta), M.ctypes.data) != _lib.L2A_OK:
            raise _lib.L2AError("icem_noise='powerlaw' plans over horizons of 1 .. 128 steps (L2A_ICEM_NOISE_MAX_H) with icem_beta in "
                                "[0, 8]: horizon %d, icem_beta %r" % (h, self.icem_beta))
        return M

    def _icem_reset(self, dones):
        """``reset(dones)`` for the iCEM planner: the marked envs' next step starts from a zero mean, the initial spread and no kept
        elites; ``None``, or a number of envs other than the plan's, starts all of them afresh.  Without ``use_icem`` nothing happens."""
        if self.use_icem:
            self._warm_reset("icem", self._icemstep, dones)

    def _icem_normal_device(self, shape, device):
        """Hook for tests: return the iteration's standard normals ``[n_it, m, D]`` as a CUDA fp32 tensor to inject them; ``None``
        (the default) lets ``l2a_icem_sample`` draw them on the device (Philox4x32-10 + Box-Muller, CEM's stream)."""
        return None

    icem_trace_returns = False      # copy EVERY iteration's returns into `last_plan["icem_trace"]` (tests); the last one's always come

    icem_fetch_returns = True       # `_native_icem_step`: copy the returns into `last_plan` on every step (the last iteration's table;
                                    # with `icem_trace_returns` every iteration's)

    @staticmethod
    def _icem_trace(heads, pops, tables):
        """``last_plan["icem_trace"]`` from the refits' result rows ``heads [iters, m, act_dim + 4]`` (the action | best return | best
        index | elite count | valid count, the integers by their bits): per iteration n, best return and index, elite and valid
        counts, and as ``returns`` a copy of ``tables[it] [m, pops[it]]`` where that is not None."""
        at = heads.shape[2] - 4
        as_int = lambda a: a.copy().view(np.int32).astype(np.int64)     # noqa: E731
        steps = []
        for it, n_it in enumerate(pops):
            step = dict(n=n_it, best_return=heads[it, :, at].copy(), best_index=as_int(heads[it, :, at + 1]),
                        elites=as_int(heads[it, :, at + 2]), valid=as_int(heads[it, :, at + 3]))
            if tables[it] is not None:
                step["returns"] = tables[it].copy()
            steps.append(step)
        return steps

    def _native_icem_step(self, observations):
        """The iCEM plan step through the C controller (``l2a_icem_controller_create_device``; at ``world > 1`` this rank's
        ``l2a_icem_controller_create_sharded_device``, whose per-iteration gather of the returns is the int64 MAX all-reduce of
        ``m * pops[it] + 3`` words through ``_reduce_payload`` - or the library's communicator, ``L2A_NATIVE_COMM=1``): the Philox
        offsets, the shift rule, the rotation of the state and the bits of ``get_icem_action``.  None (``_native_warm_step``: the
        Python loop plans, now and later) for a reward program, a reward model, a particle plan, a recurrent model, a test hook that
        replaced the normals or the launch path, a library without the entry points, a backend that cannot reduce the words, a
        forked child.  ``last_plan`` gets ``get_icem_action``'s keys; the step itself reads back ``icem_iters * m * (act_dim + 4)``
        floats only, the state and the returns are one copy of their own afterwards: the class or instance attribute
        ``icem_fetch_returns = False`` leaves every ``returns`` key out and the tables on the device (``self._icemstep.result()``
        still returns every iteration's table on request); with ``icem_trace_returns`` every iteration's table is filled in,
        otherwise the last one's."""
        def plan(native, m, n, h):
            sigma = self._icem_sigma_vector()
            K, Kk, pops = self._icem_sizes()
            hooked = getattr(self._icem_normal_device, "__func__", None) is not MPCController._icem_normal_device

            def make(seed, shard):
                from .native_icem_step import NativeIcemStep
                st = NativeIcemStep(native, m, n, h, self.action_space.low, self.action_space.high, self.discount, self._reward_spec,
                                    pops, K, Kk, self.alpha, self.icem_rho, sigma, self.icem_add_mean, seed, shard=shard)
                if self.icem_noise == "powerlaw":
                    try:
                        st.set_noise(self._icem_noise_matrix(h))
                    except Exception:
                        st.close()
                        raise
                return st
            return (K, Kk, tuple(pops), float(self.alpha), self.icem_rho, sigma.tobytes(), self.icem_add_mean, self.icem_noise,
                    self.icem_beta), not hooked and self.ensemble_planning != "particles", make

        stepped = self._native_warm_step("icem", observations, plan)
        if stepped is None:
            return None
        st, _, rank, world = stepped
        pops =[int(n_it) for n_it in st.pops]
        fetch, trace = bool(self.icem_fetch_returns), bool(self.icem_trace_returns)
        mean, std, elites, counts, head, rets = st.result(with_returns=fetch)
        steps = self._icem_trace(head, pops, [rets[it] if fetch and (trace or it == st.iters - 1) else None for it in range(st.iters)])
        last = steps[-1]
        self.last_plan = dict(best_index=last["best_index"], best_return=last["best_return"], icem_mean=mean, icem_std=std,
                              icem_elites=elites, icem_elite_count=counts, icem_valid=last["valid"], icem_trace=steps,
                              icem_noise=np.str_(self.icem_noise), icem_beta=np.float64(self.icem_beta))
        if fetch:
            self.last_plan["returns"] = last["returns"]
        if world > 1:
            self.last_plan["shard"] = [self._shard_range(n_it, rank, world) for n_it in pops]
        return st.act.copy()

    def get_icem_action(self, observations, retry=False):
        """One iCEM plan step on the GPU (``csrc/l2a_icem.hip``; semantics in ``include/l2a.h``).  Per env the plan mean, the spread
        ``[m, h * act_dim]``, the kept elites ``[m, Kk, h * act_dim]`` and their counts stay on the device between controller steps.
        Per iteration: ``l2a_icem_sample`` (shift - a fresh start for an env that is new or was reset, one step on with the spread
        re-opened for the first iteration of a later step, none for further iterations -, the kept elites as the first rows, AR(1)
        noise - with ``icem_noise="powerlaw"`` ``l2a_icem_sample_noise`` and the power-law matrix of ``icem_beta`` instead -, clip,
        with ``icem_add_mean`` the mean itself as the last iteration's last row), the fused rollout of the iteration's
        ``n_it`` candidates (``_rollout``: closed-form reward, reward program, reward model and particle plans alike),
        ``l2a_icem_refit`` (top-k of the valid candidates, momentum update of mean and spread, the kept elites, the packed result).
        The observations go up once, one copy brings the packed result back.  The action returned is the first action of the last
        iteration's best candidate.  The normals of iteration ``it`` of the s-th step are the Philox stream under
        ``torch.initial_seed()`` at offset ``(s * icem_iters + it) * n * m * D`` - the stride is the full ``n``, and the counter is the
        planner's own, not CEM's or MPPI's.  State and counter are committed only when the launch status was read clean: a flagged
        tile-split launch replays the step from the same state with the same offsets.  ``last_plan``: ``best_index``, ``best_return``,
        ``returns`` (the last iteration's), ``icem_mean``, ``icem_std``, ``icem_elites [m, Kk, D]`` (env i's kept rows in rank order: its
        first ``icem_elite_count[i]`` rows, zeros behind them), ``icem_valid``, ``icem_trace`` (per iteration: n, best return and index,
        elite and valid counts), ``icem_noise``, ``icem_beta`` (as NumPy scalars: every entry but the trace has a dtype)."""
        import ctypes
        from ..dynamics.native_model import _ptr, _stream_ptr
        if not self._fusable():
            raise _lib.L2AError("iCEM planning needs a fusable closed-form reward (env.reward_spec: a RewardSpec or a RewardProgram) "
                                "or, with use_reward_model, a reward model the library scores (MLPRewardModel)")
        if self.rng != "device":
            raise _lib.L2AError("iCEM planning draws its normals on the device (rng='device'); NumPy normals are not supported")
        if self.native_cem_step or self.native_mppi_step:
            raise _lib.L2AError("an iCEM step as one C controller call is native_icem_step=True: leave native_cem_step and "
                                "native_mppi_step off with use_icem")
        if self.native_icem_step and not retry:
            out = self._native_icem_step(observations)
            if out is not None:
                return out
        if self._dist()[1] > 1:
            raise _lib.L2AError("iCEM planning does not shard its candidates over torch.distributed ranks in this Python loop: pass "
                                "shard_candidates=False (every rank then plans on its own), or native_icem_step=True (the C controller "
                                "shards a plan with a closed-form reward spec and an MLP model)")
        n, m, h = self.n_candidates, len(observations), self.horizon
        act_dim = self.action_space.shape[0]
        D = h * act_dim
        K, Kk, pops = self._icem_sizes()
        iters = self.icem_iters
        dev = self._device()
        native = self.dynamics_model.planner_model()
        ctx, lib = native.ctx, native.lib
        if not hasattr(lib, "l2a_icem_sample"):
            raise _lib.L2AError("this libl2a_hip.so has no iCEM kernels (l2a_icem_sample): rebuild it")
        low, high, sigma, shifts, first, cur, seed, call0 = self._warm_open("icem", m, dev)
        noise = None
        if self.icem_noise == "powerlaw":       # M once per (h, beta), kept on the device next to the constants
            held = self._bufs.get("icem_noise")
            if held is None or held[0] != (h, self.icem_beta) or held[1].device != dev:
                held = self._bufs["icem_noise"] = ((h, self.icem_beta), torch.as_tensor(self._icem_noise_matrix(h), device=dev))
            noise = held[1]
        # the persistent state and two scratch copies of it
        means = self._buf("icem_means", (3, m, D), torch.float32, dev)
        stds = self._buf("icem_stds", (3, m, D), torch.float32, dev)
        kept = self._buf("icem_kept", (3, m, max(Kk, 1), D), torch.float32, dev)
        kcs = self._buf("icem_kc", (3, m), torch.int32, dev)
        work = self._buf("icem_work", (m, K), torch.int32, dev)
        a_clip =self._buf("icem_a_clip", (n, m, D), torch.float32, dev)
        seq_all = self._buf("icem_seq", (h * m * n * act_dim,), torch.float32, dev)
        width = act_dim + 4
        trace = bool(self.icem_trace_returns)
        # one buffer, one read-back: every iteration's result rows | mean | std | kept rows | kept counts | returns
        sizes = [iters * m * width, m * D, m * D, m * Kk * D, m, m * (sum(pops) if trace else pops[-1])]
        at = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
        packed = self._buf("icem_packed", (at[-1],), torch.float32, dev)
        heads = packed[:at[1]].view(iters, m, width)
        obs_dev = self._upload_obs(observations)                # once per plan step
        src = cur
        ret_at = at[5]
        for it in range(iters):
            n_it = pops[it]
            dst = self._spare_copy(src, cur)
            z = self._icem_normal_device((n_it, m, D), dev)
            if z is not None:
                z = z.to(device=dev, dtype=torch.float32).contiguous()
            offset = (call0 + it) * n * m * D
            seq = seq_all[:h * m * n_it * act_dim].view(h, m * n_it, act_dim)
            # (the two entries differ in one argument: the AR(1) coefficient, or the device matrix of nz = M z)
            sample, name = (lib.l2a_icem_sample, "l2a_icem_sample") if noise is None else (lib.l2a_icem_sample_noise, "l2a_icem_sample_noise")
            ctx.check(sample(ctx.handle, _ptr(z), ctypes.c_ulonglong(seed), ctypes.c_ulonglong(offset & 0xFFFFFFFFFFFFFFFF),
                             _ptr(means[src]), _ptr(stds[src]), _ptr(kept[src]) if Kk else None,
                             _ptr(kcs[src]) if Kk else None, _ptr(first if it == 0 else shifts[1]), _ptr(sigma),
                             self.icem_rho if noise is None else _ptr(noise), _ptr(low), _ptr(high), n_it, m, h, act_dim, Kk,
                             int(self.icem_add_mean and it == iters - 1), _ptr(means[dst]), _ptr(stds[dst]), _ptr(a_clip),
                             _ptr(seq), _stream_ptr(dev)), name)
            _, rets = self._rollout(observations, seq, n_it, 0, want_returns=True, obs_dev=obs_dev)
            ctx.check(lib.l2a_icem_refit(ctx.handle, _ptr(rets), _ptr(a_clip), _ptr(low), _ptr(high), n_it, m, h, act_dim, K, Kk,
                                         float(self.alpha), _ptr(work), _ptr(means[dst]), _ptr(stds[dst]),
                                         _ptr(kept[dst]) if Kk else None, _ptr(kcs[dst]), _ptr(heads[it]), _stream_ptr(dev)),
                      "l2a_icem_refit")
            if trace or it == iters - 1:
                packed[ret_at:ret_at + m * n_it].view(m, n_it).copy_(rets)
                ret_at += m * n_it
            src = dst
        packed[at[1]:at[2]].view(m, D).copy_(means[src])
        packed[at[2]:at[3]].view(m, D).copy_(stds[src])
        if Kk:
            packed[at[3]:at[4]].view(m, Kk, D).copy_(kept[src])
        packed[at[4]:at[5]].view(torch.int32).copy_(kcs[src])
        host = packed.cpu().numpy()
        if self._flagged(retry):
            return self.get_icem_action(observations, retry=True)       # same counters, same starting state: the same step again
        self._warm_commit("icem", m, call0 + iters, src)
        head = host[:at[1]].reshape(iters, m, width)
        ret_at, tables = at[5], []
        for it in range(iters):             # the returns tables that came back: every iteration's, or the last one's
            size = m * pops[it] if trace or it == iters - 1 else 0
            tables.append(host[ret_at:ret_at + size].reshape(m, pops[it]) if size else None)
            ret_at += size
        steps = self._icem_trace(head, pops, tables)
        last = steps[-1]
        # the refit writes an env's first `count` kept rows only: what lies behind them in the buffer is no elite of this step
        elites, counts = host[at[3]:at[4]].reshape(m, Kk, D).copy(), host[at[4]:at[5]].copy().view(np.int32).astype(np.int64)
        for i in range(m):
            elites[i, counts[i]:] = 0.0
        self.last_plan = dict(best_index=last["best_index"], best_return=last["best_return"], returns=last["returns"],
                              icem_mean=host[at[1]:at[2]].reshape(m, D).copy(), icem_std=host[at[2]:at[3]].reshape(m, D).copy(),
                              icem_elites=elites, icem_elite_count=counts, icem_valid=last["valid"], icem_trace=steps,
                              icem_noise=np.str_(self.icem_noise), icem_beta=np.float64(self.icem_beta))
        return head[-1, :, :act_dim].astype(np.float64)
