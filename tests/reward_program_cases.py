"""Shared builders of the reward-program tests (CPU and GPU): the programs, and an env that declares one."""

import numpy as np

from learning_to_adapt_amd.envs import RewardProgram, SyntheticEnv


def every_kind_program(obs_dim, act_dim):
    """Every term kind and every source once: a SQSUM whose range ends at ``obs_dim``, a NORM with a target, and the
    large terms (SQSUM, NORM) with coefficients of one sign, so that they do not cancel each other."""
    goal = np.array([0.5, -1.25, 2.0])
    return (RewardProgram().with_bias(0.5)
            .linear("obs", min(3, obs_dim - 1), 0.3)
            .linear("delta", obs_dim - 2, 0.7)
            .in_range("next", 5, -2.0, 3.5, coef=2.0)
            .sqsum("act", 0, act_dim, -0.05)
            .sqsum("obs", obs_dim - 4, 4, -0.01)
            .norm("next", 0, 3, -0.1, target=goal)
            .norm("delta", 2, 2, -0.2))


def new_reward_program(obs_dim, act_dim, dt):
    """A reward none of the reference's envs has: ``bias + LINEAR(DELTA) / dt + INRANGE(NEXT height) - SQSUM(ACT) -
    NORM(NEXT[0:3] - goal)``."""
    goal = np.array([0.3, -0.2, 0.1])
    return (RewardProgram().with_bias(0.1)
            .linear("delta", obs_dim - 3, 1.0, div=dt)
            .in_range("next", 1, -0.5, 0.5, coef=1.0)
            .sqsum("act", 0, act_dim, -0.05)
            .norm("next", 0, 3, -1.0, target=goal))


def program_env(kind, program=None):
    """A ``SyntheticEnv`` whose reward is a program (``SyntheticEnv.reward`` evaluates ``reward_spec``)."""
    env = SyntheticEnv(kind)
    od, ad = env.observation_space.shape[0], env.action_space.shape[0]
    env.reward_spec = program if program is not None else new_reward_program(od, ad, env.dt)
    return env
