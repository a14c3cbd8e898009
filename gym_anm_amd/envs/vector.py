"""NumPy-facing vector-environment adapter.

RL libraries that drive ``gymnasium.vector.VectorEnv``-style environments from the host (NumPy actions
in, NumPy observations out) can wrap any batched environment of this package with it.  The simulator
step itself stays on the GPU; the adapter adds one host-to-device copy of the actions and one
device-to-host copy of (obs, reward, terminated) per step, i.e. the PCIe round trip DESIGN.md prices.
Trainers that keep their policy on the GPU should use the batched environment directly.

The reference has no vector environment (one ``ANMEnv`` object per environment, anm_env.py:17-156); the
attribute names below are Gymnasium's (``num_envs``, ``single_action_space``,
``single_observation_space``), the autoreset convention is Gymnasium's "next-step" mode, which is what
the in-kernel autoreset implements.
"""

from __future__ import annotations

import numpy as np
import torch


class NumpyVectorEnv:
    metadata = {"autoreset_mode": "next_step", "render_modes": []}

    def __init__(self, env):
        if not getattr(env, "autoreset", False):
            raise ValueError("NumpyVectorEnv needs an environment built with autoreset=True")
        self.env = env
        self.num_envs = env.num_envs
        self.single_action_space = env.action_space
        self.single_observation_space = env.observation_space
        self.action_space = env.action_space          # per-environment Box; actions are [num_envs, A]
        self.observation_space = env.observation_space
        # (action_map= / obs_map=: the two spaces above are the mapped ones, [-1, 1] and the Box of images; MW / MVAr here)
        self.raw_action_space = getattr(env, "raw_action_space", env.action_space)
        self.render_mode = None
        env.check_actions = False                     # checked here on the host, where the data already is
        self._pinned = None
        # episode statistics kept by the step kernels (BatchedANMEnv(episode_stats=True)): reported like Gymnasium's vector
        # RecordEpisodeStatistics, the rows whose episode ended at a step found from the change of `episodes_done`
        self._stats = bool(getattr(env, "episode_stats", False))
        self._n_done = env.episodes_done.cpu().numpy().copy() if self._stats else None

    def reset(self, *, seed=None, options=None):
        obs, info = self.env.reset(seed=seed, options=options)
        return obs.cpu().numpy(), info

    def step(self, actions):
        actions = np.asarray(actions, dtype=self.single_action_space.dtype)   # (float32 with io_dtype=torch.float32)
        lo, hi = self.single_action_space.low, self.single_action_space.high
        if actions.shape != (self.num_envs, lo.shape[0]) or not ((actions >= lo) & (actions <= hi)).all():
            raise AssertionError("Action %r (%s) invalid." % (actions, type(actions)))  # anm_env.py:356-357
        obs, rew, term, trunc, info = self.env.step(torch.from_numpy(actions).to(self.env.device))
        if self._stats:
            env = self.env
            n_done = env.episodes_done.cpu().numpy()
            ended = n_done != self._n_done
            self._n_done = n_done.copy()
            info = dict(info)
            # "d": the discounted return (the return the reference's write-ups report); rows outside the mask are 0
            info["episode"] = {"r": np.where(ended, env.last_episode_return.cpu().numpy(), 0.0),
                               "l": np.where(ended, env.last_episode_length.cpu().numpy(), 0).astype(np.int32),
                               "d": np.where(ended, env.last_episode_discounted_return.cpu().numpy(), 0.0)}
            info["_episode"] = ended
        return (obs.cpu().numpy(), rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), info)

    def close(self):
        self.env.close()
