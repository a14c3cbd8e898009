"""Episode time limit, truncation flag and episode statistics: the specification the step kernels follow
(csrc/anm_env_ops.hpp: EpisodeIO, episode_timed_out / episode_clear / episode_step; the lane-group kernels call the same
three functions).  Like ``rng.py`` this text is normative: the kernels are tested against it bit for bit.

Let ``T = max_episode_steps`` (``T > 0``; ``None`` -- 0 in the C ABI -- means no limit) and ``t = timestep[e]`` on entry to
a step call.

1. Entry.  ``ended = terminated[e] or (T and t >= T)``: the time-limit half is derived from ``timestep``, never from the
   ``truncated`` buffer.  With autoreset an ended environment is re-initialised instead of stepped -- the autoreset path
   as it always was: the action is ignored, ``reward = e_loss = penalty = 0``, ``timestep = 0``, the initial state is
   drawn with epoch ``reset_count[e]``, which is then incremented; a draw whose first power flow does not converge leaves
   ``terminated = 1``, looks absorbing and is retried at the next call.  That call writes ``truncated[e] = 0``.  Without
   autoreset a terminated environment stays absorbing, and one that is only past the limit keeps being stepped, every
   output bit-identical to the same environment without a limit (Gymnasium's ``TimeLimit``).
2. Exit of a real step that leaves ``timestep = t' = t + 1``: ``truncated[e] = (t' >= T)`` whatever ``terminated`` is.
   The absorbing no-op step leaves ``truncated`` as it is.
3. Statistics.  Running values ``ret, disc_ret, discount``; a reset (in-kernel or ``reset()``, masked rows only) sets
   them to ``0, 0, 1``.  A real step with stored reward ``r`` does, in this order, ``ret = ret + r``;
   ``disc_ret = fma(discount, r, disc_ret)`` (ONE rounding: ``rng.fma``); ``discount = discount * gamma``.  The episode
   ends on the step where ``terminated_out or t' == T`` (``==``: an environment stepped on beyond the limit reports one
   episode, not one per step); then ``last_ret = ret``, ``last_disc_ret = disc_ret``, ``last_len = t'`` (this step
   included) and ``n_done += 1``.  The absorbing step, the reset-instead-of-step call and a failed reset draw end no
   episode.
"""

from __future__ import annotations

import operator

from . import errors as E
from .rng import fma


def check_limit(max_episode_steps):
    """``None`` (no limit) or a positive integer; anything else is an ``ArgsError``."""
    if max_episode_steps is None:
        return None
    try:
        if isinstance(max_episode_steps, bool):
            raise TypeError
        T = operator.index(max_episode_steps)
    except TypeError:
        raise E.ArgsError("The argument max_episode_steps is %r but should be None or a positive integer." % (max_episode_steps,)) from None
    if T <= 0 or T >= 2**31:
        raise E.ArgsError("The argument max_episode_steps is %r but should be None or a positive integer (below 2^31)." % (max_episode_steps,))
    return T


def ended_on_entry(terminated, timestep, T):
    """Rule 1: has the episode of this environment ended when a step call begins?"""
    return bool(terminated) or bool(T and timestep >= T)


class EpisodeTracker:
    """One environment's flags and statistics, driven by what the step calls did.

    A step call is one of three EVENTS, told apart by how it left ``timestep``:
    ``reset()`` -- the environment was re-initialised (an in-kernel autoreset, a failed draw included, or a host reset);
    ``step(r, terminated)`` -- a real step that stored reward ``r`` and the flag ``terminated``;
    ``noop()`` -- the step of an absorbing environment."""

    def __init__(self, gamma, max_episode_steps=None):
        self.gamma, self.T = float(gamma), check_limit(max_episode_steps)
        self.timestep = 0
        self.truncated = False
        self.ret, self.disc_ret, self.discount = 0.0, 0.0, 1.0
        self.last_ret, self.last_disc_ret, self.last_len, self.n_done = 0.0, 0.0, 0, 0

    def reset(self):
        self.timestep = 0
        self.truncated = False
        self.ret, self.disc_ret, self.discount = 0.0, 0.0, 1.0

    def noop(self):
        pass

    def step(self, r, terminated):
        """Returns True when this step ended the episode."""
        r = float(r)
        t1 = self.timestep + 1
        self.timestep = t1
        self.truncated = bool(self.T and t1 >= self.T)
        self.ret = self.ret + r
        self.disc_ret = fma(self.discount, r, self.disc_ret)
        self.discount = self.discount * self.gamma
        ended = bool(terminated) or (self.T is not None and t1 == self.T)
        if ended:
            self.last_ret, self.last_disc_ret, self.last_len = self.ret, self.disc_ret, t1
            self.n_done += 1
        return ended

    def call(self, terminated_in, autoreset, r, terminated_out, reset_converged=True):
        """One step call of the kernels on this environment, rule 1 included: what it does follows from the flags on entry.
        ``r`` / ``terminated_out``: what a real step would store; ``reset_converged``: whether the draw of a
        re-initialisation converges.  Returns ``(event, terminated after the call)``."""
        if ended_on_entry(terminated_in, self.timestep, self.T) and autoreset:
            self.reset()
            return "reset", not reset_converged
        if terminated_in:
            self.noop()
            return "noop", True
        self.step(r, terminated_out)
        return "step", bool(terminated_out)
