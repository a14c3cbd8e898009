"""Batched ``ANMEnv``: the Gymnasium surface of the reference over ``num_envs`` environments.

Mirrors ``gym_anm/envs/anm_env.py``: same constructor arguments (plus ``num_envs`` / ``device`` /
solver options), same hooks for task designers (``init_state``, ``next_vars``,
``observation_bounds``, ``observation``), same attributes (``K``, ``gamma``, ``lamb``,
``delta_t``, ``simulator``, ``state_values``, ``state_N``, ``action_space``, ``obs_values``,
``observation_space``, ``observation_N``, ``terminated``, ``timestep``, ``state``, ``e_loss``,
``penalty``, ``costs_clipping``, ``pfe_converged``) and the same ``reset`` / ``step`` contracts,
with a leading ``num_envs`` dimension on every per-environment quantity:

* ``reset(seed=, options=) -> (obs[num_envs, O], {})``
* ``step(action[num_envs, A]) -> (obs, reward[num_envs], terminated[num_envs], truncated[num_envs], {})``

``step`` is ONE launch of the fused HIP kernel (next_vars lookup in series mode, set-point
projection, Newton-Raphson power flow, branch flows, reward + clipping, state and observation);
nothing is copied to the host and nothing synchronises.  Non-convergence of the power flow is not
an error: it sets ``terminated`` (anm_env.py:421), the environment then stays in the absorbing
zero state with reward 0 (anm_env.py:365-367) until it is reset -- explicitly through
``reset(options={"mask": ...})``, or by itself at the next ``step`` when ``autoreset=True``
(series-mode tasks; Gymnasium's "next step" vector autoreset).

Every tensor is float64 unless ``io_dtype=torch.float32``: then the kernels read float32 actions and write float32
observations and rewards (the float64 values rounded once), the spaces are float32 ``Box``es and everything else stays
float64 (gym_anm_amd/io_dtype.py).  ``action_map=`` / ``obs_map=`` / ``reward_scale=`` put fixed affine maps on the same three
arrays, inside the kernels: unit actions in, scaled observations and rewards out (gym_anm_amd/io_affine.py).
"""

from __future__ import annotations

import ctypes as C
import gc
from copy import deepcopy

import numpy as np
import torch

from .. import _lib
from .. import episode as _episode
from .. import errors as E
from .. import io_affine as _aff
from .. import io_dtype as _io
from .. import io_norm as _nrm
from .. import rng as _rng
from ..model import STATE_VARIABLES
from ..simulator import BatchedSimulator, StateView, _stream_ptr
from ..spaces import Box, GymEnv


def check_env_args(K, delta_t, lamb, gamma, observation, aux_bounds, state_bounds):
    """Argument validation of ``gym_anm/envs/utils.py:7-122`` (same exceptions)."""
    if K < 0:
        raise E.ArgsError("The argument K is %d but should be >= 0." % (K))
    if delta_t <= 0:
        raise E.ArgsError("The argument delta_t is %.2f but should be > 0." % (delta_t))
    if lamb < 0:
        raise E.ArgsError("The argument lamb is %d but should be >= 0." % (lamb))
    if gamma < 0 or gamma > 1:
        raise E.ArgsError("The argument gamma is %.4f but should be in [0, 1]." % (gamma))
    if isinstance(observation, str) and observation == "state":
        pass
    elif isinstance(observation, list):
        for obs in observation:
            if len(obs) not in (2, 3):
                raise E.ObsSpaceError("The observation tuple {} should be a list with 2 or 3 elements.".format(obs))
            key, nodes = obs[0], obs[1]
            if key not in STATE_VARIABLES:
                raise E.ObsNotSupportedError(key, STATE_VARIABLES)
            if isinstance(nodes, str) and nodes == "all":
                pass
            elif key == "aux":
                for n in nodes:
                    if n >= K:
                        raise E.ObsSpaceError("Aux variable index {} is out of bound for {} aux variables.".format(n, K))
            elif isinstance(nodes, list):
                for n in nodes:
                    if n not in state_bounds[key]:
                        raise E.ObsSpaceError(
                            "Observation {} is not supported for device/branch/bus with ID {}.".format(key, n)
                        )
            else:
                raise E.ObsSpaceError()
            if len(obs) == 3 and obs[2] not in STATE_VARIABLES[key]:
                raise E.UnitsNotSupportedError(obs[2], STATE_VARIABLES[key], key)
    elif callable(observation):
        pass
    else:
        raise E.ArgsError(
            'The argument observation is of type {} but should be either a list, a callable, or the string "state".'.format(
                type(observation)
            )
        )
    if aux_bounds is not None and len(aux_bounds) != K:
        raise E.ArgsError(
            "The argument aux_bounds has length {} but the environment has K={} auxiliary variables.".format(
                len(aux_bounds), K
            )
        )


class BatchedANMEnv(GymEnv):
    def __init__(self, network, observation, K, delta_t, gamma, lamb, aux_bounds=None, costs_clipping=None, seed=None,
                 num_envs=1, device="cuda", tol=1e-5, max_iter=100, precision="f64", autoreset=False, series=None,
                 env_offset=0, impl=None, straggler_after="auto", straggler_mid="auto", handoff_after="auto", row_continuation=0, track_full=False,
                 fuse_observation=True, variants=None, env_variant=None, exogenous=None, exo_low=None, exo_high=None, exo_noise=None,
                 exo_corr=None, forecast_horizon=None,
                 max_episode_steps=None, episode_stats=False, io_dtype=None, action_map=None, obs_map=None, reward_scale=None,
                 obs_norm=None, reward_norm=None, norm_eps=_nrm.EPS_DEFAULT, _backend=None):  # fmt: skip
        GymEnv.reset(self, seed=seed)
        # a simulator sits in a reference cycle, so the device buffers of an environment that was dropped wait for the cycle
        # collector: collect here, where the next environment is about to allocate its own, not at some later step()
        gc.collect()
        # affine policy I/O inside the kernels (gym_anm_amd/io_affine.py has the semantics): checked before anything is built
        self._check_io_map_args(action_map, obs_map, reward_scale, observation, fuse_observation, track_full,
                                variants is not None or env_variant is not None, obs_norm, reward_norm, norm_eps)
        self.K, self.gamma, self.lamb, self.delta_t = K, gamma, lamb, delta_t
        self.aux_bounds = aux_bounds
        if costs_clipping is None:
            c1, c2 = np.inf, np.inf
        else:
            c1 = np.inf if costs_clipping[0] is None else costs_clipping[0]
            c2 = np.inf if costs_clipping[1] is None else costs_clipping[1]
        self.costs_clipping = (c1, c2)
        self.num_envs = int(num_envs)
        self.autoreset = bool(autoreset)
        self.env_offset = int(env_offset)  # global index of environment 0 (sharded batches)
        # float32 policy-facing I/O, produced and consumed by the kernels (gym_anm_amd/io_dtype.py has the semantics):
        # actions in, observations and rewards out as float32; everything else stays float64
        self.io_dtype = _io.check_io_dtype(io_dtype)
        self._io32 = self.io_dtype == torch.float32
        if self._io32 and (variants is not None or env_variant is not None):
            raise E.EnvInitializationError("io_dtype=torch.float32 does not take parameter classes (variants=)")

        self.simulator = BatchedSimulator(network, delta_t, lamb, num_envs=num_envs, device=device, tol=tol,
                                          max_iter=max_iter, precision=precision, impl=impl,
                                          handoff_after=handoff_after, row_continuation=row_continuation, variants=variants,
                                          env_variant=env_variant, _backend=_backend)  # fmt: skip
        sim = self.simulator
        self.device = sim.device
        check_env_args(K, delta_t, lamb, gamma, observation, aux_bounds, sim.state_bounds)
        # episode time limit and statistics, kept by the step kernels (gym_anm_amd/episode.py has the semantics)
        self.max_episode_steps = _episode.check_limit(max_episode_steps)
        self.episode_stats = bool(episode_stats)
        if (self.max_episode_steps or self.episode_stats) and sim.backend.device_type != "cuda":
            # (a backend that ignores the fields would run another task without saying so)
            raise E.EnvInitializationError("max_episode_steps / episode_stats need the GPU library: this backend keeps no "
                                           "episode time limit or statistics in its kernels")

        if self._io32 and sim.backend.device_type != "cuda":
            # (a backend that ignores the mode would read float32 actions as doubles without saying so)
            raise E.EnvInitializationError("io_dtype=torch.float32 needs the GPU library: this backend reads and writes "
                                           "float64 arrays alone")

        if self._mapped and sim.backend.device_type != "cuda":
            # (a backend that ignores the maps would step with the unit actions as MW without saying so)
            raise E.EnvInitializationError("action_map / obs_map / reward_scale / obs_norm / reward_norm need the GPU library: "
                                           "this backend maps nothing in its kernels")

        self.state_values = self._expand_all_ids(
            [("dev_p", "all", "MW"), ("dev_q", "all", "MVAr"), ("des_soc", "all", "MWh"), ("gen_p_max", "all", "MW"),
             ("aux", "all", None)]
        )  # fmt: skip
        self.state_N = sum(len(s[1]) for s in self.state_values)
        lo, hi = sim.model.action_bounds()
        if self._io32:  # bounds rounded inward: every float32 point of the Box lies in the reference's float64 Box
            lo, hi = _io.action_bounds32(lo, hi)
        self.action_space = Box(low=lo, high=hi, dtype=np.float32 if self._io32 else np.float64)
        self.raw_action_space = self.action_space   # MW / MVAr: what the kernels step with, whatever the policy sends
        if self._action_map_arg is not None:
            # the policy sends u in [-1, 1]; the kernels step with clamp(fma(half, u, mid)) inside the float64 Box
            lo64, hi64 = (np.asarray(x, dtype=np.float64) for x in sim.model.action_bounds())
            mid, half = _aff.unit_action_map(lo64, hi64) if isinstance(self._action_map_arg, str) else self._action_map_arg
            self._map_act = _aff.check_action_map(mid, half, lo64, hi64)
            lo, hi = -np.ones(len(lo64)), np.ones(len(lo64))
            self.action_space = Box(low=lo, high=hi, dtype=np.float32 if self._io32 else np.float64)
        self.single_action_space = self.action_space

        self.obs_values = self._build_observation_space(observation)
        self.observation_space = self.observation_bounds()
        # the float64 Box the kernels clip to; in float32 mode the space itself has its bounds rounded to nearest
        self._obs_space64 = self.observation_space
        if self.observation_space is not None:
            self.observation_N = self.observation_space.shape[0]
            if self._obs_map_arg is not None:   # the Box of images: the map is monotone (io_affine.py rule 5)
                lo64, hi64 = np.asarray(self._obs_space64.low, float), np.asarray(self._obs_space64.high, float)
                sc, bi = _aff.box_obs_map(lo64, hi64) if isinstance(self._obs_map_arg, str) else self._obs_map_arg
                self._map_obs = _aff.check_obs_map(sc, bi, self.observation_N)
                self.observation_space = Box(*_aff.observation_image(lo64, hi64, *self._map_obs), dtype=np.float64)
            if self._obs_norm:   # the tables move: no finite Box holds (io_norm.py); they start at those of the initial statistics
                self._map_obs = _nrm.tables(np.zeros(self.observation_N), np.ones(self.observation_N), self.norm_eps)
                inf = np.full(self.observation_N, np.inf)
                self.observation_space = Box(low=-inf, high=inf, dtype=np.float64)
            if self._io32:
                lo32, hi32 = _io.observation_bounds32(self.observation_space.low, self.observation_space.high)
                self.observation_space = Box(low=lo32, high=hi32, dtype=np.float32)
        self.single_observation_space = self.observation_space

        self._alloc_buffers()
        # key of the device-side sampler (reset(options={"sampler": "device"}), autoreset).  Unseeded environments draw
        # it from np_random (entropy-seeded in that case), so that two unseeded environments -- e.g. the ranks of a
        # sharded batch -- are not correlated; explicit seeds stay deterministic.
        self.rng_seed = int(self.np_random.integers(2**62)) if seed is None else int(seed)
        self._act_low = torch.as_tensor(lo, dtype=self.io_dtype, device=self.device)
        self._act_high = torch.as_tensor(hi, dtype=self.io_dtype, device=self.device)
        self.check_actions = True
        self._series = None if series is None else np.ascontiguousarray(series, dtype=np.float64)
        self._check_forecast(forecast_horizon, exogenous)
        self._check_exogenous(exogenous, exo_low, exo_high, exo_noise, exo_corr, variants is not None or env_variant is not None)
        self._alloc_forecast()
        self._obs_is_state = self.obs_values is not None and self.obs_values == self.state_values
        self._set_task()
        self._set_observation_gather(fuse_observation)
        self._set_io_map()
        self._plan_step_path(track_full, straggler_after, straggler_mid, max_iter)

    def _check_io_map_args(self, action_map, obs_map, reward_scale, observation, fuse_observation, track_full, has_classes,
                           obs_norm=None, reward_norm=None, norm_eps=_nrm.EPS_DEFAULT):
        """action_map=None | "unit" | (mid, half); obs_map=None | "box" | (scale, bias); reward_scale=None | a finite number
        > 0: fixed affine maps applied INSIDE the step and reset kernels (gym_anm_amd/io_affine.py).  The policy sends u, the
        kernels step with a = clamp(fma(half, u, mid)) inside the action Box ("unit": [-1, 1] onto the Box); they store
        fma(o, scale, bias) for every observation entry o ("box": every column with finite ends onto about [-1, 1]) and
        reward * reward_scale.  Everything else -- state, costs, episode statistics, exo_forecast (MW) -- stays raw.  With all
        three None nothing changes.  What the mode does not serve is refused here, by the name of the argument.

        obs_norm=None | "running", reward_norm=None | "running", norm_eps: the observation tables / the reward scale of the
        same map follow running statistics kept on the device -- mean and variance of the observations, variance of the
        discounted return -- rewritten after every step() by two small launches behind the step kernel
        (gym_anm_amd/io_norm.py).  obs_norm excludes obs_map, reward_norm excludes reward_scale, action_map is free."""
        self._obs_norm, self._reward_norm, self.norm_eps = _nrm.check_norm_args(obs_norm, reward_norm, norm_eps, obs_map, reward_scale)
        self._norm_on = self._obs_norm or self._reward_norm
        self.norm_training = True   # False: step() skips the update -- tables and statistics frozen (evaluation)
        for name, val, word in (("action_map", action_map, "unit"), ("obs_map", obs_map, "box")):
            if val is None or (isinstance(val, str) and val == word):
                continue
            if isinstance(val, str) or not isinstance(val, (tuple, list)) or len(val) != 2:
                raise E.ArgsError("The argument %s is %r but should be None, %r or a pair of vectors." % (name, val, word))
        self._action_map_arg = None if action_map is None else action_map if isinstance(action_map, str) else tuple(action_map)
        self._obs_map_arg = None if obs_map is None else obs_map if isinstance(obs_map, str) else tuple(obs_map)
        self.reward_scale = None if reward_scale is None else _aff.check_reward_scale(reward_scale)
        self._map_act = self._map_obs = None   # the resolved host tables: (mid, half, low, high), (scale, bias)
        self._mapped = action_map is not None or obs_map is not None or reward_scale is not None or self._norm_on
        if not self._mapped:
            return
        which = "/".join(n for n, v in (("action_map", action_map), ("obs_map", obs_map), ("reward_scale", reward_scale),
                                        ("obs_norm", obs_norm), ("reward_norm", reward_norm)) if v is not None)
        if has_classes:
            raise E.EnvInitializationError("%s does not take parameter classes (variants=)" % which)
        if callable(observation):
            raise E.EnvInitializationError("%s does not go with a callable observation: the kernels map what they write, and a "
                                           "callable observation is computed outside them" % which)
        if isinstance(observation, list) and not fuse_observation:
            raise E.EnvInitializationError("%s needs the list-form observation gathered inside the step kernel: "
                                           "fuse_observation=False leaves it to anm_gather_obs_f64, which maps nothing" % which)
        if track_full and not isinstance(observation, list):
            raise E.EnvInitializationError("%s takes track_full=True only next to a list-form observation gathered inside the "
                                           "step kernel" % which)

    @property
    def io_map(self):
        """The host tables of the affine I/O maps in use (float64 arrays; io_affine.py), or None without the mode: a dict with
        ``action`` = (mid, half, low, high) or None, ``obs`` = (scale, bias) or None, ``reward_scale`` (1.0 when not given)."""
        if not self._mapped:
            return None
        rs = 1.0 if self.reward_scale is None else self.reward_scale
        if self._reward_norm:   # (running: what the device holds now -- the read synchronises)
            rs = float(self._norm_stats[_nrm.STATS_HEAD - 4])
        return dict(action=self._map_act, obs=self._obs_tables_now(), reward_scale=rs)

    def _obs_tables_now(self):
        """(scale, bias) on the host, or None: the fixed tables, or -- obs_norm -- a copy of what the device holds now"""
        if not self._obs_norm:
            return self._map_obs
        D, H = self.observation_N, _nrm.STATS_HEAD
        t = self._norm_stats[H + 2 * D:H + 4 * D].cpu().numpy()
        return t[:D].copy(), t[D:].copy()

    def encode_action(self, a_mw):
        """The u to send for an action in MW / MVAr (an ``MPCAgent``'s): ``(a_mw - mid) / half``; the action itself without
        ``action_map``.  Not bit-exact under the kernels' decode (io_affine.encode_action)."""
        if self._map_act is None:
            return a_mw
        return _aff.encode_action(a_mw, self._map_act[0], self._map_act[1])

    def _set_io_map(self):
        """Hand the maps to the library (anm_model_set_io_map): after the task and the observation list, whose lengths its
        tables have."""
        if not self._mapped:
            return
        sim = self.simulator
        if self._gather is not None and not self._obs_fused:
            raise E.EnvInitializationError("action_map / obs_map / reward_scale need the list-form observation gathered inside "
                                           "the step kernel: this model cannot gather in its kernel")
        rs0 = _nrm.reward_scale(1.0, self.norm_eps) if self._reward_norm else self.reward_scale
        m = _lib.IoMap(reward_scale=1.0 if rs0 is None else rs0)
        keep = []
        for names, tabs in ((("act_mid", "act_half", "act_low", "act_high"), self._map_act), (("obs_scale", "obs_bias"), self._map_obs)):
            for name, tab in zip(names, tabs or ()):
                arr, ptr = _lib.as_c(tab, np.float64)
                keep.append(arr)
                setattr(m, name, ptr)
        with sim._device_ctx():
            sim.backend.check(sim.backend.lib.anm_model_set_io_map(sim._handle, C.byref(m)), "anm_model_set_io_map")
        if self._norm_on:
            self._norm_write_tables()

    def _alloc_buffers(self):
        """Device-resident per-environment state, and the episode buffers the step kernels keep."""
        E_, S = self.num_envs, self.state_N
        f64 = dict(dtype=torch.float64, device=self.device)
        fio = dict(dtype=self.io_dtype, device=self.device)   # what the policy sees: obs and reward
        self._state_buf = torch.zeros((E_, S), **f64)
        self._state_same = None  # uint8 [E]: 1 = the state row equals the obs row and was left unwritten (see `state`)
        self._state_obs = torch.zeros((E_, S), **fio)  # clip(state, state-space bounds), written by the kernel
        self.reward = torch.zeros(E_, **fio)
        self.e_loss = torch.zeros(E_, **f64)
        self.penalty = torch.zeros(E_, **f64)
        self._term_u8 = torch.zeros(E_, dtype=torch.uint8, device=self.device)
        self._term_bool = self._term_u8.view(torch.bool)  # zero-copy: the kernel only writes 0 / 1
        self.timestep = torch.zeros(E_, dtype=torch.int32, device=self.device)
        self._conv_u8 = torch.zeros(E_, dtype=torch.uint8, device=self.device)
        # convergence of the last power flow (see `pfe_converged`): a tensor from the start; after a step it is
        # `~terminated`, formed when somebody asks (step() itself launches nothing but the step kernel)
        self._conv_bool = torch.ones(E_, dtype=torch.bool, device=self.device)
        self._conv_stale = False
        self._reset_count = torch.zeros(E_, dtype=torch.int32, device=self.device)
        self._trunc_u8 = torch.zeros(E_, dtype=torch.uint8, device=self.device)
        self._truncated = self._trunc_u8.view(torch.bool)  # zero-copy: written by the kernels when a limit is set
        self._episode_bufs = None
        if self.episode_stats:
            i32 = dict(dtype=torch.int32, device=self.device)
            self.episode_return = torch.zeros(E_, **f64)
            self.episode_discounted_return = torch.zeros(E_, **f64)
            self._episode_discount = torch.ones(E_, **f64)
            self.last_episode_return = torch.zeros(E_, **f64)
            self.last_episode_discounted_return = torch.zeros(E_, **f64)
            self.last_episode_length = torch.zeros(E_, **i32)
            self.episodes_done = torch.zeros(E_, **i32)
        if self.max_episode_steps or self.episode_stats:
            b = _lib.EpisodeBuffers(truncated=self._trunc_u8.data_ptr())
            if self.episode_stats:
                b.ep_return, b.ep_disc_return = self.episode_return.data_ptr(), self.episode_discounted_return.data_ptr()
                b.ep_discount = self._episode_discount.data_ptr()
                b.last_return = self.last_episode_return.data_ptr()
                b.last_disc_return = self.last_episode_discounted_return.data_ptr()
                b.last_length, b.episodes_done = self.last_episode_length.data_ptr(), self.episodes_done.data_ptr()
            self._episode_bufs = b
        # running normalisation (gym_anm_amd/io_norm.py): statistics, counters, the slabs between the two launches of an
        # update, and per environment the discounted-return accumulator and the timestep last seen
        self._norm_ref = self._norm_args = None
        if self._norm_on:
            D, H = self.observation_N, _nrm.STATS_HEAD
            self._norm_stats = torch.zeros(H + 4 * D, **f64)
            self._norm_counters = torch.zeros(2, dtype=torch.int64, device=self.device)
            self._norm_slabs = torch.zeros(_nrm.slab_doubles(E_, D), **f64)
            self._norm_G = torch.zeros(E_, **f64)
            self._norm_t_seen = torch.zeros(E_, dtype=torch.int32, device=self.device)
            self._norm_struct = _lib.IoNorm(
                stats=self._norm_stats.data_ptr(), counters=self._norm_counters.data_ptr(), slabs=self._norm_slabs.data_ptr(),
                n_slab_doubles=self._norm_slabs.numel(), ret_acc=self._norm_G.data_ptr(), t_seen=self._norm_t_seen.data_ptr(),
                gamma=float(self.gamma), eps=self.norm_eps, obs_on=int(self._obs_norm), reward_on=int(self._reward_norm))
            self._norm_ref = C.byref(self._norm_struct)
            self._norm_fill(_nrm.initial_state(E_, D))

    # ---- running normalisation (gym_anm_amd/io_norm.py) -----------------------------------------------------------------------
    def _norm_fill(self, d):
        """The device buffers from a state dict of io_norm.py (host values); the mirrors of the tables by rule 1 -- a part
        that is off: the identity of io_affine.py rule 8 -- until anm_model_io_norm_tables rewrites them."""
        D, H = self.observation_N, _nrm.STATS_HEAD
        mean, var = np.asarray(d["mean"], dtype=np.float64), np.asarray(d["var"], dtype=np.float64)
        G, seen = np.asarray(d["G"], dtype=np.float64), np.asarray(d["t_seen"], dtype=np.int32)
        if mean.shape != (D,) or var.shape != (D,) or G.shape != (self.num_envs,) or seen.shape != (self.num_envs,):
            raise E.ArgsError("norm state: mean and var must have %d entries, G and t_seen %d" % (D, self.num_envs))
        scale, bias = _nrm.tables(mean, var, self.norm_eps) if self._obs_norm else (np.ones(D), np.full(D, -0.0))
        rs = _nrm.reward_scale(d["rvar"], self.norm_eps) if self._reward_norm else 1.0
        head = [float(d["cnt"]), float(d["rcnt"]), float(d["rmean"]), float(d["rvar"]), rs, 0.0, 0.0, 0.0]
        self._norm_stats.copy_(torch.as_tensor(np.concatenate([head, mean, var, scale, bias]), dtype=torch.float64))
        self._norm_counters.copy_(torch.as_tensor([int(d["n_updates"]), int(d["n_skipped"])], dtype=torch.int64))
        self._norm_G.copy_(torch.as_tensor(G))
        self._norm_t_seen.copy_(torch.as_tensor(seen))

    def _norm_write_tables(self):
        """Rule 1 on the device: the tables of the map from the statistics block (anm_model_io_norm_tables)."""
        sim = self.simulator
        with sim._device_ctx():
            sim.backend.check(sim.backend.lib.anm_model_io_norm_tables(sim._handle, self._norm_ref, _stream_ptr(self.device)),
                              "anm_model_io_norm_tables")

    def _norm_views(self, lo):
        from types import SimpleNamespace

        D, H, s = self.observation_N, _nrm.STATS_HEAD, self._norm_stats
        if lo == 0:
            return SimpleNamespace(count=s[0:1], mean=s[H:H + D], var=s[H + D:H + 2 * D], scale=s[H + 2 * D:H + 3 * D],
                                   bias=s[H + 3 * D:H + 4 * D])
        return SimpleNamespace(count=s[1:2], mean=s[2:3], var=s[3:4], scale=s[4:5])

    @property
    def obs_rms(self):
        """The running observation statistics ON THE DEVICE, to read (views: count [1], mean, var and the tables they give,
        scale and bias, [obs_dim] each; float64), or None without obs_norm.  To change them: load_norm_state()."""
        return self._norm_views(0) if self._obs_norm else None

    @property
    def ret_rms(self):
        """The running statistics of the discounted return on the device, to read (views: count, mean, var, and scale = the
        reward_scale of the map; [1] each), or None without reward_norm."""
        return self._norm_views(1) if self._reward_norm else None

    def norm_state(self):
        """Host copies of everything the running normalisation keeps (the dict of io_norm.py: cnt, mean, var, rcnt, rmean,
        rvar, G, t_seen, n_updates, n_skipped): a checkpoint.  Synchronises."""
        if not self._norm_on:
            raise E.ArgsError("norm_state() needs obs_norm or reward_norm")
        D, H = self.observation_N, _nrm.STATS_HEAD
        s, c = self._norm_stats.cpu().numpy(), self._norm_counters.cpu().numpy()
        return dict(cnt=float(s[0]), rcnt=float(s[1]), rmean=float(s[2]), rvar=float(s[3]), mean=s[H:H + D].copy(),
                    var=s[H + D:H + 2 * D].copy(), G=self._norm_G.cpu().numpy(), t_seen=self._norm_t_seen.cpu().numpy(),
                    n_updates=int(c[0]), n_skipped=int(c[1]))

    def load_norm_state(self, d):
        """Restore a norm_state() and rewrite the tables of the map on the device from it (rule 1)."""
        if not self._norm_on:
            raise E.ArgsError("load_norm_state() needs obs_norm or reward_norm")
        self._norm_fill(d)
        self._norm_write_tables()

    def _norm_update(self, stream=None, switch=None):
        """The update pair behind a step, on the same stream (`stream`, `switch`: what _step_call found for its own launch):
        reads what the step stored, rewrites the tables in place."""
        sim, dev = self.simulator, self.device
        args = self._norm_args
        if args is None:
            args = self._norm_args = (
                (self._obs_buf if self._obs_fused else self._state_obs).data_ptr(), self.reward.data_ptr(),
                self._term_u8.data_ptr(), self._trunc_u8.data_ptr(), self.timestep.data_ptr(), self._norm_ref)
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            switch = torch.cuda.current_device() != dev.index
        fn = sim.backend.lib.anm_model_io_norm_update
        if switch:
            with torch.cuda.device(dev):
                rc = fn(sim._handle, self.num_envs, *args, stream)
        else:
            rc = fn(sim._handle, self.num_envs, *args, stream)
        if rc != 0:
            sim.backend.check(rc, "anm_model_io_norm_update")

    def _check_exogenous(self, exogenous, exo_low, exo_high, exo_noise, exo_corr, has_classes):
        """The exogenous mode and its tables, checked and resolved; nothing is handed to the library here.

        exogenous="uniform": the loads and generator potentials of every step are drawn INSIDE the step kernels,
        P_i ~ U(exo_low[i], exo_high[i]) MW (units: loads by device id, then non-slack generators; defaults: loads
        [p_min, 0], generators [0, p_max]) from the counter-based RNG -- the stream layout is rng.py's (exo_uniform).
        K = 1: the aux variable is the step index of the episode.  step() is one launch and never calls next_vars().
        exogenous="series_noise": series mode plus bounded noise drawn INSIDE the step kernels, clipped to
        [exo_low, exo_high] -- P_i = clip(series[i, aux'] + exo_noise[i, aux'] (2 u_i - 1)) MW, keyed by the step index of
        the episode (rng.py: exo_series_noise).  K = 1: the aux variable is the table index, as in series mode.
        exo_corr=rho (series-noise mode; a scalar or [n_exo], every entry finite and in [0, 1)): the noise is an AR(1)
        chain instead of white -- every unit keeps a noise state z in `exo_z` ([num_envs, n_exo], float64, read-only for
        the caller), z' = fma(rho, z, sqrt(1 - rho^2) w), and z' takes the place of the factor w (rng.py:
        exo_series_corr).  None: the mode as it was, no buffer; 0.0: the new path, which then equals it bit for bit."""
        sim = self.simulator
        if exogenous not in (None, "host", "uniform", "series_noise"):
            raise E.ArgsError("The argument exogenous is %r but should be None, 'host', 'uniform' or 'series_noise'." % (exogenous,))
        self.exogenous = exogenous if exogenous in ("uniform", "series_noise") else "host"
        self._uniform = self.exogenous == "uniform"
        self._noisy = self.exogenous == "series_noise"
        self._drawn = self._uniform or self._noisy   # P_load / P_pot come from the kernels' RNG: next_vars() is never called
        sim.exogenous = self.exogenous   # (what an agent built from the simulator alone can know of the task: agents/mpc.py)
        self.exo_low = self.exo_high = self.exo_noise = self.exo_corr = self.exo_z = self._exo_innov = None
        n_exo = sim.N_load + sim.N_non_slack_gen
        if exo_noise is not None and not self._noisy:
            raise E.ArgsError("exo_noise needs exogenous='series_noise'")
        if exo_corr is not None:
            if not self._noisy:
                raise E.ArgsError("exo_corr needs exogenous='series_noise'")
            try:
                rho = np.ascontiguousarray(np.broadcast_to(np.asarray(exo_corr, dtype=np.float64), (n_exo,)))
            except ValueError:
                raise E.ArgsError("exo_corr must be a scalar or have %d entries (loads, then non-slack generators)" % n_exo) from None
            if not (np.isfinite(rho).all() and (rho >= 0).all() and (rho < 1).all()):
                raise E.ArgsError("exo_corr must be finite and in [0, 1)")
            self.exo_corr = rho
            # (formed here, once, and handed to the library beside rho: the kernels take no square root)
            self._exo_innov = np.ascontiguousarray(_rng.exo_innovation(rho))
        sim.exo_corr = self.exo_corr   # (tells the agents, like sim.exogenous above)
        if not self._drawn:
            if exo_low is not None or exo_high is not None:
                raise E.ArgsError("exo_low / exo_high need exogenous='uniform'")
            return
        mode = "exogenous='%s'" % self.exogenous
        if self._uniform and self._series is not None:
            raise E.EnvInitializationError("exogenous='uniform' and series= do not go together")
        if self._noisy and self._series is None:
            raise E.EnvInitializationError("exogenous='series_noise' needs series= (the table the noise is added to)")
        if self.K != 1:
            raise E.EnvInitializationError("%s needs K = 1 (the aux variable is the %s index)" % (mode, "step" if self._uniform else "table"))
        if has_classes:
            raise E.EnvInitializationError("%s does not take parameter classes (variants=)" % mode)
        if sim.backend.device_type != "cuda":
            # (a backend that ignores the mode would run a different task without saying so)
            raise E.EnvInitializationError("%s needs the GPU library: this backend does not draw in its kernels" % mode)
        if self._noisy:   # the amplitude table, broadcast to the shape of the series
            if self._series.ndim != 2 or self._series.shape[0] != n_exo:
                raise E.ArgsError("series must have %d rows (loads, then non-slack generators)" % n_exo)
            if exo_noise is None:
                raise E.ArgsError("exogenous='series_noise' needs exo_noise (a scalar, [n_exo] or [n_exo, period], MW)")
            amp = np.asarray(exo_noise, dtype=np.float64)
            if amp.ndim == 1:
                amp = amp[:, None]
            try:
                amp = np.ascontiguousarray(np.broadcast_to(amp, self._series.shape))
            except ValueError:
                raise E.ArgsError("exo_noise must be a scalar, [%d] or [%d, %d]" % (n_exo, n_exo, self._series.shape[1])) from None
            if not (np.isfinite(amp).all() and (amp >= 0).all()):
                raise E.ArgsError("exo_noise must be finite and >= 0")
            self.exo_noise = amp
        d_lo, d_hi = _rng.default_exo_bounds(sim.model)
        self.exo_low = d_lo if exo_low is None else np.ascontiguousarray(exo_low, dtype=np.float64)
        self.exo_high = d_hi if exo_high is None else np.ascontiguousarray(exo_high, dtype=np.float64)
        if self.exo_low.shape != (n_exo,) or self.exo_high.shape != (n_exo,):
            raise E.ArgsError("exo_low / exo_high must have %d entries (loads, then non-slack generators)" % n_exo)
        ordered = (self.exo_low <= self.exo_high).all()   # (NaN fails the comparison; series-noise: infinite ends mean "no clip")
        if self._uniform and not (ordered and np.isfinite(self.exo_low).all() and np.isfinite(self.exo_high).all()):
            raise E.ArgsError("exo_low / exo_high must be finite with exo_low <= exo_high")
        if not ordered:
            raise E.ArgsError("exo_low / exo_high must not be NaN, with exo_low <= exo_high")

    def _check_forecast(self, forecast_horizon, exogenous):
        """forecast_horizon=H (series-noise mode; an int in [1, 64], the planning horizons k_mpc accepts): the step and reset
        kernels write, wherever they write a state row, the EXPECTED loads and generator potentials of the next H steps into
        `exo_forecast` ([num_envs, n_exo, H] MW, io_dtype; units: loads by device id, then non-slack generators) -- the
        second input of a policy, beside the observation.  After every reset() and step(), for every environment,
        exo_forecast[e] == rng.exo_forecast_expected(H, exo_low, exo_high, aux=state[e, -1], z=exo_z[e], ...) bit for bit
        (float32 I/O: that double rounded once); undefined before the first reset.  None: no buffer, nothing changes."""
        self.forecast_horizon = self.exo_forecast = self.forecast_space = None
        if forecast_horizon is None:
            return
        if isinstance(forecast_horizon, bool) or not isinstance(forecast_horizon, (int, np.integer)):
            raise E.ArgsError("The argument forecast_horizon is %r but should be an int in [1, 64] or None." % (forecast_horizon,))
        if not 1 <= int(forecast_horizon) <= 64:
            raise E.ArgsError("The argument forecast_horizon is %d but should be in [1, 64]." % int(forecast_horizon))
        if exogenous != "series_noise":
            # (uniform mode: the forecast is a constant; series and host-hook mode: nothing is drawn in the kernels)
            raise E.ArgsError("forecast_horizon needs exogenous='series_noise'")
        if self.simulator.backend.device_type != "cuda":
            raise E.EnvInitializationError("forecast_horizon needs the GPU library: this backend writes no forecast in its kernels")
        self.forecast_horizon = int(forecast_horizon)

    def _alloc_forecast(self):
        """The rows the kernels write and their space, once the task's ends are resolved."""
        if self.forecast_horizon is None:
            return
        H, n_exo = self.forecast_horizon, len(self.exo_low)
        self.exo_forecast = torch.zeros((self.num_envs, n_exo, H), dtype=self.io_dtype, device=self.device)
        lo = np.ascontiguousarray(np.broadcast_to(self.exo_low[:, None], (n_exo, H)))
        hi = np.ascontiguousarray(np.broadcast_to(self.exo_high[:, None], (n_exo, H)))
        if self._io32:   # bounds rounded to nearest, like the observation's: the conversion is monotone
            lo, hi = _io.observation_bounds32(lo, hi)
        self.forecast_space = Box(low=lo, high=hi, dtype=np.float32 if self._io32 else np.float64)

    def _env_config(self):
        """The anm_env_config of the task: the struct that ends with the last field the task uses.  The arrays behind its
        pointers stay alive on self (`_cfg_keep`: the observation bounds; the exogenous tables; `exo_z`)."""
        slo, shi = self._state_bounds_vectors()
        if self._obs_is_state and self.observation_space is not None:
            slo, shi = np.asarray(self._obs_space64.low, float), np.asarray(self._obs_space64.high, float)
        self._cfg_keep = (slo, shi)
        kw = dict(K=self.K, gamma=float(self.gamma), clip_e_loss=float(self.costs_clipping[0]), clip_penalty=float(self.costs_clipping[1]),
                  obs_low=_lib.as_c(slo, np.float64)[1], obs_high=_lib.as_c(shi, np.float64)[1],
                  exo_mode=_lib.EXO_UNIFORM if self._uniform else _lib.EXO_SERIES_NOISE if self._noisy else _lib.EXO_HOST)  # fmt: skip
        if self._series is not None:
            kw.update(series=self._series.ctypes.data_as(_lib.c_double_p), period=int(self._series.shape[1]))
        if self._drawn:
            kw.update(exo_low=self.exo_low.ctypes.data_as(_lib.c_double_p), exo_high=self.exo_high.ctypes.data_as(_lib.c_double_p))
        struct = _lib.EnvConfig
        if self._episode_bufs is not None:
            struct = _lib.EnvConfigEpisode
            kw.update(max_episode_steps=self.max_episode_steps or 0, episode=C.pointer(self._episode_bufs))
        if self._noisy:
            struct = _lib.EnvConfigNoise
            kw.update(exo_noise=self.exo_noise.ctypes.data_as(_lib.c_double_p))
        if self.exo_corr is not None:
            struct = _lib.EnvConfigCorr
            self.exo_z = torch.zeros((self.num_envs, len(self.exo_corr)), dtype=torch.float64, device=self.device)
            kw.update(exo_rho=self.exo_corr.ctypes.data_as(_lib.c_double_p),
                      exo_innov=self._exo_innov.ctypes.data_as(_lib.c_double_p), exo_z=self.exo_z.data_ptr())
        if self.forecast_horizon is not None:   # (without exo_corr the correlation trio before it stays null)
            struct = _lib.EnvConfigForecast
            kw.update(forecast_horizon=self.forecast_horizon, exo_forecast=self.exo_forecast.data_ptr())
        return struct(**kw)

    def _set_task(self):
        """Hand the task to the library: anm_model_set_env, the I/O mode, the observation bounds of every class."""
        sim = self.simulator
        cfg = self._env_config()
        with sim._device_ctx():
            sim.backend.check(sim.backend.lib.anm_model_set_env(sim._handle, C.byref(cfg)), "anm_model_set_env")
            if self._io32:
                sim.backend.check(sim.backend.lib.anm_model_set_io(sim._handle, _lib.IO_F32), "anm_model_set_io")
        # parameter classes: the reference builds one environment per network, each clipping its observation to the
        # Box of ITS network (anm_env.py:193-233, 313-331).  For the "state" observation every class gets its own
        # bounds; `class_observation_bounds` has them ([n_classes, state_N] each).  (observation_space itself, one
        # Box for the batch, stays that of class 0; list-form observations keep one Box.)
        self.class_observation_bounds = None
        vms = getattr(sim, "variant_models", [sim.model])
        if len(vms) > 1 and self._obs_is_state and type(self).observation_bounds is BatchedANMEnv.observation_bounds:
            los, his = [self._cfg_keep[0]], [self._cfg_keep[1]]
            with sim._device_ctx():
                for k, vm in enumerate(vms[1:], start=1):
                    lo_k, hi_k = self._state_bounds_vectors(vm.state_bounds())
                    (a_lo, p_lo), (a_hi, p_hi) = (_lib.as_c(x, np.float64) for x in (lo_k, hi_k))
                    sim.backend.check(sim.backend.lib.anm_model_set_class_obs_bounds(sim._handle, k, p_lo, p_hi),
                                      "anm_model_set_class_obs_bounds")
                    los.append(lo_k)
                    his.append(hi_k)
            self.class_observation_bounds = (np.stack(los), np.stack(his))

    def _set_observation_gather(self, fuse_observation):
        """List-form observations (anm_env.py:497-521): gathered, scaled and clipped inside the step kernel when
        the library can (anm_model_set_obs), else by anm_gather_obs_f64 from the electrical-state dump."""
        sim = self.simulator
        self._gather = None  # (index, scale, low, high) device tensors
        self._obs_fused = False
        self._obs_buf = None
        self._obs_gather64 = None   # float32 mode: where reset() gathers a list-form observation before the one cast
        if self.obs_values is None or self._obs_is_state:
            return
        self._gather = self._build_gather(self.obs_values)
        lib = sim.backend.lib
        if fuse_observation and lib.anm_model_obs_fusable(sim._handle):
            idx, sc, lo_, hi_ = (t.cpu().numpy() for t in self._gather)
            a_i, p_i = _lib.as_c(idx, np.int32)
            (a_s, p_s), (a_l, p_l), (a_h, p_h) = (_lib.as_c(x, np.float64) for x in (sc, lo_, hi_))
            with sim._device_ctx():
                sim.backend.check(lib.anm_model_set_obs(sim._handle, len(a_i), p_i, p_s, p_l, p_h), "anm_model_set_obs")
            self._obs_fused = True
            self._obs_buf = torch.zeros((self.num_envs, len(a_i)), dtype=self.io_dtype, device=self.device)
        if self._io32 and not self._obs_fused:
            raise E.EnvInitializationError(
                "io_dtype=torch.float32 needs the list-form observation gathered inside the step kernel: "
                + ("fuse_observation=False" if not fuse_observation else "this model cannot gather in its kernel")
                + " leaves it to anm_gather_obs_f64, which writes float64 observations")

    def _plan_step_path(self, track_full, straggler_after, straggler_mid, max_iter):
        """What a step launches: the electrical-state dump, the compact time index of the fast path, the rows it
        leaves unwritten (state_same) and the workspace of the two-launch step."""
        sim = self.simulator
        # track_full: also dump the electrical state of every step, so that simulator.state /
        # simulator.pfe_converged follow the environment like the reference's (simulator.py:529-537)
        self.track_full = bool(track_full)
        if self._mapped and self.track_full and not self._obs_fused:
            raise E.EnvInitializationError("action_map / obs_map / reward_scale take track_full=True only next to a list-form "
                                           "observation gathered inside the step kernel")
        if self._io32 and self.track_full and not self._obs_fused:
            raise E.EnvInitializationError("io_dtype=torch.float32 takes track_full=True only next to a list-form observation "
                                           "gathered inside the step kernel")
        self._need_full_reset = self._gather is not None or self.track_full
        self._need_full = (self._gather is not None and not self._obs_fused) or self.track_full
        self._after_step = False
        self._step_args = None
        self._reset_count_ptr = self._reset_count.data_ptr()
        # compact time index next to `state` (series mode, thread-per-environment family): enables the
        # coalesced-row step kernel
        self._aux_index = None
        # (series-noise mode: the general step kernel serves it; no compact index, no state_same, no two-launch workspace)
        if self._series is not None and self.K == 1 and sim.impl == "thread" and not self._noisy:
            self._aux_index = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self._aux_index_ptr = None if self._aux_index is None else self._aux_index.data_ptr()
        # "state" observation on the fast path: obs = clip(state) is the state itself unless a bound bites, so
        # the kernel writes the state row only then and flags the rest (anm_model_bind_state_same)
        # (float32 mode: the state row has no float64 twin in obs and is always written; the affine I/O map: likewise)
        if self._aux_index is not None and self._obs_is_state and sim.backend.device_type == "cuda" and not self._io32 \
                and not self._mapped:
            self._state_same = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            with sim._device_ctx():
                sim.backend.check(sim.backend.lib.anm_model_bind_state_same(sim._handle, self._state_same.data_ptr()),
                                  "anm_model_bind_state_same")
        # two-phase step (see anm_step_ws in include/anm_mi355x.h): the first launch stops after
        # `straggler_after` Newton iterations, a second launch continues the solves still running
        self._ws = self._ws_ref = None
        if straggler_after == "auto":
            # measured on MI355X (scripts/handoff_sweep.py, profiles/r02_d_handoff_sweep.txt): at 65 536
            # environments the in-wave lane-group hand-over (anm_solver_opts.handoff_after) is the faster cure for
            # stragglers (92 vs 114 us); the two-launch step -- stragglers of the whole batch packed into a second
            # launch, 8 per wavefront on lane groups -- wins once the batch is a multiple of the 65 536 lanes of the
            # chip (reference cap: 131 072: 121 vs 138 us, 262 144: 146 vs 183 us, 524 288: 193 vs 287 us, 1 M: 318
            # vs 484 us; with a cap of 20 the in-wave hand-over wins or ties up to 524 288, 1 M: 230 vs 239 us)
            big = 131072 if int(max_iter) >= 50 else 1048576
            straggler_after = 6 if self.num_envs >= big else None
        rec = sim.backend.lib.anm_step_ws_record_doubles()
        if self._aux_index is not None and straggler_after and rec > 0 and int(straggler_after) < int(max_iter):
            # records for 1/16 of the batch (~1.5 % of the solves are still running after 6 iterations; a solve
            # that finds no record continues on a lane group of its own wavefront)
            n_rec = min(self.num_envs, max(4096, self.num_envs // 16))
            self._ws_buf = torch.zeros(8 + n_rec * rec + (n_rec + 1) // 2, dtype=torch.float64, device=self.device)
            # straggler_mid: where the first straggler launch leaves the solves still running to a second one (None:
            # one level).  Measured (profiles/r03_f_throughput.txt): the straggler launch is bound by the 94-trip
            # chain of a diverging solve up to 524 288 environments -- a second level only adds a launch there (132 /
            # 158 / 206 us against 121 / 146 / 194) -- and by instruction issue at 1 M, where repacking the long
            # runners 8 per wavefront pays (298 against 318 us): "auto" = two levels from 1 M environments on
            if straggler_mid == "auto":
                straggler_mid = 12 if self.num_envs >= 1000000 else None
            mid = -1 if straggler_mid is None else int(straggler_mid)
            self._ws = _lib.StepWs(self._ws_buf.data_ptr(), self._ws_buf.numel(), int(straggler_after), mid)
            self._ws_ref = C.byref(self._ws)
        self._opts_ref = C.byref(sim.opts)

    # ---- hooks for task designers (anm_env.py:158-191) -----------------------------------------------
    def init_state(self):
        """Sample initial states: return a ``[num_envs, state_N]`` array/tensor (reference layout)."""
        raise NotImplementedError

    def next_vars(self, s_t):
        """Return ``[num_envs, N_load + N_gen + K]``: load injections (MW), generator potentials (MW)
        and the next auxiliary variables, given the state batch ``s_t``.  Not used in series mode."""
        raise NotImplementedError

    def observation_bounds(self):  # anm_env.py:193-233
        if self.obs_values is None:
            return None
        lower, upper = self._bounds_vectors(self.obs_values, self.simulator.state_bounds)
        return Box(low=lower, high=upper, dtype=np.float64)

    # ---- spaces helpers (anm_env.py:497-549) ------------------------------------------------------------
    def _build_observation_space(self, observation):
        if isinstance(observation, str) and observation == "state":
            obs_values = deepcopy(self.state_values)
        elif isinstance(observation, list):
            obs_values = deepcopy(observation)
            for idx, o in enumerate(obs_values):
                if len(o) == 2:
                    obs_values[idx] = tuple(list(o) + [STATE_VARIABLES[o[0]][0]])
        elif callable(observation):
            obs_values = None
            self.observation = observation  # shadows the method below, like the reference (anm_env.py:511-514)
            self.observation_fn = observation
        else:
            raise E.ObsSpaceError()
        return self._expand_all_ids(obs_values)

    def _expand_all_ids(self, values):
        m = self.simulator.model
        if values is None:
            return None
        for idx, o in enumerate(values):
            if isinstance(o[1], str) and o[1] == "all":
                if "bus" in o[0]:
                    ids = list(m.bus_ids)
                elif "dev" in o[0]:
                    ids = list(m.dev_ids)
                elif "des" in o[0]:
                    ids = [m.dev_ids[k] for k in m.des_idx]
                elif "gen" in o[0]:
                    ids = [m.dev_ids[k] for k in m.gen_idx]
                elif "branch" in o[0]:
                    ids = list(m.branch_ids)
                elif o[0] == "aux":
                    ids = list(range(0, self.K))
                else:
                    raise E.ObsNotSupportedError(o[0], STATE_VARIABLES.keys())
                values[idx] = (o[0], ids, o[2])
        return values

    def _state_bounds_vectors(self, bounds=None):
        """Box bounds of the *state* vector, used when the observation is the state (``bounds``: the state bounds of
        another network of the same topology: a parameter class)."""
        return self._bounds_vectors(self.state_values, self.simulator.state_bounds if bounds is None else bounds)

    def _bounds_vectors(self, values, bounds):
        """(low, high) of the variables `values` names: `bounds` for the electrical ones, aux_bounds (else none) for aux."""
        lo, hi = [], []
        for key, nodes, unit in values:
            for n in nodes:
                if key == "aux":
                    if self.aux_bounds is not None:
                        lo.append(self.aux_bounds[n][0])
                        hi.append(self.aux_bounds[n][1])
                    else:
                        lo.append(-np.inf)
                        hi.append(np.inf)
                else:
                    lo.append(bounds[key][n][unit][0])
                    hi.append(bounds[key][n][unit][1])
        return np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)

    def _build_gather(self, values):
        """Index/scale/clip vectors that turn the kernel's full-state dump (+ aux) into the
        list-form observation (anm_env.py:562-592 with the units of simulator.py:559-616)."""
        sim, m = self.simulator, self.simulator.model
        index, scale = [], []
        for key, nodes, unit in values:
            for n in nodes:
                if key == "aux":
                    index.append(sim.full_dim + n)  # aux columns are appended to the dump
                    scale.append(1.0)
                    continue
                if key.startswith("bus"):
                    j = m.bus_ids.index(n)
                elif key.startswith("dev"):
                    j = m.dev_ids.index(n)
                elif key == "des_soc":
                    j = [m.dev_ids[k] for k in m.des_idx].index(n)
                elif key == "gen_p_max":
                    j = [m.dev_ids[k] for k in m.gen_idx].index(n)
                else:
                    j = m.branch_ids.index(tuple(n))
                index.append(sim.full_offsets[key] + j)
                kv_j = j
                if key.startswith("branch"):  # kA for branches is not defined by the reference (pu only)
                    kv_j = 0
                scale.append(sim.unit_scale(key, unit, kv_j))
        space = self._obs_space64
        dev = self.device
        return (
            torch.as_tensor(index, dtype=torch.int32, device=dev),
            torch.as_tensor(scale, dtype=torch.float64, device=dev),
            torch.as_tensor(np.asarray(space.low, float), dtype=torch.float64, device=dev),   # (the float64 Box)
            torch.as_tensor(np.asarray(space.high, float), dtype=torch.float64, device=dev),
        )

    # ---- observation ---------------------------------------------------------------------------------------
    def observation(self, s_t):
        """``o_t = observation(s_t)``: clip(state variables, Box) (anm_env.py:313-331), batched.

        With ``obs_map`` and a list-form observation (``reset()`` only; ``step()`` gets the mapped list from its kernel) the
        gathered rows of ALL environments go to the host, through ``io_affine.map_obs`` and back: the call synchronises and
        copies ``num_envs x n_obs`` doubles each way, masked resets included.  A training loop that resets often should use
        ``autoreset=True``, whose rows the step kernel maps itself."""
        if self._obs_is_state:
            return self._state_obs
        sim = self.simulator
        index, scale, low, high = self._gather
        n_obs = index.numel()
        if self._obs_buf is None:
            self._obs_buf = torch.zeros((self.num_envs, n_obs), dtype=torch.float64, device=self.device)
        out = self._obs_buf
        remap = self._map_obs is not None   # (reset() only: gathered raw, mapped on the host -- io_affine.py rule 6)
        tables = self._obs_tables_now() if remap else None   # (obs_norm: the tables the device holds now)
        if self._io32 or remap:   # (reset() only: gathered in float64, cast once -- io_dtype.py rule 5)
            if self._obs_gather64 is None:
                self._obs_gather64 = torch.zeros((self.num_envs, n_obs), dtype=torch.float64, device=self.device)
            out = self._obs_gather64
        with sim._device_ctx():
            rc = sim.backend.lib.anm_gather_obs_f64(
                self.num_envs, sim.full.shape[1], sim.full.data_ptr(), self._state_buf.shape[1], self.K,
                self._state_buf.data_ptr(), self._term_u8.data_ptr(), n_obs, index.data_ptr(), scale.data_ptr(),
                low.data_ptr(), high.data_ptr(), out.data_ptr(), _stream_ptr(self.device),
            )  # fmt: skip
        sim.backend.check(rc, "anm_gather_obs_f64")
        if remap:   # exactly the kernels' fma, evaluated on the host (rng.fma_v): reset() is not the hot path
            out = torch.as_tensor(_aff.map_obs(out.cpu().numpy(), *tables), dtype=torch.float64, device=self.device)
        if out is not self._obs_buf:
            self._obs_buf.copy_(out)
        return self._obs_buf

    @property
    def state(self):
        """State vectors ``[num_envs, state_N]`` (anm_env.py:139-147).  On the fast path this is assembled on
        access: rows the kernel did not write because they equal the observation are taken from it."""
        if self._state_same is None:
            return self._state_buf
        return torch.where(self._state_same.view(torch.bool).unsqueeze(1), self._state_obs, self._state_buf)

    @property
    def terminated(self):
        return self._term_bool

    @property
    def truncated(self):
        """``timestep >= max_episode_steps`` as the last step (or reset) left it; all False without a limit."""
        return self._truncated

    @property
    def episode_length(self):
        """Steps of the running episode (``timestep``)."""
        return self.timestep

    @property
    def pfe_converged(self):
        """Convergence of the last power flow of every environment (simulator.pfe_converged in the
        reference): that of the reset right after a reset; after a step an environment has converged iff
        it is not terminated (anm_env.py:421).  Formed on access: `step()` only marks it stale."""
        if self._conv_stale:
            self._conv_bool = ~self._term_bool
            self._conv_stale = False
        return self._conv_bool

    # ---- reset (anm_env.py:235-311) --------------------------------------------------------------------------
    def _launch_reset(self, init_state, mask_u8):
        sim = self.simulator
        with sim._device_ctx():
            rc = sim.backend.lib.anm_reset_f64(
                sim._handle, self.num_envs, None if init_state is None else init_state.data_ptr(),
                None if mask_u8 is None else mask_u8.data_ptr(), self.rng_seed, self.env_offset, self._reset_count_ptr,
                sim.soc.data_ptr(), self._state_buf.data_ptr(), self._state_obs.data_ptr(), self._conv_u8.data_ptr(),
                self._term_u8.data_ptr(), self.timestep.data_ptr(), sim.nr_iters.data_ptr(),
                sim.full.data_ptr() if (self._need_full_reset or self._need_full) else None, self._aux_index_ptr,
                C.byref(sim.opts), _stream_ptr(self.device),
            )  # fmt: skip
        sim.backend.check(rc, "anm_reset_f64")
        if self._reward_norm:   # io_norm.py rule 2: the return accumulator of a re-initialised row starts over
            if mask_u8 is None:
                self._norm_G.zero_()
                self._norm_t_seen.zero_()
            else:
                self._norm_G.masked_fill_(mask_u8.ne(0), 0.0)
                self._norm_t_seen.masked_fill_(mask_u8.ne(0), 0)
        if self._state_same is not None:  # the reset kernel writes both rows
            if mask_u8 is None:
                self._state_same.zero_()
            else:
                self._state_same.mul_(1 - mask_u8)
        self._after_step = False
        # convergence per environment: the environments this reset touched report the reset's power flow, the others
        # keep what their last step left (not terminated <=> converged, anm_env.py:421)
        conv = torch.ne(self._conv_u8, 0)
        if mask_u8 is None:
            self._conv_bool = conv
        else:
            self._conv_bool = torch.where(mask_u8.ne(0), conv, self.pfe_converged)
        self._conv_stale = False
        if self._need_full_reset or self._need_full:
            sim.state = StateView(sim, sim.full)
            sim.pfe_converged = self._conv_bool

    def reset(self, *, seed=None, options=None):
        """Reset every environment (or those selected by ``options["mask"]``).

        ``options["init_state"]`` (``[num_envs, state_N]``) bypasses ``init_state()``; otherwise
        initial states are drawn with ``init_state()`` and redrawn (up to 100 times, like the
        reference) for the environments whose first power flow does not converge.
        """
        GymEnv.reset(self, seed=seed)
        if seed is not None:
            self.rng_seed = int(seed)
        options = options or {}
        # (uniform mode: plain reset() draws on the device unless the task brings an init_state() of its own; series-noise
        # mode: always -- a host init_state() of the task, ANM6EasyVec's for one, knows nothing of the noise)
        if options.get("sampler") == "device" or (options.get("init_state") is None and (
                self._noisy or (self._uniform and type(self).init_state is BatchedANMEnv.init_state))):
            return self._reset_on_device(options.get("mask"))
        mask = options.get("mask")
        mask_u8 = None
        if mask is not None:
            mask_u8 = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        given = options.get("init_state")
        todo = mask_u8.clone() if mask_u8 is not None else torch.ones(self.num_envs, dtype=torch.uint8,
                                                                     device=self.device)  # fmt: skip
        n_max = 100
        for attempt in range(1, n_max + 1):
            s0 = given if given is not None else self.init_state()
            s0 = torch.as_tensor(s0, dtype=torch.float64, device=self.device)
            if s0.dim() == 1:
                s0 = s0.unsqueeze(0).expand(self.num_envs, -1)
            if s0.shape[1] != self.state_N:
                raise E.EnvInitializationError(
                    "Expected size of initial state s0 is %d but actual is %d" % (self.state_N, s0.shape[1])
                )
            self._launch_reset(s0.contiguous(), todo)
            if self._drawn:
                # a new episode for every environment this reset touched, whoever supplied the rows: one environment
                # never uses a step stream twice (the epoch is part of its key)
                self._reset_count += todo.to(torch.int32)
            todo = todo * (1 - self._conv_u8)
            if given is not None or not bool(todo.any()):
                break
            if attempt == n_max:
                raise E.EnvInitializationError(
                    "No non-terminal state found out of %d initial states for environment %s"
                    % (n_max, type(self).__name__)
                )
        if given is not None:
            # an explicit initial state that does not converge leaves that environment terminated
            sel = todo.ne(0)
            self._term_u8[sel] = 1
        touched = mask_u8.ne(0) if mask_u8 is not None else slice(None)
        self.e_loss[touched] = 0.0
        self.penalty[touched] = 0.0
        obs = self.observation(self.state)
        if self.observation_space is None:
            n = obs.shape[1]
            self.observation_space = Box(low=-np.ones(n) * np.inf, high=np.ones(n) * np.inf)
            self.observation_N = n
        return obs, {}

    def _reset_on_device(self, mask=None):
        """``reset(options={"sampler": "device"})`` (series-mode tasks): initial states are drawn inside
        the reset kernel by the counter-based RNG that also serves autoreset, keyed by
        ``(seed, env_offset + env, reset_count[env])``, instead of by ``init_state()`` on the host.
        Environments whose first power flow does not converge are redrawn, up to the reference's
        limit of 100 attempts (anm_env.py:266-289)."""
        if self._series is None and not self._uniform:
            raise E.EnvInitializationError("the device sampler needs a series-mode task")
        if mask is None:
            todo = torch.ones(self.num_envs, dtype=torch.uint8, device=self.device)
        else:
            todo = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        touched = todo.ne(0)
        for attempt in range(100):
            self._launch_reset(None, todo)
            todo = todo * (1 - self._conv_u8)
            if not bool(todo.any()):
                break
        else:
            raise E.EnvInitializationError(
                "No non-terminal state found out of 100 initial states for environment %s" % type(self).__name__
            )
        self.e_loss[touched] = 0.0
        self.penalty[touched] = 0.0
        return self.observation(self.state), {}

    def sample_init_state(self, raw=False):
        """The initial states ``reset(options={"sampler": "device"})`` / the autoreset would draw NOW for every
        environment -- ``ANM6Easy.init_state`` (anm6_easy.py:25-52) generalised to the series-mode task, keyed by
        ``(seed, env_offset + env, reset_count[env])`` -- without resetting anything: ``[num_envs, state_N]`` in the
        layout ``reset(options={"init_state": ...})`` takes.  ``raw=True``: also the Philox words behind each row
        (``int64 [num_envs, blocks, 4]`` holding uint32 values; anm_sample_init_state_f64)."""
        if self._series is None and not self._uniform:
            raise E.EnvInitializationError("the device sampler needs a series-mode task")
        sim = self.simulator
        out = torch.zeros((self.num_envs, self.state_N), dtype=torch.float64, device=self.device)
        words = None
        if raw:
            n_blocks = 1 + (sim.N_non_slack_gen + sim.N_des + 1) // 2
            words = torch.zeros((self.num_envs, n_blocks, 4), dtype=torch.int32, device=self.device)
        with sim._device_ctx():
            rc = sim.backend.lib.anm_sample_init_state_f64(
                sim._handle, self.num_envs, self.rng_seed, self.env_offset, self._reset_count_ptr, out.data_ptr(),
                None if words is None else words.data_ptr(), _stream_ptr(self.device))
        sim.backend.check(rc, "anm_sample_init_state_f64")
        if raw:
            return out, words.to(torch.int64) & 0xFFFFFFFF
        return out

    # ---- step (anm_env.py:333-453) -----------------------------------------------------------------------------
    def _step_call(self, action_ptr, exo_ptr, aux_ptr):
        """One anm_step_f64 launch on torch's current stream (all buffer pointers are persistent)."""
        sim = self.simulator
        dev = self.device
        if dev.type == "cuda":
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            switch = torch.cuda.current_device() != dev.index
        else:
            stream, switch = None, False
        args = self._step_args
        if args is None:
            args = self._step_args = (
                sim.soc.data_ptr(), self._state_buf.data_ptr(), self._term_u8.data_ptr(), self.timestep.data_ptr(),
                (self._obs_buf if self._obs_fused else self._state_obs).data_ptr(), self.reward.data_ptr(),
                self.e_loss.data_ptr(), self.penalty.data_ptr(), sim.nr_iters.data_ptr(),
                sim.full.data_ptr() if self._need_full else None,
            )  # fmt: skip
        fn = sim.backend.lib.anm_step_f64
        if switch:
            with torch.cuda.device(dev):
                rc = fn(sim._handle, self.num_envs, action_ptr, exo_ptr, aux_ptr, *args, 1 if self.autoreset else 0,
                        self.rng_seed, self.env_offset, self._reset_count_ptr, self._aux_index_ptr, self._ws_ref, self._opts_ref,
                        stream)  # fmt: skip
        else:
            rc = fn(sim._handle, self.num_envs, action_ptr, exo_ptr, aux_ptr, *args, 1 if self.autoreset else 0,
                    self.rng_seed, self.env_offset, self._reset_count_ptr, self._aux_index_ptr, self._ws_ref, self._opts_ref,
                        stream)  # fmt: skip
        if rc != 0:
            sim.backend.check(rc, "anm_step_f64")
        if self._norm_on and self.norm_training:   # two small launches behind the step: the tables the NEXT step maps with
            self._norm_update(stream, switch)

    def step(self, action):
        sim = self.simulator
        # (float32 mode: a float32, contiguous, on-device tensor goes to the kernel as it is -- no copy, no second launch)
        if not (isinstance(action, torch.Tensor) and action.dtype == self.io_dtype and action.device == self.device):
            action = torch.as_tensor(action, dtype=self.io_dtype, device=self.device)
        if action.dim() == 1:
            action = action.unsqueeze(0)
        if action.shape != (self.num_envs, sim.dims.action_dim):
            raise AssertionError("Action %r (%s) invalid." % (tuple(action.shape), type(action)))
        if self.check_actions:  # anm_env.py:356-357 (one device reduction + sync; disable for throughput runs)
            ok = bool(((action >= self._act_low) & (action <= self._act_high)).all())
            assert ok, "Action %r (%s) invalid." % (action, type(action))
        if not action.is_contiguous():
            action = action.contiguous()
        exo_ptr = aux_ptr = None
        if self._series is None and not self._uniform:
            v = torch.as_tensor(self.next_vars(self.state), dtype=torch.float64, device=self.device)
            expected = sim.N_load + sim.N_non_slack_gen + self.K
            if v.dim() != 2 or v.shape[1] != expected:
                raise E.EnvNextVarsError(
                    "Next vars vector has size %d but expected is %d" % (v.shape[-1] if v.dim() else 0, expected)
                )
            n_exo = sim.N_load + sim.N_non_slack_gen
            exo = v[:, :n_exo].contiguous()
            aux = v[:, n_exo:].contiguous()
            exo_ptr, aux_ptr = exo.data_ptr(), (aux.data_ptr() if self.K > 0 else None)
        self._step_call(action.data_ptr(), exo_ptr, aux_ptr)
        self._after_step = True
        self._conv_stale = True  # pfe_converged = ~terminated, formed on access (no launch, no allocation here)
        if self._need_full:
            sim.state = StateView(sim, sim.full)
            sim.pfe_converged = self.pfe_converged
        if self._obs_is_state:
            obs = self._state_obs
        elif self._obs_fused:
            obs = self._obs_buf  # written by the step kernel itself
        elif self.obs_values is None:
            obs = self.observation_fn(self.state)
            obs = torch.where(self._term_bool.unsqueeze(1), torch.zeros_like(obs), obs)  # anm_env.py:365-367, 442-446
        else:
            obs = self.observation(self.state)  # the gather kernel zeroes the rows of terminated environments
        return obs, self.reward, self._term_bool, self._truncated, {}

    def render(self, mode="human"):
        raise NotImplementedError()

    def close(self):
        pass
