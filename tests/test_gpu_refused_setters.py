"""GPU tier: a refused ``anm_model_set_env`` or ``anm_model_set_obs`` leaves the model as it was.  Both setters check
first, upload into buffers of their own and touch the model last, so a call that returns non-zero changes nothing: the
task is not silently another one afterwards.  Each test steps a model that took refused calls next to an untouched twin
and requires the same bits.

The task for set_env is the one in which a half-applied call would show: the correlated series-noise mode (its mode,
amplitude table, AR(1) table and ``exo_z`` all live on the model) with an episode limit of 3, over 5 steps with
autoreset -- a truncation and an in-kernel reset are crossed."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib
from gym_anm_amd.envs.anm6 import ANM6EasyVec, ANM6Vec, anm6easy_series

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_ = 64


def easy(impl, **kw):
    env = ANM6EasyVec(num_envs=E_, device=DEV, seed=11, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def step_both(a_env, b_env, steps, names):
    gen = torch.Generator(device=DEV).manual_seed(5)
    for t in range(steps):
        a = uniform_actions(a_env, gen)
        oa, ob = a_env.step(a)[0], b_env.step(a)[0]
        assert torch.equal(oa, ob), ("obs", t)
        for k in names:
            assert torch.equal(getattr(a_env, k), getattr(b_env, k)), (k, t)


@pytest.mark.parametrize("impl", ["thread", "radial"])
def test_a_refused_set_env_leaves_the_model_as_it_was(impl):
    ser = anm6easy_series()
    kw = dict(exogenous="series_noise", exo_noise=0.25 * np.abs(ser), exo_corr=0.5, max_episode_steps=3, autoreset=True)
    env, twin = easy(impl, **kw), easy(impl, **kw)
    env.reset(options={"sampler": "device"})
    twin.reset(options={"sampler": "device"})
    assert torch.equal(env.state, twin.state) and torch.equal(env.exo_z, twin.exo_z)
    sim, lib = env.simulator, env.simulator.backend.lib
    n = env.exo_z.shape[1]
    slo, shi = env._cfg_keep
    half = _lib.EpisodeBuffers(ep_disc_return=env.e_loss.data_ptr())

    def cfg(cls=_lib.EnvConfigCorr, tail=None, **b):
        """the task of `env` but for what `b` names"""
        arr = dict(ser=ser, amp=env.exo_noise, lo=env.exo_low, hi=env.exo_high, rho=env.exo_corr, innov=env._exo_innov)
        arr = {k: np.ascontiguousarray(b.get(k, v), dtype=np.float64) for k, v in arr.items()}
        ptr = {k: v.ctypes.data_as(_lib.c_double_p) for k, v in arr.items()}
        c = cls(K=1, gamma=float(env.gamma), clip_e_loss=float(env.costs_clipping[0]), clip_penalty=float(env.costs_clipping[1]),
                obs_low=_lib.as_c(slo, np.float64)[1], obs_high=_lib.as_c(shi, np.float64)[1], series=ptr["ser"], period=ser.shape[1],
                exo_mode=_lib.EXO_SERIES_NOISE, exo_low=ptr["lo"], exo_high=ptr["hi"],
                max_episode_steps=b.get("limit", 3), episode=b.get("episode", C.pointer(env._episode_bufs)))
        if cls is not _lib.EnvConfigEpisode and not b.get("no_amp"):
            c.exo_noise = ptr["amp"]
        if cls is _lib.EnvConfigCorr:
            c.exo_rho, c.exo_innov, c.exo_z = ptr["rho"], ptr["innov"], env.exo_z.data_ptr()
        if tail is not None:
            C.c_int32.from_address(C.addressof(c) + _lib.EnvConfig.K.offset + 4).value = tail
        c._keep = arr
        return c

    def vec(v):
        x = np.full(n, 0.5)
        x[0] = v
        return x

    refused = [(dict(tail=7), b"unknown value of tail"),
               (dict(limit=-1), b"max_episode_steps must not be negative"),
               (dict(episode=C.pointer(half)), b"ep_disc_return and ep_discount go together"),
               (dict(cls=_lib.EnvConfigEpisode), b"needs the amplitude table"),
               (dict(amp=np.full(ser.shape, -1.0)), b"must be finite and >= 0"),
               (dict(lo=np.ones(n), hi=np.zeros(n)), b"exo_low <= exo_high"),
               (dict(rho=vec(1.0)), b"exo_rho must be finite and in [0, 1)")]
    for b, msg in refused:
        c = cfg(**b)
        assert lib.anm_model_set_env(sim._handle, C.byref(c)) != 0, b
        assert msg in lib.anm_last_error(), (b, lib.anm_last_error())
    step_both(env, twin, 5, ("reward", "state", "terminated", "truncated", "exo_z"))
    assert int(env._reset_count.max()) >= 2          # (the limit was crossed and the kernel reset those environments)
    assert float(env.exo_z.abs().max()) > 0.0        # (the chain ran: the noise states are not the cleared buffer)


def test_a_refused_set_obs_keeps_the_list():
    obs = [("bus_p", "all"), ("dev_q", "all"), ("des_soc", "all"), ("aux", "all")]

    def make():
        e = ANM6Vec(obs, 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, 95),)), costs_clipping=(1, 100), seed=11, num_envs=E_,
                    device=DEV, impl="thread", series=anm6easy_series(), autoreset=True)
        e.check_actions = False
        return e

    env, twin = make(), make()
    assert env._obs_fused and env.simulator.impl == "thread"
    env.reset(options={"sampler": "device"})
    twin.reset(options={"sampler": "device"})
    sim, lib = env.simulator, env.simulator.backend.lib
    bad = np.array([0, sim.full_dim + 1], dtype=np.int32)     # (K = 1: the one aux slot is full_dim)
    one, lo, hi = np.ones(2), -np.ones(2), np.ones(2)
    args = (_lib.as_c(bad, np.int32)[1], _lib.as_c(one, np.float64)[1], _lib.as_c(lo, np.float64)[1], _lib.as_c(hi, np.float64)[1])
    assert lib.anm_model_set_obs(sim._handle, 2, *args) != 0 and b"index out of range" in lib.anm_last_error()
    step_both(env, twin, 2, ("reward", "state", "terminated"))
    assert float(env._obs_buf.abs().max()) > 0.0
