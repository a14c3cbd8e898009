"""GPU tier: the I/O layers of the thread-per-environment family compute the same step.

The family has three step kernels around one solve -- k_step_rows (coalesced rows; the default), k_step_general (rows
staged in LDS; here through ``track_full=True``) and k_step_view (per-lane rows; here through an identity batch view) --
which share their action-row load, their hand-over to lane groups, their scalar stores and the init-state draws of the
autoreset.  ANM6Easy, 130 environments (two full wavefronts and a tail of two rows: the ``rows < 64`` clamp of the action
load and the partial-mask branch of the row stores), one seed, one ``env_offset``, a device reset and 24 steps of seeded
actions fed to all of them.  After the reset and after every step every output of the general and of the view layer
equals that of the row layer under ``torch.equal``; the float32 arms of the action load (k_step_rows_io32, and
k_step_general with a fused list observation that names the state's own entries) give the same float64 outputs and the
float64 observation and reward rounded once.  No output is left out of the comparison.  The run is checked not to be
vacuous: a hand-over happened, an environment terminated and was reset in the kernel, and a tail environment did both."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib
from gym_anm_amd.envs.anm6 import ANM6Vec, anm6easy_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ = 130
TAIL = (128, 129)
STEPS = 24
SEED = 2                       # (the first seed at which a tail environment collapses and is reset within the 24 steps)
ENV_OFFSET = (1 << 32) - 100   # the batch straddles 2^32: both words of the environment index are in the RNG key
HANDOFF = 6                    # Newton iterations in thread mode before a running solve moves to a lane group
OUTPUTS = ("state", "obs", "reward", "e_loss", "penalty", "terminated", "timestep", "soc", "nr_iters", "reset_count")
# the state's own entries as a list that is not the state list itself: gathered inside k_step_general
STATE_AS_LIST = [("dev_p", [0, 1, 2], "MW"), ("dev_p", [3, 4, 5, 6], "MW"), ("dev_q", "all", "MVAr"), ("des_soc", "all", "MWh"),
                 ("gen_p_max", "all", "MW"), ("aux", "all")]


def make_env(observation="state", view=False, **kw):
    """ANM6Easy (the constants of ANM6EasyVec), thread family, autoreset"""
    env = ANM6Vec(observation, 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 95]]), costs_clipping=(1, 100), seed=SEED,
                  num_envs=E_, device=DEV, series=anm6easy_series(), impl="thread", autoreset=True, env_offset=ENV_OFFSET, **kw)
    assert env.simulator.impl == "thread"
    env.check_actions = False
    if view:   # an identity view: every row where it was, moved per lane by k_step_view
        sim = env.simulator
        lib = sim.backend.lib
        assert lib.anm_model_bind_state_same(sim._handle, None) == 0
        env._state_same = None
        env._view_keep = _lib.BatchView(env_index=None)
        assert lib.anm_model_bind_view(sim._handle, C.byref(env._view_keep)) == 0
    return env


@functools.lru_cache(maxsize=None)
def actions():
    """[STEPS, E, 6] uniform over the action Box, every entry a float32 number: the float32 arms read the same values"""
    env = make_env(io_dtype=torch.float32)
    lo, hi = torch.as_tensor(env.action_space.low), torch.as_tensor(env.action_space.high)
    assert lo.dtype == torch.float32
    u = torch.rand((STEPS, E_, lo.numel()), generator=torch.Generator().manual_seed(SEED), dtype=torch.float64)
    a = torch.minimum(torch.maximum((lo.double() + (hi.double() - lo.double()) * u).float(), lo), hi)
    return a.to(DEV).contiguous()


def snapshot(env, obs):
    out = dict(state=env.state, obs=obs, reward=env.reward, e_loss=env.e_loss, penalty=env.penalty, terminated=env.terminated,
               timestep=env.timestep, soc=env.simulator.soc, nr_iters=env.simulator.nr_iters, reset_count=env._reset_count)
    return {k: v.clone() for k, v in out.items()}


def run(env):
    """the outputs after the device reset and after each of the 24 steps"""
    f32 = env.io_dtype == torch.float32
    obs, _ = env.reset(options={"sampler": "device"})
    snaps = [snapshot(env, obs)]
    for a in actions():
        obs, _, _, _, _ = env.step(a if f32 else a.double())
        snaps.append(snapshot(env, obs))
    return snaps


@functools.lru_cache(maxsize=None)
def rows_run():
    """(a) the default: k_step_rows.  Computed once; nobody writes to it"""
    return run(make_env())


def assert_same(snaps, where, f32=False):
    ref = rows_run()
    assert len(snaps) == len(ref) == STEPS + 1
    for t, (x, y) in enumerate(zip(snaps, ref)):
        for k in OUTPUTS:
            at = "%s, %s: %s" % (where, "reset" if t == 0 else "step %d" % (t - 1), k)
            if f32 and k in ("obs", "reward"):   # the float64 value rounded once, bit for bit
                assert x[k].dtype == torch.float32 and y[k].dtype == torch.float64 and x[k].shape == y[k].shape, at
                assert torch.equal(x[k].contiguous().view(torch.int32), y[k].float().contiguous().view(torch.int32)), at
            else:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and torch.equal(x[k], y[k]), at


def test_the_run_hands_over_and_resets_in_the_tail():
    ref = rows_run()
    iters = torch.stack([s["nr_iters"] for s in ref[1:]])            # [STEPS, E]
    handed = (iters > HANDOFF).any(dim=0)
    reset = ref[-1]["reset_count"] > ref[0]["reset_count"]           # terminated, and re-initialised by a later step
    term = torch.stack([s["terminated"] for s in ref[1:]]).any(dim=0)
    print("environments handed over: %d, terminated: %d, reset in the kernel: %d; tail: %s %s" %
          (int(handed.sum()), int(term.sum()), int(reset.sum()), handed[list(TAIL)].tolist(), reset[list(TAIL)].tolist()))
    assert bool(handed.any())
    assert bool((term & reset).any())
    assert bool((handed & term & reset)[list(TAIL)].any())


def test_general_layer_equals_row_layer():
    env = make_env(track_full=True)      # (b) the electrical-state dump: k_step_general
    assert env._need_full
    assert_same(run(env), "k_step_general")


def test_view_layer_equals_row_layer():
    assert_same(run(make_env(view=True)), "k_step_view")   # (c)


def test_float32_arms_equal_row_layer_rounded_once():
    assert_same(run(make_env(io_dtype=torch.float32)), "k_step_rows_io32", f32=True)
    env = make_env(STATE_AS_LIST, io_dtype=torch.float32, track_full=True)
    assert env._obs_fused and env.obs_values != env.state_values and env._need_full
    assert_same(run(env), "k_step_general, float32", f32=True)
