"""GPU tier: correlated noise for the noisy time series (``BatchedANMEnv(exogenous="series_noise", exo_corr=rho)``) -- every
load and non-slack generator keeps a noise state z in ``exo_z``, an AR(1) chain advanced inside the step kernels
(specification: gym_anm_amd/rng.py, exo_series_corr).  After tests/test_gpu_exo_noise.py, whose task tables these tests use:
  1. the mode equals the host-hook path fed with the specification's draws, bit for bit, exo_z included;
  2. zero correlation equals the uncorrelated mode, bit for bit, autoreset, time limit and statistics included;
  3. replay by the specification across in-kernel resets; 4. reset() from rows, masked reset(), the absorbing step;
  5. float32 I/O; 6. shards; 7. HIP graph, no allocation; 8. what the mode refuses.
Batches: 229 = 3 * 64 + 37 environments for the thread-per-environment family (a partial last block: the lanes beyond the
batch work on a clamped index and must not touch exo_z), 41 for the lane-group families (a partial last wavefront of lane
groups), and 1, 63, 65 / 1, 9 once."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.envs.anm6 import ANM6EasyVec
from gym_anm_amd.envs.anm_env import BatchedANMEnv

from parity_common import uniform_actions
from test_gpu_exo_noise import CASES, DEV, INF, STATS, make_env, task_of

pytestmark = pytest.mark.gpu


def batch_of(impl):
    return 229 if impl == "thread" else 41


def rho_of(net):
    """(0.9, 0.5, 0, ...): a strongly and a mildly correlated unit, the others run the new path with rho = 0"""
    rho = np.zeros(task_of(net)[0].shape[0])
    rho[:2] = 0.9, 0.5
    return rho


def global_envs(env):
    return np.uint64(env.env_offset) + np.arange(env.num_envs, dtype=np.uint64)


def init_z(env, epoch):
    return rng.series_corr_init_z_v(env.rng_seed, global_envs(env), np.asarray(epoch).astype(np.uint64), env.exo_z.shape[1])


def mapped(z, aux, task):
    """the mode's map of noise states z [E, n_exo] at table indices aux [E], exactly (rng.fma_v)"""
    ser, amp, low, high = task
    out = np.empty(z.shape)
    for i in range(z.shape[1]):
        x = rng.fma_v(amp[i][aux], z[:, i], ser[i][aux])
        out[:, i] = np.where(x < low[i], low[i], np.where(x > high[i], high[i], x))
    return out


def exo_columns(model):
    """state columns of the loads' P and of the generators' P_max (what the draws become when nothing else touches them)"""
    D, nd = model.N_device, model.N_des
    return list(model.load_idx) + [2 * D + nd + g for g in range(model.N_non_slack_gen)]


def outputs(env, obs=None):
    out = [("state", env.state), ("reward", env.reward), ("e_loss", env.e_loss), ("penalty", env.penalty), ("terminated", env.terminated),
           ("truncated", env.truncated), ("soc", env.simulator.soc), ("timestep", env.timestep), ("reset_count", env._reset_count),
           ("nr_iters", env.simulator.nr_iters)]
    return out + ([] if obs is None else [("obs", obs)])


# ---- 1. the mode equals the hook path fed with the specification ---------------------------------------------------------
class HookTask(BatchedANMEnv):
    """the same task through next_vars(): the specification's chain, kept on the host.  An environment that is terminated
    (no autoreset here) is not stepped: its z stays, as its timestep does."""

    def next_vars(self, s_t):
        ser, amp, low, high = self.spec_task
        aux1 = np.fmod(s_t[:, -1].cpu().numpy() + 1.0, float(ser.shape[1])).astype(np.int64)
        t1 = (self.timestep.cpu().numpy().astype(np.int64) + 1).astype(np.uint64)
        P, z1 = rng.exo_series_corr_v(self.rng_seed, global_envs(self), self.spec_epoch, t1, aux1, self.spec_z, ser, amp,
                                      self.spec_rho, rng.exo_innovation(self.spec_rho), low, high)
        self.spec_z = np.where(self.terminated.cpu().numpy()[:, None], self.spec_z, z1)
        return torch.as_tensor(np.concatenate((P, aux1[:, None].astype(np.float64)), axis=1), device=self.device)


HOOK_CASES = [(n, i, batch_of(i)) for n, i in CASES] + [("anm6", "thread", e) for e in (1, 63, 65)] + \
             [("anm6", i, e) for i in ("radial", "mesh") for e in (1, 9)]


@pytest.mark.parametrize("net,impl,E_", HOOK_CASES)
def test_the_mode_equals_the_hook_path_bit_for_bit(net, impl, E_):
    T, SEED, OFF = 20, 4242, (1 << 32) - 20                     # (the global index crosses 2^32 inside the larger batches)
    rho = rho_of(net)
    cor = make_env(net, impl, E_, SEED, env_offset=OFF, exo_corr=rho)
    hook = make_env(net, impl, E_, SEED, cls=HookTask, mode="hook", env_offset=OFF)
    assert cor.exo_z.shape == (E_, len(rho)) and cor.exo_z.dtype == torch.float64 and (cor.exo_corr == rho).all()
    assert cor.simulator.exo_corr is cor.exo_corr
    z_buf = cor.exo_z.data_ptr()
    rows = cor.sample_init_state()
    cor.reset(options={"init_state": rows})
    hook.reset(options={"init_state": rows})
    hook.spec_task, hook.spec_rho = task_of(net), rho
    hook.spec_epoch = (cor._reset_count - 1).cpu().numpy().astype(np.uint64)
    assert not hook.spec_epoch.any()
    hook.spec_z = init_z(cor, hook.spec_epoch)
    assert np.array_equal(cor.exo_z.cpu().numpy(), hook.spec_z)      # a reset from rows stores w(step 0) of its epoch
    assert torch.equal(cor.state, hook.state)
    gen = torch.Generator(device=DEV).manual_seed(7)
    n_alive, z_max = 0, 0.0
    for t in range(T):
        a = uniform_actions(cor, gen)
        oc, oh = cor.step(a)[0], hook.step(a)[0]
        for (name, x), (_, y) in zip(outputs(cor, oc), outputs(hook, oh)):
            if name not in ("reset_count", "truncated"):
                assert torch.equal(x, y), "step %d: %s differs (%s, %s, %d)" % (t, name, net, impl, E_)
        got = cor.exo_z.cpu().numpy()
        assert got.tobytes() == hook.spec_z.tobytes(), "step %d: exo_z (%s, %s, %d): %d rows differ" % (
            t, net, impl, E_, int((got != hook.spec_z).any(axis=1).sum()))
        n_alive += int((~cor.terminated).sum())
        z_max = max(z_max, float(np.abs(got[:, 0]).max()))
    assert cor.exo_z.data_ptr() == z_buf and n_alive > E_ * T // 4
    assert z_max > 1.0 or E_ < 41      # (rho = 0.9: the chain leaves [-1, 1] -- it is not the factor -- and stays bounded)
    assert z_max <= rng.exo_innovation(0.9)[0] / (1 - 0.9) + 1


# ---- 2. zero correlation is the uncorrelated mode ----------------------------------------------------------------------------
def run_pair(a, b, T, seed):
    oa, ob = a.reset()[0], b.reset()[0]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for t in range(T + 1):
        if t:
            act = uniform_actions(a, gen)
            oa, ob = a.step(act)[0], b.step(act)[0]
        for (name, x), (_, y) in zip(outputs(a, oa) + [(k, getattr(a, k)) for k in STATS], outputs(b, ob) + [(k, getattr(b, k)) for k in STATS]):
            assert torch.equal(x, y), "step %d: %s differs" % (t, name)


@pytest.mark.parametrize("net,impl", CASES)
def test_zero_correlation_equals_the_uncorrelated_mode_bit_for_bit(net, impl):
    kw = dict(autoreset=True, max_episode_steps=5, episode_stats=True)
    a = make_env(net, impl, batch_of(impl), 31, **kw)
    b = make_env(net, impl, batch_of(impl), 31, exo_corr=0.0, **kw)
    assert a.exo_corr is None and a.exo_z is None and (b.exo_corr == 0).all()
    run_pair(a, b, 30, 5)
    assert int(a.episodes_done.min()) >= 4      # (the limit of 5 re-initialises everybody every six calls)
    # rho = 0: z is the factor of the last draw itself
    z = b.exo_z.cpu().numpy()
    want = rng.exo_factors_v(b.rng_seed, global_envs(b), (b._reset_count - 1).cpu().numpy().astype(np.uint64),
                             b.timestep.cpu().numpy().astype(np.uint64), z.shape[1])
    assert z.tobytes() == want.tobytes()


# ---- 3. replay across in-kernel resets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_replay_by_the_specification_across_in_kernel_resets(net, impl):
    """Every call of every environment is replayed from what the call before left: (state row, timestep, reset count, exo_z
    row) and the recorded reset counts.  exo_z, timestep and reset_count are compared exactly.  The loads' P and the
    generators' P_max columns of the state row hold the draw after a division and a multiplication by baseMVA (or a
    multiplication by its rounded reciprocal): at most 1.5 ulp, held to 2^-51 relative."""
    E_, T, SEED = batch_of(impl), 30, 8 if (net, impl) == ("anm6", "thread") else 3
    ser, amp, low, high = task = task_of(net)
    period, rho = ser.shape[1], rho_of(net)
    c = rng.exo_innovation(rho)
    env = make_env(net, impl, E_, SEED, exo_corr=rho, autoreset=True, max_episode_steps=5, episode_stats=True, env_offset=1000)
    cols = exo_columns(env.simulator.model)
    envs = global_envs(env)
    env.reset()
    assert np.array_equal(env.exo_z.cpu().numpy(), init_z(env, (env._reset_count - 1).cpu().numpy()))
    gen = torch.Generator(device=DEV).manual_seed(5)
    snap = lambda: tuple(x.cpu().numpy().copy() for x in (env.state, env.timestep, env._reset_count, env.exo_z, env.terminated))  # noqa: E731
    n_reset = n_step = n_collapse = n_failed_draw = 0
    for t in range(T):
        s0, ts0, rc0, z0, term0 = snap()
        env.step(uniform_actions(env, gen))
        s1, ts1, rc1, z1, term1 = snap()
        reset = term0 | (ts0 >= 5)
        assert np.array_equal(rc1, rc0 + reset) and np.array_equal(ts1, np.where(reset, 0, ts0 + 1)), t
        # a re-initialised environment: z = w(step 0) of the epoch the draw was made with, the row is the uncorrelated mode's
        zi = init_z(env, rc0)
        aux_r = (rng.philox4x32_v(np.uint64(SEED), envs, rc0.astype(np.uint64), np.uint64(0))[..., 0] * np.uint64(period)) >> np.uint64(32)
        aux_r = aux_r.astype(np.int64)
        Pi = mapped(zi, aux_r, task)
        # a stepped one: the chain advanced from the z the call found
        aux_s = np.fmod(s0[:, -1] + 1.0, float(period)).astype(np.int64)
        Ps, zs = rng.exo_series_corr_v(SEED, envs, (rc0 - 1).astype(np.uint64), (ts0 + 1).astype(np.uint64), aux_s, z0, ser, amp, rho, c, low, high)
        want_z = np.where(reset[:, None], zi, zs)
        assert z1.tobytes() == want_z.tobytes(), "call %d: exo_z, %d rows differ" % (t, int((z1 != want_z).any(axis=1).sum()))
        ok = ~term1                                          # (a collapsed step or a failed draw leaves a zero row)
        assert not s1[term1].any()
        want_P, want_aux = np.where(reset[:, None], Pi, Ps), np.where(reset, aux_r, aux_s)
        assert np.array_equal(s1[ok, -1], want_aux[ok].astype(np.float64)), t
        err = np.abs(s1[ok][:, cols] - want_P[ok])
        assert (err <= 2.0**-51 * np.abs(want_P[ok])).all(), (t, float(err.max()))
        n_reset += int(reset.sum())
        n_step += int((~reset).sum())
        n_collapse += int((term1 & ~reset).sum())
        n_failed_draw += int((term1 & reset).sum())
    print("%s %s: %d steps, %d resets, %d collapses away from the limit, %d failed draws" % (net, impl, n_step, n_reset, n_collapse, n_failed_draw))
    assert n_reset >= 4 * E_ and n_step >= 20 * E_
    if (net, impl) == ("anm6", "thread"):
        assert n_collapse >= 1        # a reset that the time limit did not cause (the seed is chosen for it)


# ---- 4. reset() from rows, masked reset(), the absorbing step --------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_resets_store_the_initial_z_and_the_absorbing_step_stores_nothing(net, impl):
    E_ = batch_of(impl)
    env = make_env(net, impl, E_, 17, exo_corr=rho_of(net), env_offset=(1 << 32) - 7)
    z = lambda: env.exo_z.cpu().numpy().copy()  # noqa: E731
    epoch = lambda: (env._reset_count - 1).cpu().numpy()  # noqa: E731
    gen = torch.Generator(device=DEV).manual_seed(11)
    env.reset()
    assert np.array_equal(z(), init_z(env, epoch()))
    for _ in range(3):
        env.step(uniform_actions(env, gen))
    z0, rc0 = z(), env._reset_count.clone()
    assert (z0 != init_z(env, epoch())).any(axis=1).all()
    # masked reset(): the device sampler for every third environment
    mask = torch.arange(E_, device=DEV) % 3 == 1
    m = mask.cpu().numpy()
    env.reset(options={"mask": mask})
    z1 = z()
    assert bool((env._reset_count[mask] > rc0[mask]).all()) and torch.equal(env._reset_count[~mask], rc0[~mask])
    assert np.array_equal(z1[m], init_z(env, epoch())[m]) and z1[~m].tobytes() == z0[~m].tobytes()
    assert (z1[m] != z0[m]).any(axis=1).all()
    # reset() from rows the caller brings, masked: the rows are kept, z is the initial z of the new epoch
    rows = env.sample_init_state()
    rows[:, -1] = torch.remainder(rows[:, -1] + 2, task_of(net)[0].shape[1])        # (rows of the caller's own: another table index)
    mask2 = torch.arange(E_, device=DEV) % 4 == 0
    m2 = mask2.cpu().numpy()
    rc1 = env._reset_count.clone()
    env.reset(options={"init_state": rows, "mask": mask2})
    z2 = z()
    assert torch.equal(env._reset_count, rc1 + mask2.to(torch.int32))
    assert np.array_equal(z2[m2], rng.series_corr_init_z_v(env.rng_seed, global_envs(env)[m2], rc1.cpu().numpy()[m2].astype(np.uint64), z2.shape[1]))
    assert z2[~m2].tobytes() == z1[~m2].tobytes() and torch.equal(env.state[mask2][:, -1], rows[mask2][:, -1])
    # ... and without a mask
    env.reset(options={"init_state": rows})
    assert np.array_equal(z(), init_z(env, epoch())) and torch.equal(env._reset_count, rc1 + mask2.to(torch.int32) + 1)
    # the absorbing step: rows forced terminal, no autoreset -- nothing of them is touched, exo_z included
    env.step(uniform_actions(env, gen))
    dead = torch.arange(E_, device=DEV) % 5 == 2
    d = dead.cpu().numpy()
    env._term_u8[dead] = 1
    z3, ts3 = z(), env.timestep.clone()
    env.step(uniform_actions(env, gen))
    z4 = z()
    assert z4[d].tobytes() == z3[d].tobytes() and torch.equal(env.timestep[dead], ts3[dead])
    alive = ~d & ~env.terminated.cpu().numpy()
    assert alive.any() and (z4[alive] != z3[alive]).any(axis=1).all()


# ---- 5. ... 7. composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_float32_io_is_the_float64_run_rounded_once(net, impl):
    kw = dict(autoreset=True, max_episode_steps=7, exo_corr=rho_of(net))
    a = make_env(net, impl, batch_of(impl), 8, **kw)
    b = make_env(net, impl, batch_of(impl), 8, io_dtype=torch.float32, **kw)
    oa, ob = a.reset()[0], b.reset()[0]
    gen = torch.Generator(device=DEV).manual_seed(2)
    for t in range(13):
        if t:
            act32 = uniform_actions(a, gen).float()
            oa, ob = a.step(act32.double())[0], b.step(act32)[0]
        assert ob.dtype == torch.float32 and b.reward.dtype == torch.float32 and b.exo_z.dtype == torch.float64
        assert torch.equal(ob, oa.float()) and torch.equal(b.reward, a.reward.float()), t
        for (name, x), (_, y) in zip(outputs(a) + [("exo_z", a.exo_z)], outputs(b) + [("exo_z", b.exo_z)]):
            if name != "reward":
                assert torch.equal(x, y), "step %d: %s" % (t, name)


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_two_shards_equal_the_whole_batch(impl):
    E_ = batch_of(impl)
    H0 = E_ // 2 - 3
    kw = dict(autoreset=True, max_episode_steps=4, exo_corr=rho_of("anm6"))
    whole = make_env("anm6", impl, E_, 77, **kw)
    shards = [make_env("anm6", impl, n, 77, env_offset=off, **kw) for off, n in ((0, H0), (H0, E_ - H0))]
    ow = whole.reset(seed=77)[0]
    os_ = [s.reset(seed=77)[0] for s in shards]
    gen = torch.Generator(device=DEV).manual_seed(3)
    for t in range(11):
        if t:
            a = uniform_actions(whole, gen)
            ow = whole.step(a)[0]
            os_ = [s.step(a[lo_:hi_].contiguous())[0] for s, (lo_, hi_) in zip(shards, ((0, H0), (H0, E_)))]
        parts = [outputs(s, o) + [("exo_z", s.exo_z)] for s, o in zip(shards, os_)]
        for k, (name, x) in enumerate(outputs(whole, ow) + [("exo_z", whole.exo_z)]):
            assert torch.equal(x, torch.cat([p[k][1] for p in parts])), "step %d: %s" % (t, name)
    assert int(whole._reset_count.min()) >= 3


@pytest.mark.parametrize("net,impl", CASES)
def test_a_captured_step_replays_what_eager_steps_compute_and_allocates_nothing(net, impl):
    kw = dict(autoreset=True, exo_corr=rho_of(net))
    eager, graphed = make_env(net, impl, batch_of(impl), 21, **kw), make_env(net, impl, batch_of(impl), 21, **kw)
    eager.reset()
    graphed.reset()
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = [uniform_actions(eager, gen) for _ in range(12)]
    a_buf = acts[0].clone()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):       # the FIRST step after reset() is the captured one
            obs_g = graphed.step(a_buf)[0]
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    assert not bool(graphed.timestep.any()) and torch.equal(eager.exo_z, graphed.exo_z)      # (capturing ran nothing)
    before = None
    for t, act in enumerate(acts):
        a_buf.copy_(act)
        g.replay()
        obs_e = eager.step(act)[0]
        torch.cuda.synchronize()
        if t == 1:
            before = torch.cuda.memory_allocated(DEV)
        for (name, x), (_, y) in zip(outputs(eager, obs_e) + [("exo_z", eager.exo_z)], outputs(graphed, obs_g) + [("exo_z", graphed.exo_z)]):
            assert torch.equal(x, y), "replay %d: %s" % (t, name)
    assert torch.cuda.memory_allocated(DEV) == before
    assert bool((eager.timestep == 12).any())


def test_anm6easyvec_takes_the_keyword_through():
    env = ANM6EasyVec(num_envs=41, device=DEV, seed=3, tol=1e-6, exogenous="series_noise", exo_noise=0.5, exo_corr=0.8, autoreset=True)
    twin = make_env("anm6", env.simulator.impl, 41, 3, noise=0.5, ends=rng.default_exo_bounds(env.simulator.model), autoreset=True,
                    exo_corr=np.full(5, 0.8))
    env.check_actions = False
    assert env.exo_corr.shape == (5,) and (env.exo_corr == 0.8).all() and env.exo_z.shape == (41, 5)
    env.reset()
    twin.reset()
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    env.step(a)
    twin.step(a)
    assert torch.equal(env.state, twin.state) and torch.equal(env.exo_z, twin.exo_z) and bool((env.exo_z != 0).all())


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_what_the_mode_refuses():
    from gym_anm_amd.agents import MPCAgentConstant, MPCAgentPerfect, MPCAgentPerfectStream
    from gym_anm_amd.envs.mixed import MixedBatchedANMEnv

    ser, amp, low, high = task_of("anm6")
    n = ser.shape[0]
    rho = rho_of("anm6")
    env = make_env("anm6", "radial", 41, 1, exo_corr=rho)
    env.reset()
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    sim = env.simulator
    lib = sim.backend.lib
    # everything the uncorrelated mode refuses in a step and where views and classes are bound
    exo = torch.zeros((41, n), dtype=torch.float64, device=DEV)
    aux = torch.zeros((41, 1), dtype=torch.float64, device=DEV)
    with pytest.raises(errors.HipExtensionError, match="exo and aux_next must be NULL"):
        env._step_call(a.data_ptr(), exo.data_ptr(), aux.data_ptr())
    env._step_call(a.data_ptr(), None, None)
    args = list(env._step_args)
    args[3] = None
    env._step_args = tuple(args)
    with pytest.raises(errors.HipExtensionError, match="timestep"):
        env._step_call(a.data_ptr(), None, None)
    env._step_args = None
    keep_rc, env._reset_count_ptr = env._reset_count_ptr, None
    with pytest.raises(errors.HipExtensionError, match="reset_count"):
        env._step_call(a.data_ptr(), None, None)
    with pytest.raises(errors.HipExtensionError, match="correlated noise needs reset_count"):      # a reset from rows needs the epoch
        env._launch_reset(env.state.clone(), None)
    env._reset_count_ptr = keep_rc
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(sim._handle, C.byref(view)) != 0 and b"series-noise" in lib.anm_last_error()
    cls = torch.zeros(41, dtype=torch.int32, device=DEV)
    assert lib.anm_model_bind_env_classes(sim._handle, cls.data_ptr(), 41) != 0 and b"series-noise" in lib.anm_last_error()
    desc, keep = _lib.network_desc(sim.model)
    descs = (C.POINTER(_lib.NetworkDesc) * 2)(C.pointer(desc), C.pointer(desc))
    assert lib.anm_model_set_classes(sim._handle, 2, descs) != 0 and b"parameter classes" in lib.anm_last_error()
    env.reset()
    env.step(a)

    # anm_model_set_env with an anm_env_config_corr, on a series-mode model
    plain = make_env("anm6", "radial", 41, 1, mode="series")
    psim = plain.simulator
    slo, shi = plain._cfg_keep
    z_dev = torch.zeros((41, n), dtype=torch.float64, device=DEV)

    def cfg(cls=_lib.EnvConfigCorr, **b):
        arr = {k: np.ascontiguousarray(b.get(k, d), dtype=np.float64)
               for k, d in (("lo", low), ("hi", high), ("amp", amp), ("ser", ser), ("rho", rho), ("innov", rng.exo_innovation(rho)))}
        c = cls(K=b.get("K", 1), gamma=0.9, clip_e_loss=1.0, clip_penalty=100.0, obs_low=_lib.as_c(slo, np.float64)[1],
                obs_high=_lib.as_c(shi, np.float64)[1],
                series=None if b.get("no_series") else arr["ser"].ctypes.data_as(_lib.c_double_p), period=0 if b.get("no_series") else ser.shape[1],
                exo_mode=b.get("mode", _lib.EXO_SERIES_NOISE), exo_low=arr["lo"].ctypes.data_as(_lib.c_double_p),
                exo_high=arr["hi"].ctypes.data_as(_lib.c_double_p))
        if not b.get("no_amp"):
            c.exo_noise = arr["amp"].ctypes.data_as(_lib.c_double_p)
        if cls is _lib.EnvConfigCorr:
            for k, v in (("exo_rho", arr["rho"].ctypes.data_as(_lib.c_double_p)), ("exo_innov", arr["innov"].ctypes.data_as(_lib.c_double_p)),
                         ("exo_z", z_dev.data_ptr())):
                if k not in b.get("null", ()):
                    setattr(c, k, v)
        if "tail" in b:
            C.c_int32.from_address(C.addressof(c) + _lib.EnvConfig.K.offset + 4).value = b["tail"]
        c._keep = arr
        return c

    def vec(k, v):
        x = np.full(n, 0.5)
        x[k] = v
        return x

    assert lib.anm_model_bind_view(psim._handle, C.byref(view)) == 0
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg())) != 0 and b"batch view" in lib.anm_last_error()
    assert lib.anm_model_bind_view(psim._handle, None) == 0
    bad = [(dict(mode=_lib.EXO_UNIFORM, no_series=True), b"needs exo_mode = ANM_EXO_SERIES_NOISE"),
           (dict(mode=_lib.EXO_HOST), b"needs exo_mode = ANM_EXO_SERIES_NOISE"),
           (dict(tail=4), b"unknown value of tail"), (dict(tail=-1), b"unknown value of tail"),
           (dict(null=("exo_rho",)), b"none may be NULL"), (dict(null=("exo_innov",)), b"none may be NULL"), (dict(null=("exo_z",)), b"none may be NULL"),
           (dict(rho=vec(0, 1.0)), b"exo_rho must be finite and in [0, 1)"), (dict(rho=vec(4, -1e-300)), b"exo_rho must be"),
           (dict(rho=vec(2, np.nan)), b"exo_rho must be"), (dict(rho=vec(1, INF)), b"exo_rho must be"),
           (dict(innov=vec(0, 0.0)), b"exo_innov must be finite and in (0, 1]"), (dict(innov=vec(3, 1.0 + 2.0**-52)), b"exo_innov must be"),
           (dict(innov=vec(1, np.nan)), b"exo_innov must be"), (dict(innov=vec(4, -0.5)), b"exo_innov must be"),
           (dict(K=2), b"K = 1"), (dict(no_series=True), b"needs a series"), (dict(no_amp=True), b"amplitude table")]
    for b, msg in bad:
        c = cfg(**b)
        assert lib.anm_model_set_env(psim._handle, C.byref(c)) != 0, b
        assert msg in lib.anm_last_error(), (b, lib.anm_last_error())
    # structs with the older tails are read as before: the pointers behind exo_noise are not looked at
    c = cfg(null=("exo_rho", "exo_innov", "exo_z"), tail=_lib.ENV_TAIL_NOISE)
    assert lib.anm_model_set_env(psim._handle, C.byref(c)) == 0
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg())) == 0          # ... and the struct as it should be
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg(rho=np.zeros(n), innov=np.ones(n)))) == 0

    # the public classes
    net6 = networks.anm6_network()
    mk = lambda **kw: BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, series=ser, **kw)  # noqa: E731
    with pytest.raises(errors.ArgsError, match="exo_corr needs"):
        mk(exo_corr=0.5)
    with pytest.raises(errors.ArgsError, match="exo_corr needs"):
        BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="uniform", exo_corr=0.5)
    for shape in (np.zeros(4), np.zeros((5, 96)), np.zeros((1, 5))):
        with pytest.raises(errors.ArgsError, match="scalar or have 5 entries"):
            mk(exogenous="series_noise", exo_noise=1.0, exo_corr=shape)
    for value in (1.0, -0.25, np.nan, INF, vec(3, 1.0)):
        with pytest.raises(errors.ArgsError, match=r"in \[0, 1\)"):
            mk(exogenous="series_noise", exo_noise=1.0, exo_corr=value)
    with pytest.raises(errors.EnvInitializationError, match="parameter classes"):
        make_env("anm6", "radial", 41, 1, exo_corr=0.5, variants=[networks.anm6_network()], env_variant=np.zeros(41, dtype=np.int32))
    with pytest.raises(errors.EnvInitializationError, match="drawn in"):
        MixedBatchedANMEnv([dict(network=net6, series=ser, exogenous="series_noise", exo_noise=1.0, exo_corr=0.5)], [0, 0, 0, 0], device=DEV)

    # the agents: the stream forecast is refused, the profile forecast and the constant one read state and tables alone
    unc, env = make_env("anm6", "radial", 41, 1), make_env("anm6", "radial", 41, 1, exo_corr=rho)
    sim = env.simulator
    unc.reset()
    env.reset()
    assert torch.equal(env.state, unc.state) and torch.equal(env.simulator.soc, unc.simulator.soc)      # the same drawn rows for every rho
    with pytest.raises(errors.ArgsError, match="correlated noise"):
        MPCAgentPerfectStream(sim, env.action_space, env.gamma, planning_steps=2)
    stream = MPCAgentPerfectStream(unc.simulator, unc.action_space, unc.gamma, planning_steps=2)
    stream.act(unc)
    for call in (stream.act, stream.forecast, lambda e: stream.solver.act(3, e, stream._lo, stream._hi)):
        with pytest.raises(errors.ArgsError, match="correlated noise"):
            call(env)
    for Agent in (MPCAgentPerfect, MPCAgentConstant):
        on_cor = Agent(sim, env.action_space, env.gamma, safety_margin=0.92, planning_steps=4)
        on_unc = Agent(unc.simulator, unc.action_space, unc.gamma, safety_margin=0.92, planning_steps=4)
        on_cor.warn_unconverged = on_unc.warn_unconverged = False
        assert torch.equal(on_cor.act(env), on_unc.act(unc)), Agent.__name__
