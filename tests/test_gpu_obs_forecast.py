"""GPU tier: the expected forecast written by the step and reset kernels (``BatchedANMEnv(exogenous="series_noise",
forecast_horizon=H)``, ``env.exo_forecast`` ``[num_envs, n_exo, H]``; specification: gym_anm_amd/rng.py,
exo_forecast_expected).  ONE invariant: after every reset() and step(), for every environment, the row equals the
specification at (state[e, -1], exo_z[e]) bit for bit.  After tests/test_gpu_exo_noise.py and tests/test_gpu_exo_corr.py,
whose task tables and helpers these tests use:
  1. the invariant, with and without in-kernel resets; 2. the feature changes nothing else; 3. nothing outside the rows is
  written; 4. reset() from rows, masked reset(), the absorbing step; 5. float32 I/O; 6. shards; 7. HIP graph, no allocation;
  8. a list-form observation beside it; 9. what the C ABI refuses; 10. MPCAgentExpected.forecast reads the buffer.
Batches: 229 (thread-per-environment family) / 41 (lane-group families): partial last blocks, whose idle lanes run on a
clamped environment index and must store nothing; ANM6 at 1, 63, 65 / 1, 9 once."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.agents import MPCAgentExpected
from gym_anm_amd.envs.anm6 import ANM6EasyVec
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.envs.mixed import MixedBatchedANMEnv

from parity_common import uniform_actions
from test_gpu_exo_corr import batch_of, outputs, rho_of
from test_gpu_exo_noise import CASES, DEV, NETS, make_env, task_of

pytestmark = pytest.mark.gpu

# the seed of the ANM6 thread runs without autoreset: some of the 229 environments terminate within the 20 steps under it
# (test_the_invariant asserts it) -- the zero row with table index 0 is then part of what is compared
SEED_TERMINAL = 5


def expected(env, net, H=None):
    """the specification at what the environment holds now: [E, n_exo, H] float64"""
    ser, amp, low, high = task_of(net)
    corr = env.exo_corr is not None
    return rng.exo_forecast_expected_v(env.num_envs, env.forecast_horizon if H is None else H, low, high,
                                       aux=env.state[:, -1].cpu().numpy().astype(np.int64),
                                       z=env.exo_z.cpu().numpy() if corr else None, series=ser, noise=amp,
                                       rho=env.exo_corr if corr else None)


def assert_invariant(env, net, what):
    got, want = env.exo_forecast.cpu().numpy(), expected(env, net)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), "%s: %d of %d rows differ" % (what, int((got != want).any(axis=(1, 2)).sum()), len(got))


def corr_of(net, corr):
    return rho_of(net) if corr else None


# ---- 1. the invariant ------------------------------------------------------------------------------------------------------
def run_invariant(net, impl, E_, corr, H, autoreset, seed):
    kw = dict(autoreset=True, max_episode_steps=5) if autoreset else {}
    env = make_env(net, impl, E_, seed, exo_corr=corr_of(net, corr), forecast_horizon=H, **kw)
    n_exo = task_of(net)[0].shape[0]
    assert env.forecast_horizon == H and env.exo_forecast.shape == (E_, n_exo, H) and env.exo_forecast.dtype == torch.float64
    assert env.forecast_space.shape == (n_exo, H) and env.forecast_space.dtype == np.float64
    assert np.array_equal(env.forecast_space.low, np.broadcast_to(env.exo_low[:, None], (n_exo, H)))
    assert np.array_equal(env.forecast_space.high, np.broadcast_to(env.exo_high[:, None], (n_exo, H)))
    ptr = env.exo_forecast.data_ptr()
    out = env.reset()
    assert isinstance(out, tuple) and len(out) == 2
    assert_invariant(env, net, "reset")
    gen = torch.Generator(device=DEV).manual_seed(7)
    n_term = n_reset = 0
    for t in range(20):
        rc0 = env._reset_count.clone()
        out = env.step(uniform_actions(env, gen))
        assert len(out) == 5
        assert_invariant(env, net, "step %d (%s, %s, E = %d, corr %s, H = %d, autoreset %s)" % (t, net, impl, E_, corr, H, autoreset))
        n_term += int(env.terminated.sum())
        n_reset += int((env._reset_count != rc0).sum())
    assert env.exo_forecast.data_ptr() == ptr
    return env, n_term, n_reset


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("H", [1, 3, 7])
@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("net,impl", CASES)
def test_the_invariant(net, impl, corr, H, autoreset):
    E_ = batch_of(impl)
    seed = SEED_TERMINAL if (net, impl, autoreset) == ("anm6", "thread", False) else 31
    env, n_term, n_reset = run_invariant(net, impl, E_, corr, H, autoreset, seed)
    if autoreset:      # the limit of 5 re-initialises everybody every six calls, inside the kernels
        assert n_reset >= 3 * E_
    else:
        assert n_reset == 0
        if (net, impl) == ("anm6", "thread"):
            # terminated environments: the zero row, table index 0, the noise states the terminal step stored
            dead = env.terminated
            assert int(dead.sum()) >= 1 and not bool(env.state[dead].any())
            want0 = expected(env, net)[dead.cpu().numpy()]
            ser, amp, low, high = task_of(net)
            if not corr:   # no noise state: the clipped table from index 1 on
                x = np.clip(ser[:, (1 + np.arange(H)) % ser.shape[1]], low[:, None], high[:, None])
                assert np.array_equal(want0, np.broadcast_to(x, want0.shape))


@pytest.mark.parametrize("impl,E_", [("thread", 1), ("thread", 63), ("thread", 65), ("radial", 1), ("radial", 9), ("mesh", 1), ("mesh", 9)])
def test_the_invariant_at_small_batches(impl, E_):
    run_invariant("anm6", impl, E_, True, 7, True, 31)


# ---- 2. the feature changes nothing else -------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("net,impl", CASES)
def test_the_feature_changes_nothing_else(net, impl, corr):
    kw = dict(autoreset=True, max_episode_steps=5, exo_corr=corr_of(net, corr))
    a = make_env(net, impl, batch_of(impl), 31, **kw)
    b = make_env(net, impl, batch_of(impl), 31, forecast_horizon=7, **kw)
    assert a.forecast_horizon is None and a.exo_forecast is None and a.forecast_space is None
    oa, ob = a.reset()[0], b.reset()[0]
    gen = torch.Generator(device=DEV).manual_seed(5)
    for t in range(21):
        if t:
            act = uniform_actions(a, gen)
            oa, ob = a.step(act)[0], b.step(act)[0]
        for (name, x), (_, y) in zip(outputs(a, oa), outputs(b, ob)):
            assert torch.equal(x, y), "step %d: %s differs" % (t, name)
        if corr:
            assert torch.equal(a.exo_z, b.exo_z), t
    assert int(b._reset_count.min()) >= 4


# ---- 3. nothing outside the rows is written ----------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial")])
def test_nothing_outside_the_rows_is_written(net, impl, corr):
    E_, H = batch_of(impl), 7
    env = make_env(net, impl, E_, 31, exo_corr=corr_of(net, corr), forecast_horizon=H, autoreset=True, max_episode_steps=3)
    n_exo = env.exo_forecast.shape[1]
    big = torch.full((3 * E_, n_exo, H), float("nan"), dtype=torch.float64, device=DEV)
    cfg = env._env_config()
    # (_env_config gave the environment a new exo_z and put it into cfg: both agree)
    cfg.exo_forecast = big[E_:].data_ptr()
    sim = env.simulator
    sim.backend.check(sim.backend.lib.anm_model_set_env(sim._handle, C.byref(cfg)), "anm_model_set_env")
    env.exo_forecast = big[E_:2 * E_]
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(3)
    for t in range(5):
        env.step(uniform_actions(env, gen))
    assert_invariant(env, net, "the rows of the batch")
    assert bool(torch.isnan(big[:E_]).all()) and bool(torch.isnan(big[2 * E_:]).all())
    assert not bool(torch.isnan(big[E_:2 * E_]).any())


# ---- 4. reset() from rows, masked reset(), the absorbing step ----------------------------------------------------------------
@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("net,impl", CASES)
def test_resets_write_the_row_and_the_absorbing_step_leaves_it_alone(net, impl, corr):
    E_, H = batch_of(impl), 7
    env = make_env(net, impl, E_, 17, exo_corr=corr_of(net, corr), forecast_horizon=H, env_offset=(1 << 32) - 7)
    f = lambda: env.exo_forecast.cpu().numpy().copy()  # noqa: E731
    gen = torch.Generator(device=DEV).manual_seed(11)
    env.reset()
    assert_invariant(env, net, "reset")
    for _ in range(3):
        env.step(uniform_actions(env, gen))
    f0 = f()
    # masked reset(): the device sampler for every third environment; the others keep their rows
    mask = torch.arange(E_, device=DEV) % 3 == 1
    m = mask.cpu().numpy()
    env.reset(options={"mask": mask})
    f1 = f()
    assert_invariant(env, net, "masked reset")
    assert f1[~m].tobytes() == f0[~m].tobytes() and (f1[m] != f0[m]).any(axis=(1, 2)).sum() > m.sum() // 2
    # reset() from rows the caller brings (another table index), masked
    rows = env.sample_init_state()
    rows[:, -1] = torch.remainder(rows[:, -1] + 2, task_of(net)[0].shape[1])
    mask2 = torch.arange(E_, device=DEV) % 4 == 0
    m2 = mask2.cpu().numpy()
    env.reset(options={"init_state": rows, "mask": mask2})
    f2 = f()
    assert_invariant(env, net, "masked reset from rows")
    assert f2[~m2].tobytes() == f1[~m2].tobytes() and torch.equal(env.state[mask2][:, -1], rows[mask2][:, -1])
    # ... and without a mask
    env.reset(options={"init_state": rows})
    assert_invariant(env, net, "reset from rows")
    assert torch.equal(env.state[:, -1], rows[:, -1])
    # the absorbing step: rows forced terminal, no autoreset -- nothing of them is touched, the forecast included
    env.step(uniform_actions(env, gen))
    dead = torch.arange(E_, device=DEV) % 5 == 2
    d = dead.cpu().numpy()
    env._term_u8[dead] = 1
    f3, s3 = f(), env.state.clone()
    env.step(uniform_actions(env, gen))
    f4 = f()
    assert f4[d].tobytes() == f3[d].tobytes() and torch.equal(env.state[dead], s3[dead])
    assert_invariant(env, net, "after an absorbing step")
    alive = ~d & ~env.terminated.cpu().numpy()
    moved = (f4[alive] != f3[alive]).any(axis=(1, 2))       # (without noise states a window on a plateau of the table stays)
    assert alive.any() and (moved.all() if corr else moved.any())


# ---- 5. ... 7. composition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_float32_io_is_the_float64_run_rounded_once(net, impl):
    kw = dict(autoreset=True, max_episode_steps=7, exo_corr=rho_of(net), forecast_horizon=7)
    a = make_env(net, impl, batch_of(impl), 8, **kw)
    b = make_env(net, impl, batch_of(impl), 8, io_dtype=torch.float32, **kw)
    assert b.exo_forecast.dtype == torch.float32 and b.forecast_space.dtype == np.float32 and a.forecast_space.dtype == np.float64
    assert np.array_equal(b.forecast_space.low, a.forecast_space.low.astype(np.float32))
    assert np.array_equal(b.forecast_space.high, a.forecast_space.high.astype(np.float32))
    a.reset()
    b.reset()
    gen = torch.Generator(device=DEV).manual_seed(2)
    for t in range(13):
        if t:
            act32 = uniform_actions(a, gen).float()
            a.step(act32.double())
            b.step(act32)
        assert b.exo_forecast.dtype == torch.float32
        assert torch.equal(b.exo_forecast, a.exo_forecast.float()), t
        assert torch.equal(a.state, b.state) and torch.equal(a.exo_z, b.exo_z), t
    assert_invariant(a, net, "the float64 twin")


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_two_shards_equal_the_whole_batch(impl):
    E_ = batch_of(impl)
    H0 = E_ // 2 - 3
    kw = dict(autoreset=True, max_episode_steps=4, exo_corr=rho_of("anm6"), forecast_horizon=3)
    whole = make_env("anm6", impl, E_, 77, **kw)
    shards = [make_env("anm6", impl, n, 77, env_offset=off, **kw) for off, n in ((0, H0), (H0, E_ - H0))]
    whole.reset(seed=77)
    for s in shards:
        s.reset(seed=77)
    gen = torch.Generator(device=DEV).manual_seed(3)
    for t in range(11):
        if t:
            a = uniform_actions(whole, gen)
            whole.step(a)
            for s, (lo_, hi_) in zip(shards, ((0, H0), (H0, E_))):
                s.step(a[lo_:hi_].contiguous())
        assert torch.equal(whole.exo_forecast, torch.cat([s.exo_forecast for s in shards])), t
        assert torch.equal(whole.state, torch.cat([s.state for s in shards])), t
    assert_invariant(whole, "anm6", "the whole batch")


@pytest.mark.parametrize("net,impl", CASES)
def test_a_captured_step_replays_what_eager_steps_compute_and_allocates_nothing(net, impl):
    kw = dict(autoreset=True, exo_corr=rho_of(net), forecast_horizon=7)
    eager, graphed = make_env(net, impl, batch_of(impl), 21, **kw), make_env(net, impl, batch_of(impl), 21, **kw)
    eager.reset()
    graphed.reset()
    ptr = graphed.exo_forecast.data_ptr()
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = [uniform_actions(eager, gen) for _ in range(12)]
    a_buf = acts[0].clone()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):       # the FIRST step after reset() is the captured one
            graphed.step(a_buf)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    assert not bool(graphed.timestep.any()) and torch.equal(eager.exo_forecast, graphed.exo_forecast)      # (capturing ran nothing)
    before = None
    for t, act in enumerate(acts):
        a_buf.copy_(act)
        g.replay()
        eager.step(act)
        torch.cuda.synchronize()
        if t == 1:
            before = torch.cuda.memory_allocated(DEV)
        assert torch.equal(eager.exo_forecast, graphed.exo_forecast) and torch.equal(eager.state, graphed.state), "replay %d" % t
        assert graphed.exo_forecast.data_ptr() == ptr
    assert torch.cuda.memory_allocated(DEV) == before
    assert_invariant(graphed, net, "after 12 replays")
    assert bool((eager.timestep == 12).any())


# ---- 8. a list-form observation beside the forecast ----------------------------------------------------------------------------
LIST_OBS = [("bus_v_magn", "all", "pu"), ("branch_s", "all", "MVA"), ("des_soc", "all", "MWh"), ("aux", "all")]


def make_list_env(net, impl, E_, seed, **kw):
    ser, amp, low, high = task_of(net)
    env = BatchedANMEnv(NETS[net](), LIST_OBS, 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, ser.shape[1] - 1),)), costs_clipping=(1, 100),
                        seed=seed, num_envs=E_, device=DEV, tol=1e-6, impl=impl, exogenous="series_noise", exo_noise=amp, exo_low=low,
                        exo_high=high, series=ser, **kw)
    assert env.simulator.impl == impl and env._obs_fused
    env.check_actions = False
    return env


@pytest.mark.parametrize("net,impl", [("case30", "radial"), ("anm6", "mesh")])
def test_a_list_form_observation_beside_the_forecast(net, impl):
    kw = dict(autoreset=True, max_episode_steps=5, exo_corr=rho_of(net))
    a = make_list_env(net, impl, 41, 9, **kw)
    b = make_list_env(net, impl, 41, 9, forecast_horizon=7, **kw)
    oa, ob = a.reset()[0], b.reset()[0]
    gen = torch.Generator(device=DEV).manual_seed(6)
    for t in range(13):
        if t:
            act = uniform_actions(a, gen)
            oa, ob = a.step(act)[0], b.step(act)[0]
        assert oa.shape[1] == len(a._gather[0]) and torch.equal(oa, ob), t
        for (name, x), (_, y) in zip(outputs(a), outputs(b)):
            assert torch.equal(x, y), "step %d: %s differs" % (t, name)
        assert_invariant(b, net, "step %d beside a list-form observation" % t)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_what_the_c_abi_and_the_constructors_refuse():
    ser, amp, low, high = task_of("anm6")
    n, E_ = ser.shape[0], 41
    rho = rho_of("anm6")
    plain = make_env("anm6", "radial", E_, 1, mode="series")
    psim = plain.simulator
    lib = psim.backend.lib
    slo, shi = plain._cfg_keep
    z_dev = torch.zeros((E_, n), dtype=torch.float64, device=DEV)
    f_dev = torch.zeros((E_, n, 64), dtype=torch.float64, device=DEV)

    def cfg(**b):
        arr = {k: np.ascontiguousarray(b.get(k, d), dtype=np.float64)
               for k, d in (("lo", low), ("hi", high), ("amp", amp), ("ser", ser), ("rho", rho), ("innov", rng.exo_innovation(rho)))}
        c = _lib.EnvConfigForecast(
            K=1, gamma=0.9, clip_e_loss=1.0, clip_penalty=100.0, obs_low=_lib.as_c(slo, np.float64)[1], obs_high=_lib.as_c(shi, np.float64)[1],
            series=None if b.get("no_series") else arr["ser"].ctypes.data_as(_lib.c_double_p), period=0 if b.get("no_series") else ser.shape[1],
            exo_mode=b.get("mode", _lib.EXO_SERIES_NOISE), exo_low=arr["lo"].ctypes.data_as(_lib.c_double_p),
            exo_high=arr["hi"].ctypes.data_as(_lib.c_double_p), exo_noise=arr["amp"].ctypes.data_as(_lib.c_double_p),
            forecast_horizon=b.get("H", 8))
        for k, v in (("exo_rho", arr["rho"].ctypes.data_as(_lib.c_double_p)), ("exo_innov", arr["innov"].ctypes.data_as(_lib.c_double_p)),
                     ("exo_z", z_dev.data_ptr())):
            if k not in b.get("null", ()):
                setattr(c, k, v)
        if not b.get("no_buffer"):
            c.exo_forecast = f_dev.data_ptr()
        if "tail" in b:
            C.c_int32.from_address(C.addressof(c) + _lib.EnvConfig.K.offset + 4).value = b["tail"]
        c._keep = arr
        return c

    trio = ("exo_rho", "exo_innov", "exo_z")
    assert _lib.ENV_TAIL_FORECAST == 5
    bad = [(dict(tail=4), b"unknown value of tail"), (dict(tail=6), b"unknown value of tail"),     # (4 was refused before the forecast: it still is)
           (dict(H=0), b"forecast_horizon"), (dict(H=65), b"forecast_horizon"), (dict(H=-1), b"forecast_horizon"),
           (dict(no_buffer=True), b"needs exo_forecast"),
           (dict(mode=_lib.EXO_UNIFORM, no_series=True), b"needs exo_mode = ANM_EXO_SERIES_NOISE"),
           (dict(mode=_lib.EXO_HOST), b"needs exo_mode = ANM_EXO_SERIES_NOISE"),
           (dict(null=("exo_rho",)), b"all set (correlated noise) or all NULL"), (dict(null=("exo_innov",)), b"all set (correlated noise) or all NULL"),
           (dict(null=("exo_z",)), b"all set (correlated noise) or all NULL"), (dict(null=("exo_rho", "exo_z")), b"all set (correlated noise) or all NULL"),
           (dict(no_series=True), b"needs a series")]
    for b, msg in bad:
        c = cfg(**b)
        assert lib.anm_model_set_env(psim._handle, C.byref(c)) != 0, b
        assert msg in lib.anm_last_error(), (b, lib.anm_last_error())
    # a bound batch view, parameter classes: what the series-noise mode refuses
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(psim._handle, C.byref(view)) == 0
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg())) != 0 and b"batch view" in lib.anm_last_error()
    assert lib.anm_model_bind_view(psim._handle, None) == 0
    # the struct as it should be: correlated, and without noise states (the trio all NULL); H = 1 and 64
    for b in (dict(), dict(null=trio), dict(H=1), dict(H=64, null=trio)):
        assert lib.anm_model_set_env(psim._handle, C.byref(cfg(**b))) == 0, (b, lib.anm_last_error())
    assert lib.anm_model_bind_view(psim._handle, C.byref(view)) != 0 and b"series-noise" in lib.anm_last_error()
    cls = torch.zeros(E_, dtype=torch.int32, device=DEV)
    assert lib.anm_model_bind_env_classes(psim._handle, cls.data_ptr(), E_) != 0 and b"series-noise" in lib.anm_last_error()

    # the public classes
    net6 = networks.anm6_network()
    mk = lambda **kw: BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, **kw)  # noqa: E731
    with pytest.raises(errors.ArgsError, match="forecast_horizon needs"):
        mk(series=ser, forecast_horizon=4)
    with pytest.raises(errors.ArgsError, match="forecast_horizon needs"):
        mk(exogenous="uniform", forecast_horizon=4)
    for value in (0, 65, -3):
        with pytest.raises(errors.ArgsError, match=r"in \[1, 64\]"):
            mk(series=ser, exogenous="series_noise", exo_noise=1.0, forecast_horizon=value)
    for value in (2.0, "3", True):
        with pytest.raises(errors.ArgsError, match="should be an int"):
            mk(series=ser, exogenous="series_noise", exo_noise=1.0, forecast_horizon=value)
    with pytest.raises(errors.EnvInitializationError, match="forecast"):
        MixedBatchedANMEnv([dict(network=net6, series=ser, forecast_horizon=4)], [0, 0, 0, 0], device=DEV)


def test_anm6easyvec_takes_the_keyword_through():
    env = ANM6EasyVec(num_envs=41, device=DEV, seed=3, tol=1e-6, exogenous="series_noise", exo_noise=0.5, exo_corr=0.8, autoreset=True,
                      forecast_horizon=64)
    env.check_actions = False
    assert env.forecast_horizon == 64 and env.exo_forecast.shape == (41, 5, 64) and env.forecast_space.shape == (5, 64)
    env.reset()
    env.step(uniform_actions(env, torch.Generator(device=DEV).manual_seed(1)))
    lo, hi = rng.default_exo_bounds(env.simulator.model)
    want = rng.exo_forecast_expected_v(41, 64, lo, hi, aux=env.state[:, -1].cpu().numpy().astype(np.int64), z=env.exo_z.cpu().numpy(),
                                       series=env._series, noise=env.exo_noise, rho=env.exo_corr)
    assert env.exo_forecast.cpu().numpy().tobytes() == want.tobytes()


# ---- 10. the agent reads the buffer ----------------------------------------------------------------------------------------------
class HostForecast(MPCAgentExpected):
    """the host path of forecast(), whatever the environment offers"""

    def forecast(self, env):
        keep, env.forecast_horizon = env.forecast_horizon, None
        try:
            return super().forecast(env)
        finally:
            env.forecast_horizon = keep


@pytest.mark.parametrize("corr", [True, False])
def test_the_agent_reads_the_forecast_from_the_buffer(corr):
    E_, N = 67, 3
    kw = dict(exo_corr=corr_of("anm6", corr))
    env = make_env("anm6", "thread", E_, 12, forecast_horizon=7, **kw)
    twin = make_env("anm6", "thread", E_, 12, **kw)
    short = make_env("anm6", "thread", E_, 12, forecast_horizon=2, **kw)             # shorter than the plan: the host path
    env32 = make_env("anm6", "thread", E_, 12, forecast_horizon=7, io_dtype=torch.float32, **kw)
    mk = lambda cls, e: cls(e.simulator, e.action_space, e.gamma, safety_margin=0.92, planning_steps=N)  # noqa: E731
    agent, host, on_twin = mk(MPCAgentExpected, env), mk(HostForecast, env), mk(MPCAgentExpected, twin)
    agent.warn_unconverged = on_twin.warn_unconverged = False
    for e in (env, twin, short, env32):
        e.reset()
    gen = torch.Generator(device=DEV).manual_seed(9)
    for t in range(3):
        if t:
            a32 = uniform_actions(env, gen).float()
            for e in (env, twin, short):
                e.step(a32.double())
            env32.step(a32)
        calls = []
        orig = rng.exo_forecast_expected_v
        rng.exo_forecast_expected_v = lambda *a_, **k_: (calls.append(1), orig(*a_, **k_))[1]
        try:
            got = agent.forecast(env)
            assert not calls                                       # from the buffer: the host specification is not run
            want = host.forecast(env)
            assert len(calls) == 1
            for e in (short, env32, twin):                         # too short, float32, no buffer: the host path, as before
                other = mk(MPCAgentExpected, e).forecast(e)
                assert len(calls) == 2 and torch.equal(other[0], want[0]) and torch.equal(other[1], want[1])
                calls.pop()
        finally:
            rng.exo_forecast_expected_v = orig
        assert len(got) == 2 and got[0].shape == (E_, 3, N) and got[1].shape == (E_, 2, N)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), t
        assert torch.equal(agent.act(env), on_twin.act(twin)), t                      # act() is unchanged
