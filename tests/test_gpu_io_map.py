"""GPU tier: affine policy I/O in the step kernels (``BatchedANMEnv(action_map=, obs_map=, reward_scale=)``,
``anm_model_set_io_map``; the specification is gym_anm_amd/io_affine.py).  Every comparison is exact -- ``torch.equal``, float32
tensors through ``.view(torch.int32)``; no tolerance anywhere.  A pair is built from one seed: A is mapped and steps with u, B is
plain and steps with ``io_affine.map_action(u)`` evaluated exactly on the host; every raw output and every episode statistic
of A equals B's, and A's obs / reward are ``map_obs`` / ``map_reward`` of B's (then the one float32 rounding).
  1. pairs over the five (network, family) pairs, both modes, both dtypes, partial maps;  2. terminal-on-entry rows;  3. tails;
  4. the fused list observation;  5. the two-launch step;  6. masked reset();  7. nothing allocated, capturable;  8. refusals
  and NULL;  9. the NumPy adapter.
Modes: "series", "uniform", and the series-noise task of tests/test_gpu_exo_noise.py with the expected forecast (H = 3) --
"noise" (white noise) and "noise_corr" (AR(1), ``exo_corr=rho_of(net)``): the map beside the ``exo_z`` read-modify-write and
the forecast rows, which stay raw MW (``exo_forecast`` of A is B's, rounded once to A's io_dtype)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, io_affine, io_dtype, networks
from gym_anm_amd.envs import ANM6EasyVec, MixedBatchedANMEnv, NumpyVectorEnv
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv

from test_gpu_exo_corr import rho_of
from test_gpu_exo_noise import task_of
from test_gpu_io_f32 import F64_OUT, FAMILIES, LIST_OBS, NETS, STATS, device_reset, f64_outputs, series_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.995
F32, F64 = torch.float32, torch.float64
FULL_MAP = dict(action_map="unit", obs_map="box", reward_scale=1 / 64)
E_THREAD, E_GROUP = 165, 229   # two full wavefronts and a partial one; a partial last lane group
NOISE_MODES, H_NOISE = ("noise", "noise_corr"), 3


def n_envs(impl):
    return E_THREAD if impl == "thread" else E_GROUP


def make_env(net, impl, mode, E_, seed, observation="state", **kw):
    if mode == "series":
        ser = series_of(net)
        kw.update(series=ser, aux_bounds=np.array(((0, ser.shape[1] - 1),)))
    elif mode in NOISE_MODES:
        ser, amp, low, high = task_of(net)
        kw.update(exogenous="series_noise", series=ser, exo_noise=amp, exo_low=low, exo_high=high, forecast_horizon=H_NOISE,
                  exo_corr=rho_of(net) if mode == "noise_corr" else None, aux_bounds=np.array(((0, ser.shape[1] - 1),)))
    else:
        assert mode == "uniform"
        kw.update(exogenous="uniform", aux_bounds=np.array(((0, 1000),)))
    env = BatchedANMEnv(NETS[net](), observation, 1, 0.25, GAMMA, 100, costs_clipping=(1, 100), seed=seed, num_envs=E_,
                        device=DEV, tol=1e-6, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def make_pair(net, impl, mode, E_, seed, maps=FULL_MAP, io_dtype=None, **kw):
    """A: mapped (in io_dtype).  B: plain float64, otherwise the same environment."""
    return make_env(net, impl, mode, E_, seed, io_dtype=io_dtype, **maps, **kw), make_env(net, impl, mode, E_, seed, **kw)


def same_bits(x, y):
    assert x.dtype == y.dtype and x.shape == y.shape
    if x.dtype == F32:
        return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    return torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))


def unit_actions(env, gen):
    """u uniform over [-1.25, 1.25] in the environment's io_dtype: a fifth of the entries leave [-1, 1] and meet the clamp"""
    u = 2.5 * torch.rand((env.num_envs, env.action_space.shape[0]), generator=gen, dtype=F64, device=DEV) - 1.25
    return u.to(env.io_dtype).contiguous()


def decode(a, u):
    """what B is fed: the exact host evaluation of rule 1 on what A reads (A without action_map: u itself, widened)"""
    m = a.io_map["action"]
    if m is None:
        return u.double()
    return torch.as_tensor(io_affine.map_action(u.cpu().numpy(), *m), dtype=F64, device=DEV)


def expect_obs(a, ob):
    m = a.io_map["obs"]
    x = ob if m is None else torch.as_tensor(io_affine.map_obs(ob.cpu().numpy(), *m), dtype=F64, device=DEV)
    return x.to(a.io_dtype)


def expect_reward(a, rb):
    x = torch.as_tensor(io_affine.map_reward(rb.cpu().numpy(), a.io_map["reward_scale"]), dtype=F64, device=DEV)
    return x.to(a.io_dtype)


def compare(a, b, oa, ob, where, stats=False, ra=None, rb=None):
    xa, xb = f64_outputs(a), f64_outputs(b)
    for k in F64_OUT:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), "%s: %s differs" % (where, k)
    if stats:
        for k in STATS:
            assert torch.equal(getattr(a, k), getattr(b, k)), "%s: %s differs" % (where, k)
    assert oa.dtype == a.io_dtype and ob.dtype == F64 and oa.shape == ob.shape
    assert same_bits(oa, expect_obs(a, ob)), "%s: obs is not map_obs of the plain mode's" % where
    ra = a.reward if ra is None else ra
    rb = b.reward if rb is None else rb
    assert ra.dtype == a.io_dtype and same_bits(ra, expect_reward(a, rb)), "%s: reward is not map_reward of the plain mode's" % where
    if a.forecast_horizon is not None:     # the series-noise modes: the noise states are B's, the forecast stays raw MW under the map
        assert (a.exo_z is None) == (b.exo_z is None) == (a.exo_corr is None)
        if a.exo_z is not None:
            assert a.exo_z.dtype == F64 and same_bits(a.exo_z, b.exo_z), "%s: exo_z differs" % where
        assert a.exo_forecast.dtype == a.io_dtype and b.exo_forecast.dtype == F64 and a.exo_forecast.shape == b.exo_forecast.shape
        assert same_bits(a.exo_forecast, b.exo_forecast.to(a.io_dtype)), "%s: exo_forecast is not the plain mode's, rounded once" % where
    lo = torch.as_tensor(a.observation_space.low, device=DEV)
    hi = torch.as_tensor(a.observation_space.high, device=DEV)
    assert lo.dtype == a.io_dtype
    inside = ((oa >= lo) & (oa <= hi)).all(dim=1)
    assert bool((inside | a.terminated).all()), "%s: obs outside the mapped Box" % where


def rollout(a, b, n_steps, seed, where, stats=False, before_step=None):
    oa, _ = device_reset(a)
    ob, _ = device_reset(b)
    compare(a, b, oa, ob, where + " reset", stats)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n_reset = 0
    for t in range(n_steps):
        u = unit_actions(a, gen)
        if before_step is not None:
            before_step(t, a, b)
        ts_in = a.timestep.clone()
        oa, ra, ta, _, _ = a.step(u)
        ob, rb, _, _, _ = b.step(decode(a, u))
        assert ra is a.reward and ta.dtype == torch.bool
        compare(a, b, oa, ob, "%s step %d" % (where, t), stats, ra, rb)
        n_reset += int(((a.timestep == 0) & (ts_in > 0)).sum())
    return n_reset


# ---- 1. the mapped mode is the plain mode plus the three maps ---------------------------------------------------------------------
ROLL = dict(autoreset=True, max_episode_steps=3, episode_stats=True)
CASES = [(n, i, m, d) for n, i in FAMILIES for m in ("series", "uniform") for d in (F64, F32)]
CASES += [(n, i, m, d) for n, i in FAMILIES for m in NOISE_MODES for d in (F64, F32)]


@pytest.mark.parametrize("net,impl,mode,dtype", CASES)
def test_mapped_mode_is_the_plain_mode_plus_the_maps(net, impl, mode, dtype):
    E_ = n_envs(impl)
    a, b = make_pair(net, impl, mode, E_, 2718, io_dtype=dtype, **ROLL)
    assert a.io_dtype == dtype and a.action_space.dtype == (np.float32 if dtype == F32 else np.float64)
    assert np.all(a.action_space.low == -1) and np.all(a.action_space.high == 1)
    want = io_dtype.action_bounds32(b.action_space.low, b.action_space.high) if dtype == F32 else (b.action_space.low, b.action_space.high)
    assert a.raw_action_space.dtype == a.action_space.dtype
    assert np.array_equal(a.raw_action_space.low, want[0]) and np.array_equal(a.raw_action_space.high, want[1])
    assert a._state_same is None
    if mode in NOISE_MODES:
        assert a.exo_forecast.shape == (E_, task_of(net)[0].shape[0], H_NOISE) and (a.exo_z is not None) == (mode == "noise_corr")
    n_reset = rollout(a, b, 8, 17, "%s %s %s %s" % (net, impl, mode, dtype), stats=True)
    print("%s %s %s %s: %d in-kernel resets" % (net, impl, mode, dtype, n_reset))
    assert n_reset >= E_          # the limit of 3 sends every environment through the in-kernel autoreset
    assert int(a.episodes_done.min()) >= 1


@pytest.mark.parametrize("maps", [dict(obs_map="box"), dict(action_map="unit"), dict(reward_scale=0.3)], ids=["obs", "action", "reward"])
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial"), ("anm6", "mesh")])
def test_one_map_alone(net, impl, maps):
    """the all-or-none rule of anm_io_map: the parts that are not given are not mapped"""
    E_ = n_envs(impl)
    a, b = make_pair(net, impl, "series", E_, 99, maps=maps, io_dtype=F32, **ROLL)
    io = a.io_map
    assert (io["action"] is None) == ("action_map" not in maps) and (io["obs"] is None) == ("obs_map" not in maps)
    if "action_map" not in maps:   # u is the action itself: keep it inside the MW Box (a float32 one, rounded inward)
        lo, hi = (torch.as_tensor(x, device=DEV) for x in (a.action_space.low, a.action_space.high))
        assert np.array_equal(a.action_space.low, a.raw_action_space.low)
        oa, _ = device_reset(a)
        ob, _ = device_reset(b)
        compare(a, b, oa, ob, "reset")
        gen = torch.Generator(device=DEV).manual_seed(4)
        for t in range(8):
            u = (lo.double() + (hi.double() - lo.double()) * torch.rand((E_, lo.numel()), generator=gen, dtype=F64, device=DEV)).float()
            u = torch.minimum(torch.maximum(u, lo), hi).contiguous()
            oa, ra, _, _, _ = a.step(u)
            ob, rb, _, _, _ = b.step(u.double())
            compare(a, b, oa, ob, "step %d" % t, True, ra, rb)
        assert int(a.episodes_done.min()) >= 1
    else:
        assert rollout(a, b, 8, 4, "%s %s %s" % (net, impl, maps), stats=True) >= E_


# ---- 2. terminal-on-entry rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("net,impl", FAMILIES)
def test_terminal_on_entry_rows_hold_the_bias(net, impl, dtype):
    terminal_on_entry_rows_hold_the_bias(net, impl, dtype, "series")


@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial"), ("anm6", "mesh")])
def test_terminal_on_entry_rows_hold_the_bias_beside_noise_and_forecast(net, impl):
    terminal_on_entry_rows_hold_the_bias(net, impl, F32, "noise_corr")


def terminal_on_entry_rows_hold_the_bias(net, impl, dtype, mode):
    a, b = make_pair(net, impl, mode, n_envs(impl), 5, io_dtype=dtype)

    def mark(t, a, b):
        if t == 0:
            for env in (a, b):
                env._term_u8[::7] = 1

    rollout(a, b, 3, 3, "terminal %s %s %s" % (net, impl, mode), before_step=mark)
    assert bool(a.terminated[::7].all())
    bias = torch.as_tensor(a.io_map["obs"][1], dtype=F64, device=DEV).to(dtype)
    rows = a._state_obs[::7]
    assert same_bits(rows, bias.expand_as(rows).contiguous())          # fma(0, scale, bias): the bias, bit for bit
    assert same_bits(a.reward[::7], torch.zeros_like(a.reward[::7]))     # +0, not -0


# ---- 3. tails ------------------------------------------------------------------------------------------------------------------------
TAILS = [("anm6", "thread", E_) for E_ in (1, 63, 65)] + [(n, i, E_) for n, i in (("anm6", "radial"), ("case30", "mesh")) for E_ in (1, 9)]


@pytest.mark.parametrize("net,impl,E_", TAILS)
def test_tails(net, impl, E_):
    a, b = make_pair(net, impl, "series", E_, 11, io_dtype=F32, **ROLL)
    rollout(a, b, 4, 5, "tail %s %s %d" % (net, impl, E_), stats=True)


# ---- 4. the list-form observation gathered in the kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial"), ("case30", "mesh")])
def test_fused_list_observation(net, impl):
    E_ = n_envs(impl)
    a, b = make_pair(net, impl, "series", E_, 8, io_dtype=F32, observation=LIST_OBS, autoreset=True, max_episode_steps=3)
    assert a._obs_fused and b._obs_fused and a._obs_buf.dtype == F32
    n_obs = a.observation_space.shape[0]
    assert n_obs != a.state_N and all(len(t) == n_obs for t in a.io_map["obs"])     # the tables are sized n_obs
    assert rollout(a, b, 7, 9, "list %s %s" % (net, impl)) >= E_
    # zero rows of terminated environments (no autoreset) hold the bias
    a, b = make_pair(net, impl, "series", 70, 8, io_dtype=F32, observation=LIST_OBS)

    def mark(t, a, b):
        for env in (a, b):
            env._term_u8[::5] = 1

    rollout(a, b, 2, 9, "list terminal %s %s" % (net, impl), before_step=mark)
    bias = torch.as_tensor(a.io_map["obs"][1], dtype=F64, device=DEV).float()
    assert same_bits(a._obs_buf[::5], bias.expand_as(a._obs_buf[::5]).contiguous())


# ---- 5. the two-launch step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_two_launch_step(dtype):
    kw = dict(num_envs=E_THREAD, seed=31, tol=1e-6, device=DEV, **ROLL)
    two = ANM6EasyVec(io_dtype=dtype, straggler_after=6, **FULL_MAP, **kw)
    one = ANM6EasyVec(io_dtype=dtype, straggler_after=None, **FULL_MAP, **kw)
    ref = ANM6EasyVec(straggler_after=6, **kw)
    assert two._ws is not None and one._ws is None and ref._ws is not None
    for env in (two, one, ref):
        env.check_actions = False
        env.reset(seed=31)
    gen = torch.Generator(device=DEV).manual_seed(6)
    seen = 0
    for t in range(8):
        u = unit_actions(two, gen)
        o2, r2, _, _, _ = two.step(u)
        o1, r1, _, _, _ = one.step(u)
        orf, rrf, _, _, _ = ref.step(decode(two, u))
        x2, x1 = f64_outputs(two), f64_outputs(one)
        for k in F64_OUT:
            assert torch.equal(x2[k], x1[k]), "step %d: %s (two launches against one)" % (t, k)
        for k in STATS:
            assert torch.equal(getattr(two, k), getattr(one, k)), "step %d: %s" % (t, k)
        assert same_bits(o2, o1) and same_bits(r2, r1)
        compare(two, ref, o2, orf, "two-launch step %d" % t, True, r2, rrf)
        seen = max(seen, int(two.simulator.nr_iters.max()))
    assert seen > 6                # some solves did go through the straggler launches and the scatter


# ---- 6. masked reset() ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl,observation", [("anm6", "thread", "state"), ("anm6", "radial", "state"), ("case30", "mesh", "state"),
                                                  ("anm6", "thread", LIST_OBS), ("case30", "radial", LIST_OBS)])
def test_masked_reset(net, impl, observation):
    masked_reset(net, impl, observation, "series")


@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("anm6", "radial"), ("case30", "mesh")])
def test_masked_reset_beside_noise_and_forecast(net, impl):
    masked_reset(net, impl, "state", "noise_corr")


def masked_reset(net, impl, observation, mode):
    E_ = 131
    a, b = make_pair(net, impl, mode, E_, 9, io_dtype=F32, observation=observation)
    where = "masked reset %s %s %s" % (net, impl, mode)
    rollout(a, b, 2, 4, where)
    m = torch.arange(E_, device=DEV) % 3 == 0
    oa, _ = device_reset(a, m)                                  # the device sampler
    ob, _ = device_reset(b, m)
    compare(a, b, oa, ob, where + " (device sampler)")
    assert not bool(a.timestep[m].any())
    rows = b.sample_init_state()                                # given rows
    assert torch.equal(rows, a.sample_init_state())
    m2 = torch.arange(E_, device=DEV) % 3 == 1
    oa, _ = a.reset(options={"init_state": rows, "mask": m2})
    ob, _ = b.reset(options={"init_state": rows, "mask": m2})
    compare(a, b, oa, ob, where + " (given rows)")
    u = unit_actions(a, torch.Generator(device=DEV).manual_seed(12))
    oa, ra, _, _, _ = a.step(u)
    ob, rb, _, _, _ = b.step(decode(a, u))
    compare(a, b, oa, ob, where + " (step after)", False, ra, rb)


# ---- 7. one launch, nothing allocated, capturable ---------------------------------------------------------------------------------------
def test_nothing_allocated_and_capturable():
    nothing_allocated_and_capturable()


def test_nothing_allocated_and_capturable_beside_noise_and_forecast():
    nothing_allocated_and_capturable(exogenous="series_noise", exo_noise=0.5, exo_corr=0.8, forecast_horizon=H_NOISE)


def nothing_allocated_and_capturable(**task):
    E_, SEED = 256, 21
    kw = dict(num_envs=E_, seed=SEED, tol=1e-6, device=DEV, io_dtype=F32, **FULL_MAP, **ROLL, **task)
    env, twin = ANM6EasyVec(**kw), ANM6EasyVec(**kw)
    for e in (env, twin):
        e.check_actions = False
        e.reset(seed=SEED)
    gen = torch.Generator(device=DEV).manual_seed(2)
    acts = [unit_actions(env, gen) for _ in range(6)]
    buf = acts[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # the very first step after reset()
        env.step(buf)
    torch.cuda.synchronize()
    assert not bool(env.timestep.any())                      # capture does not execute
    for t, a in enumerate(acts):
        buf.copy_(a)
        g.replay()
        o2, r2, _, _, _ = twin.step(a)
        x, y = f64_outputs(env), f64_outputs(twin)
        for k in F64_OUT:
            assert torch.equal(x[k], y[k]), "replay %d: %s" % (t, k)
        for k in STATS:
            assert torch.equal(getattr(env, k), getattr(twin, k)), "replay %d: %s" % (t, k)
        assert same_bits(env._state_obs, o2) and same_bits(env.reward, r2), "replay %d" % t
        if task:
            assert same_bits(env.exo_z, twin.exo_z) and same_bits(env.exo_forecast, twin.exo_forecast), "replay %d" % t
    assert int(env.episodes_done.min()) >= 1
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for a in acts[:5]:
        buf.copy_(a)
        o, r, _, _, _ = twin.step(buf)
        assert torch.cuda.memory_allocated() == m0
    assert o is twin._state_obs and r is twin.reward and o.dtype == F32 and r.dtype == F32
    if task:
        assert env.exo_forecast.dtype == F32 and env.exo_forecast.shape == (E_, 5, H_NOISE)


def test_the_mapped_anm6easy_step_is_the_coalesced_row_kernel():
    """the hot path: one launch of k_step_rows_map, not the general step kernel (read from the profiler's kernel names)"""
    from torch.profiler import ProfilerActivity, profile

    names = {}
    for dtype in (F64, F32):
        env = ANM6EasyVec(num_envs=E_THREAD, device=DEV, seed=3, tol=1e-6, io_dtype=dtype, **FULL_MAP, **ROLL)
        env.check_actions = False
        env.reset(seed=3)
        u = unit_actions(env, torch.Generator(device=DEV).manual_seed(1))
        env.step(u)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            env.step(u)
            torch.cuda.synchronize()
        names[dtype] = [e.key for e in prof.key_averages() if "k_step" in e.key or "k_radial" in e.key or "k_mesh" in e.key]
        print(dtype, names[dtype])
        assert len(names[dtype]) == 1 and "k_step_rows_map" in names[dtype][0], names[dtype]
    assert names[F64] != names[F32]        # the float64 and the float32 instantiation


# ---- 8. refusals, and NULL ------------------------------------------------------------------------------------------------------------------
def c_map(env, **over):
    """an anm_io_map of the environment's host tables (kept alive by the second value), entries replaced by `over`"""
    io = env.io_map
    tabs = dict(zip(("act_mid", "act_half", "act_low", "act_high"), io["action"]))
    tabs.update(zip(("obs_scale", "obs_bias"), io["obs"]))
    tabs.update({k: v for k, v in over.items() if k != "reward_scale"})
    m, keep = _lib.IoMap(reward_scale=over.get("reward_scale", io["reward_scale"])), []
    for k, v in tabs.items():
        if v is not None:
            arr, ptr = _lib.as_c(v, np.float64)
            keep.append(arr)
            setattr(m, k, ptr)
    return m, keep


def test_what_the_mode_refuses():
    env = make_env("anm6", "radial", "series", 64, 1, **FULL_MAP)
    twin = make_env("anm6", "radial", "series", 64, 1, **FULL_MAP)
    for e in (env, twin):
        device_reset(e)
    gen = torch.Generator(device=DEV).manual_seed(1)
    u = unit_actions(env, gen)
    env.step(u)
    twin.step(u)
    sim = env.simulator
    lib, h = sim.backend.lib, sim._handle
    err = lib.anm_last_error
    io = env.io_map
    # bad tables: the map that is set stays
    bad_half = io["action"][1].copy()
    bad_half[1] = 0.0
    bad_scale = io["obs"][0].copy()
    bad_scale[2] = np.inf
    flipped = io["action"][3].copy()
    flipped[0] = io["action"][2][0] - 1.0
    for over, word in ((dict(act_half=bad_half), b"act_half"), (dict(obs_scale=bad_scale), b"obs_scale"), (dict(reward_scale=0.0), b"reward_scale"),
                       (dict(reward_scale=float("nan")), b"reward_scale"), (dict(act_high=flipped), b"act_low > act_high"),
                       (dict(act_mid=None), b"all NULL"), (dict(obs_bias=None), b"both NULL")):
        m, keep = c_map(env, **over)
        assert lib.anm_model_set_io_map(h, C.byref(m)) != 0 and word in err(), (over, err())
    # the task and the observation list cannot change under a map
    cfg = env._env_config()
    assert lib.anm_model_set_env(h, C.byref(cfg)) != 0 and b"anm_model_set_io_map" in err()
    idx, (sc, p_sc) = _lib.as_c([0, 1], np.int32), _lib.as_c([1.0, 1.0], np.float64)
    assert lib.anm_model_set_obs(h, 2, idx[1], p_sc, p_sc, p_sc) != 0 and b"anm_model_set_io_map" in err()
    # a batch view, parameter classes, anm_model_bind_state_same: from both sides
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(h, C.byref(view)) != 0 and b"affine" in err() and b"batch view" in err()
    cls = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert lib.anm_model_bind_env_classes(h, cls.data_ptr(), 64) != 0 and b"affine" in err() and b"parameter classes" in err()
    assert lib.anm_model_set_classes(h, 2, None) != 0 and b"affine" in err() and b"parameter classes" in err()
    flags = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.anm_model_bind_state_same(h, flags.data_ptr()) != 0 and b"affine" in err()
    m, keep = c_map(env)
    plain = make_env("anm6", "radial", "series", 64, 1)
    ph = plain.simulator._handle
    assert lib.anm_model_bind_view(ph, C.byref(view)) == 0
    assert lib.anm_model_set_io_map(ph, C.byref(m)) != 0 and b"batch view" in err()
    assert lib.anm_model_bind_view(ph, None) == 0
    with_classes = make_env("anm6", "radial", "series", 64, 1, variants=[networks.anm6_network()], env_variant=np.zeros(64, dtype=np.int32))
    assert lib.anm_model_set_io_map(with_classes.simulator._handle, C.byref(m)) != 0 and b"parameter classes" in err()
    easy = ANM6EasyVec(num_envs=64, device=DEV, seed=1)        # (the fast path binds the flags)
    assert easy._state_same is not None
    assert lib.anm_model_set_io_map(easy.simulator._handle, C.byref(m)) != 0 and b"anm_model_bind_state_same" in err()
    # `full` without a list gathered in the kernel
    args = list(env._step_args)
    args[9] = sim.full.data_ptr()
    rc = lib.anm_step_f64(h, env.num_envs, u.data_ptr(), None, None, *args, 0, env.rng_seed, env.env_offset,
                          env._reset_count_ptr, env._aux_index_ptr, env._ws_ref, env._opts_ref, None)
    assert rc != 0 and b"anm_gather_obs_f64" in err() and b"affine" in err()
    # the mapped model steps on as its twin does, the others as plain models
    u = unit_actions(env, gen)
    o, r, _, _, _ = env.step(u)
    o2, r2, _, _, _ = twin.step(u)
    assert same_bits(o, o2) and same_bits(r, r2) and torch.equal(env.state, twin.state)
    for other in (plain, with_classes, easy):
        other.check_actions = False
        other.reset(options={"sampler": "device"})
        o, r, _, _, _ = other.step(decode(env, u)[: other.num_envs])
        assert o.dtype == F64 and bool(torch.isfinite(o).all())
    # the public classes
    with pytest.raises(errors.EnvInitializationError, match="parameter classes"):
        make_env("anm6", "radial", "series", 64, 1, variants=[networks.anm6_network()], env_variant=np.zeros(64, dtype=np.int32), **FULL_MAP)
    with pytest.raises(errors.EnvInitializationError, match="fuse_observation=False"):
        make_env("anm6", "thread", "series", 64, 1, observation=LIST_OBS, fuse_observation=False, obs_map="box")
    with pytest.raises(errors.EnvInitializationError, match="track_full"):
        make_env("anm6", "thread", "series", 64, 1, track_full=True, reward_scale=0.5)
    with pytest.raises(errors.EnvInitializationError, match="callable"):
        make_env("anm6", "thread", "series", 64, 1, observation=lambda s: s, obs_map="box")
    with pytest.raises(errors.ArgsError, match="obs_map"):
        make_env("anm6", "thread", "series", 64, 1, obs_map=(np.ones(3), np.zeros(3)))
    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv([dict(network=networks.anm6_network(), series=anm6easy_series())], [0, 0, 0, 0], device=DEV, action_map="unit")


def test_null_map_returns_the_model_to_plain_stepping():
    kw = dict(autoreset=True, max_episode_steps=3, episode_stats=True)
    for net, impl in (("anm6", "thread"), ("case30", "radial")):
        a = make_env(net, impl, "series", 70, 3, **FULL_MAP, **kw)
        b = make_env(net, impl, "series", 70, 3, **kw)
        assert a.simulator.backend.lib.anm_model_set_io_map(a.simulator._handle, None) == 0
        device_reset(a)
        device_reset(b)
        gen = torch.Generator(device=DEV).manual_seed(8)
        lo, hi = (torch.as_tensor(x, device=DEV) for x in (b.action_space.low, b.action_space.high))
        for t in range(5):
            act = (lo + (hi - lo) * torch.rand((70, lo.numel()), generator=gen, dtype=F64, device=DEV)).contiguous()
            oa, ra, _, _, _ = a.step(act)
            ob, rb, _, _, _ = b.step(act)
            assert same_bits(oa, ob) and same_bits(ra, rb), "%s %s step %d" % (net, impl, t)
            xa, xb = f64_outputs(a), f64_outputs(b)
            for k in F64_OUT:
                assert torch.equal(xa[k], xb[k]), "%s %s step %d: %s" % (net, impl, t, k)


# ---- 9. the NumPy adapter ---------------------------------------------------------------------------------------------------------------
def test_numpy_vector_env():
    E_, T = 64, 3
    kw = dict(num_envs=E_, seed=6, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T, episode_stats=True)
    inner = ANM6EasyVec(io_dtype=F32, **FULL_MAP, **kw)
    env, ref = NumpyVectorEnv(inner), NumpyVectorEnv(ANM6EasyVec(**kw))
    assert env.single_action_space.dtype == np.float32 and env.single_observation_space.dtype == np.float32
    assert np.all(env.action_space.low == -1) and np.all(env.action_space.high == 1)
    assert np.array_equal(env.raw_action_space.low, inner.raw_action_space.low) and env.raw_action_space.dtype == np.float32
    assert env.observation_space is inner.observation_space
    sc, bi = inner.io_map["obs"]
    o, _ = env.reset(seed=6)
    orf, _ = ref.reset(seed=6)
    assert o.dtype == np.float32 and np.array_equal(o.view(np.int32), io_affine.map_obs(orf, sc, bi).astype(np.float32).view(np.int32))
    r_np = np.random.default_rng(0)
    for t in range(T + 2):
        u = (2 * r_np.random((E_, 6)) - 1).astype(np.float32)
        o, r, term, trunc, info = env.step(u)
        orf, rrf, termf, truncf, inforf = ref.step(io_affine.map_action(u, *inner.io_map["action"]))
        assert o.dtype == np.float32 and r.dtype == np.float32
        assert np.array_equal(o.view(np.int32), io_affine.map_obs(orf, sc, bi).astype(np.float32).view(np.int32))
        assert np.array_equal(r.view(np.int32), io_affine.map_reward(rrf, 1 / 64).astype(np.float32).view(np.int32))
        assert np.array_equal(term, termf) and np.array_equal(trunc, truncf)
        for k in ("r", "d"):                                     # the statistics accumulate the raw float64 reward
            assert info["episode"][k].dtype == np.float64 and np.array_equal(info["episode"][k], inforf["episode"][k])
    with pytest.raises(AssertionError, match="invalid"):
        env.step(np.full((E_, 6), 1.5))
