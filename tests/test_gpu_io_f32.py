"""GPU tier: float32 action, observation and reward I/O in the step kernels (``BatchedANMEnv(io_dtype=torch.float32)``,
``anm_model_set_io``; the specification is gym_anm_amd/io_dtype.py).  Every comparison is exact -- float32 tensors through
``.view(torch.int32)``, so that -0 and NaN count; no tolerance anywhere.
  1. the float32 mode is the float64 mode plus one rounding;  2. terminal-on-entry rows;  3. tails;  4. the fused list
  observation;  5. the two-launch step;  6. one launch, nothing allocated, capturable;  7. masked reset();  8. refusals;
  9. the NumPy adapter."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.envs import ANM6EasyVec, NumpyVectorEnv
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.995
F32 = torch.float32

NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0)}
FAMILIES = [("anm6", "thread"), ("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial"), ("case30", "mesh")]
CASES = [(n, i, m) for n, i in FAMILIES for m in ("series", "uniform")]
F64_OUT = ("state", "e_loss", "penalty", "terminated", "truncated", "soc", "timestep", "reset_count", "nr_iters")
STATS = ("episode_return", "episode_discounted_return", "last_episode_return", "last_episode_discounted_return",
         "last_episode_length", "episodes_done")
LIST_OBS = [("bus_v_magn", "all", "pu"), ("branch_s", "all", "MVA"), ("des_soc", "all", "MWh"), ("aux", "all")]


@functools.lru_cache(maxsize=None)
def series_of(net):
    """ANM6Easy's table for the 6-bus network; for the feeder a fixed table of seeded draws, every unit uniform over its range"""
    if net == "anm6":
        return anm6easy_series()
    from gym_anm_amd.model import NetworkModel

    lo, hi = rng.default_exo_bounds(NetworkModel(NETS[net](), 0.25, 100))
    u = np.random.default_rng(2024).random((len(lo), 512))
    return np.ascontiguousarray(lo[:, None] + (hi - lo)[:, None] * u)


def make_env(net, impl, mode, E_, seed, observation="state", **kw):
    if mode == "series":
        ser = series_of(net)
        kw.update(series=ser, aux_bounds=np.array(((0, ser.shape[1] - 1),)))
    else:
        kw.update(exogenous="uniform", aux_bounds=np.array(((0, 1000),)))
    env = BatchedANMEnv(NETS[net](), observation, 1, 0.25, GAMMA, 100, costs_clipping=(1, 100), seed=seed, num_envs=E_,
                        device=DEV, tol=1e-6, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def make_pair(net, impl, mode, E_, seed, **kw):
    """A: the float32 mode.  B: the float64 mode, otherwise the same environment."""
    return make_env(net, impl, mode, E_, seed, io_dtype=F32, **kw), make_env(net, impl, mode, E_, seed, **kw)


def device_reset(env, mask=None):
    return env.reset(options={"sampler": "device", "mask": mask})


def bits(x):
    assert x.dtype == F32
    return x.contiguous().view(torch.int32)


def actions32(env, gen):
    """float32 actions uniform over the float32 Box of a float32-mode environment (clamped: the products round)"""
    lo = torch.as_tensor(env.action_space.low, device=DEV)
    hi = torch.as_tensor(env.action_space.high, device=DEV)
    assert lo.dtype == F32 and hi.dtype == F32
    u = torch.rand((env.num_envs, lo.numel()), generator=gen, dtype=torch.float64, device=DEV)
    return torch.minimum(torch.maximum((lo.double() + (hi.double() - lo.double()) * u).float(), lo), hi).contiguous()


def f64_outputs(env):
    return dict(state=env.state, e_loss=env.e_loss, penalty=env.penalty, terminated=env.terminated, truncated=env.truncated,
                soc=env.simulator.soc, timestep=env.timestep, reset_count=env._reset_count, nr_iters=env.simulator.nr_iters)


def compare(a, b, oa, ob, where, stats=False, ra=None, rb=None):
    """A against B: every float64 output equal, obs and reward of A the one rounding of B's, dtypes, obs inside the Box"""
    xa, xb = f64_outputs(a), f64_outputs(b)
    for k in F64_OUT:
        assert xa[k].dtype == xb[k].dtype and torch.equal(xa[k], xb[k]), "%s: %s differs" % (where, k)
    if stats:
        for k in STATS:
            assert torch.equal(getattr(a, k), getattr(b, k)), "%s: %s differs" % (where, k)
    assert oa.dtype == F32 and ob.dtype == torch.float64 and oa.shape == ob.shape
    assert a.state.dtype == torch.float64 and a.e_loss.dtype == torch.float64 and a.penalty.dtype == torch.float64
    assert torch.equal(bits(oa), bits(ob.float())), "%s: obs is not the float64 mode's, rounded once" % where
    ra = a.reward if ra is None else ra
    rb = b.reward if rb is None else rb
    assert ra.dtype == F32 and rb.dtype == torch.float64
    assert torch.equal(bits(ra), bits(rb.float())), "%s: reward is not the float64 mode's, rounded once" % where
    lo = torch.as_tensor(a.observation_space.low, device=DEV)
    hi = torch.as_tensor(a.observation_space.high, device=DEV)
    assert a.observation_space.dtype == np.float32 and lo.dtype == F32
    # (the zero row of a terminated environment is no clip() output: the reference writes it whatever the Box says, and a list
    # with the slack bus in it -- |V| in [1, 1] -- has it outside in the float64 mode too; it is compared bit for bit above)
    inside = ((oa >= lo) & (oa <= hi)).all(dim=1)
    assert bool((inside | a.terminated).all()), "%s: obs outside the float32 Box" % where


def rollout(a, b, n_steps, seed, where, stats=False, before_step=None):
    """device reset of both, then n_steps with the same float32 actions (B: widened); compared after the reset and every step.
    Returns (collapses, autoresets) seen in A."""
    oa, _ = device_reset(a)
    ob, _ = device_reset(b)
    compare(a, b, oa, ob, where + " reset", stats)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n_collapse = n_reset = 0
    for t in range(n_steps):
        a32 = actions32(a, gen)
        if before_step is not None:
            before_step(t, a, b)
        ts_in = a.timestep.clone()
        oa, ra, ta, tra, _ = a.step(a32)
        ob, rb, tb, trb, _ = b.step(a32.double())
        assert ra is a.reward and ta.dtype == torch.bool
        compare(a, b, oa, ob, "%s step %d" % (where, t), stats, ra, rb)
        n_collapse += int((ta & (a.timestep > 0) & (a.timestep != ts_in)).sum())
        n_reset += int(((a.timestep == 0) & (ts_in > 0)).sum())
    return n_collapse, n_reset


# ---- 1. the float32 mode is the float64 mode plus one rounding ---------------------------------------------------------------
E1 = 4133   # 64 * 64 + 37: a partial last wavefront and a partial last lane group


@pytest.mark.parametrize("net,impl,mode", CASES)
def test_float32_mode_is_the_float64_mode_plus_one_rounding(net, impl, mode):
    kw = dict(autoreset=True, env_offset=(1 << 32) - 300, max_episode_steps=5, episode_stats=True)
    a, b = make_pair(net, impl, mode, E1, 2718, **kw)
    assert a.io_dtype == F32 and b.io_dtype == torch.float64 and a.action_space.dtype == np.float32
    n_collapse, n_reset = rollout(a, b, 14, 17, "%s %s %s" % (net, impl, mode), stats=True)
    print("%s %s %s: %d collapses, %d in-kernel resets" % (net, impl, mode, n_collapse, n_reset))
    assert n_reset >= E1      # the limit of 5 sends every environment through the autoreset path (by its sixth call at the latest)
    assert int(a.episodes_done.min()) >= 1
    if net == "anm6" and mode == "series":
        assert n_collapse >= 1                                 # (~0.4 % of random-action steps collapse: of the order of 200 here)


# ---- 2. terminal-on-entry rows, made deterministic ----------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl,mode", CASES)
def test_terminal_on_entry_rows(net, impl, mode):
    """(The rows are marked before the first step after reset(): there `state` is the reset's own row in both modes.  Marked in
    mid-episode, the float64 mode's `state` of such a row would be assembled from the zeroed obs row -- anm_model_bind_state_same
    -- which no real episode produces: a collapse zeroes both rows.)"""
    a, b = make_pair(net, impl, mode, 203, 5)

    def mark(t, a, b):
        if t == 0:
            for env in (a, b):
                env._term_u8[::7] = 1

    rollout(a, b, 3, 3, "terminal %s %s %s" % (net, impl, mode), before_step=mark)
    assert bool(a.terminated[::7].all())
    obs = a._state_obs
    assert not bool(bits(obs[::7]).any()) and not bool(bits(a.reward[::7]).any())     # absorbing rows: +0, not -0


# ---- 3. tails ------------------------------------------------------------------------------------------------------------------
TAILS = [("anm6", "thread", E_) for E_ in (1, 63, 65, 129)] + [(n, i, E_) for n, i in (("anm6", "radial"), ("case30", "mesh"))
                                                               for E_ in (1, 9)]


@pytest.mark.parametrize("net,impl,E_", TAILS)
def test_tails(net, impl, E_):
    a, b = make_pair(net, impl, "series", E_, 11, autoreset=True, max_episode_steps=2, episode_stats=True)
    rollout(a, b, 3, 5, "tail %s %s %d" % (net, impl, E_), stats=True)


# ---- 4. the list-form observation gathered in the kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial"), ("case30", "mesh")])
def test_fused_list_observation(net, impl):
    a, b = make_pair(net, impl, "series", 203, 8, observation=LIST_OBS, autoreset=True, max_episode_steps=3)
    assert a._obs_fused and b._obs_fused and a._obs_buf.dtype == F32
    assert a.observation_space.shape == b.observation_space.shape and a.observation_space.shape[0] != a.state_N
    _, n_reset = rollout(a, b, 7, 9, "list %s %s" % (net, impl))
    assert n_reset >= 203                                       # rows written by the in-kernel autoreset are among those compared
    # zero rows of terminated environments (no autoreset): all bits zero
    a, b = make_pair(net, impl, "series", 70, 8, observation=LIST_OBS)

    def mark(t, a, b):
        for env in (a, b):
            env._term_u8[::5] = 1

    rollout(a, b, 2, 9, "list terminal %s %s" % (net, impl), before_step=mark)
    assert not bool(bits(a._obs_buf[::5]).any())


# ---- 5. the two-launch step -----------------------------------------------------------------------------------------------------
def test_two_launch_step():
    kw = dict(num_envs=E1, seed=31, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=5, episode_stats=True)
    two = ANM6EasyVec(io_dtype=F32, straggler_after=6, **kw)
    one = ANM6EasyVec(io_dtype=F32, straggler_after=None, **kw)
    ref = ANM6EasyVec(straggler_after=6, **kw)
    assert two._ws is not None and one._ws is None and ref._ws is not None
    for env in (two, one, ref):
        env.check_actions = False
        env.reset(seed=31)
    gen = torch.Generator(device=DEV).manual_seed(6)
    for t in range(10):
        a32 = actions32(two, gen)
        o2, r2, _, _, _ = two.step(a32)
        o1, r1, _, _, _ = one.step(a32)
        orf, rrf, _, _, _ = ref.step(a32.double())
        x2, x1 = f64_outputs(two), f64_outputs(one)
        for k in F64_OUT:
            assert torch.equal(x2[k], x1[k]), "step %d: %s (two launches against one)" % (t, k)
        for k in STATS:
            assert torch.equal(getattr(two, k), getattr(one, k)), "step %d: %s" % (t, k)
        assert torch.equal(bits(o2), bits(o1)) and torch.equal(bits(r2), bits(r1))
        compare(two, ref, o2, orf, "two-launch step %d" % t, True, r2, rrf)
    assert int(two.simulator.nr_iters.max()) > 6                # some solves did go through the straggler launches


# ---- 6. one launch, nothing allocated, capturable -------------------------------------------------------------------------------
def test_nothing_allocated_and_capturable():
    E_, SEED = 1024, 21
    kw = dict(num_envs=E_, seed=SEED, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=4, episode_stats=True, io_dtype=F32)
    env, twin = ANM6EasyVec(**kw), ANM6EasyVec(**kw)
    for e in (env, twin):
        e.check_actions = False
        e.reset(seed=SEED)
    gen = torch.Generator(device=DEV).manual_seed(2)
    acts = [actions32(env, gen) for _ in range(10)]
    buf = acts[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # the very first step after reset(): one stream, nothing allocated, no synchronisation
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
        assert torch.equal(bits(env._state_obs), bits(o2)) and torch.equal(bits(env.reward), bits(r2)), "replay %d" % t
    assert int(env.episodes_done.min()) >= 1
    # eager steps fed from a preallocated float32 tensor allocate nothing: the tensor goes to the kernel as it is
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for a in acts[:5]:
        buf.copy_(a)
        o, r, _, _, _ = twin.step(buf)
        assert torch.cuda.memory_allocated() == m0
    assert o is twin._state_obs and r is twin.reward and o.dtype == F32 and r.dtype == F32


# ---- 7. masked reset() ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl,observation", [("anm6", "thread", "state"), ("anm6", "radial", "state"), ("case30", "mesh", "state"),
                                                  ("anm6", "thread", LIST_OBS), ("case30", "radial", LIST_OBS)])
def test_masked_reset(net, impl, observation):
    E_ = 131
    a, b = make_pair(net, impl, "series", E_, 9, observation=observation)
    where = "masked reset %s %s" % (net, impl)
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
    gen = torch.Generator(device=DEV).manual_seed(12)
    a32 = actions32(a, gen)
    oa, ra, _, _, _ = a.step(a32)
    ob, rb, _, _, _ = b.step(a32.double())
    compare(a, b, oa, ob, where + " (step after)", False, ra, rb)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_what_the_mode_refuses():
    env = make_env("anm6", "radial", "series", 64, 1, io_dtype=F32)
    device_reset(env)
    a32 = actions32(env, torch.Generator(device=DEV).manual_seed(1))
    env.step(a32)
    sim = env.simulator
    lib, h = sim.backend.lib, sim._handle
    err = lib.anm_last_error
    # an unknown value
    assert lib.anm_model_set_io(h, 7) != 0 and b"unknown value" in err()
    # a batch view, from both sides
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(h, C.byref(view)) != 0 and b"float32" in err() and b"batch view" in err()
    plain = make_env("anm6", "radial", "series", 64, 1)
    ph = plain.simulator._handle
    assert lib.anm_model_bind_view(ph, C.byref(view)) == 0
    assert lib.anm_model_set_io(ph, _lib.IO_F32) != 0 and b"batch view" in err()
    assert lib.anm_model_bind_view(ph, None) == 0
    # parameter classes, from both sides
    cls = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert lib.anm_model_bind_env_classes(h, cls.data_ptr(), 64) != 0 and b"float32" in err() and b"parameter classes" in err()
    assert lib.anm_model_set_classes(h, 2, None) != 0 and b"float32" in err() and b"parameter classes" in err()
    with_classes = make_env("anm6", "radial", "series", 64, 1, variants=[networks.anm6_network()],
                            env_variant=np.zeros(64, dtype=np.int32))
    assert lib.anm_model_set_io(with_classes.simulator._handle, _lib.IO_F32) != 0 and b"parameter classes" in err()
    # anm_model_bind_state_same, from both sides
    flags = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.anm_model_bind_state_same(h, flags.data_ptr()) != 0 and b"float32" in err()
    easy = ANM6EasyVec(num_envs=64, device=DEV, seed=1)        # (the fast path binds the flags)
    assert easy._state_same is not None
    assert lib.anm_model_set_io(easy.simulator._handle, _lib.IO_F32) != 0 and b"anm_model_bind_state_same" in err()
    # `full` without a list gathered in the kernel: the unfused anm_gather_obs_f64 path
    args = list(env._step_args)
    args[9] = sim.full.data_ptr()
    rc = lib.anm_step_f64(h, env.num_envs, a32.data_ptr(), None, None, *args, 0, env.rng_seed, env.env_offset,
                          env._reset_count_ptr, env._aux_index_ptr, env._ws_ref, env._opts_ref, None)
    assert rc != 0 and b"anm_gather_obs_f64" in err() and b"float32" in err()
    # the models are as they were: the float32 one steps in float32, the others in float64
    o, r, _, _, _ = env.step(a32)
    assert o.dtype == F32 and r.dtype == F32
    for other in (plain, with_classes, easy):
        other.check_actions = False
        other.reset(options={"sampler": "device"})
        o, r, _, _, _ = other.step(a32.double()[: other.num_envs])
        assert o.dtype == torch.float64 and r.dtype == torch.float64 and bool(torch.isfinite(o).all())
    # back to float64 and on again is allowed
    assert lib.anm_model_set_io(h, _lib.IO_F64) == 0 and lib.anm_model_set_io(h, _lib.IO_F32) == 0
    # the public classes
    with pytest.raises(errors.ArgsError, match="io_dtype"):
        make_env("anm6", "radial", "series", 4, 1, io_dtype=torch.float16)
    with pytest.raises(errors.EnvInitializationError, match="parameter classes"):
        make_env("anm6", "radial", "series", 64, 1, io_dtype=F32, variants=[networks.anm6_network()],
                 env_variant=np.zeros(64, dtype=np.int32))
    with pytest.raises(errors.EnvInitializationError, match="fuse_observation=False"):
        make_env("anm6", "thread", "series", 64, 1, io_dtype=F32, observation=LIST_OBS, fuse_observation=False)
    with pytest.raises(errors.EnvInitializationError, match="track_full"):
        make_env("anm6", "thread", "series", 64, 1, io_dtype=F32, track_full=True)
    from gym_anm_amd.envs import MixedBatchedANMEnv

    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv([dict(network=networks.anm6_network(), series=anm6easy_series())], [0, 0, 0, 0], device=DEV, io_dtype=F32)


def test_non_float32_actions_are_converted_and_checked():
    env = ANM6EasyVec(num_envs=8, device=DEV, seed=2, io_dtype=F32)
    twin = ANM6EasyVec(num_envs=8, device=DEV, seed=2, io_dtype=F32)
    for e in (env, twin):
        e.reset(seed=2)
    a32 = actions32(env, torch.Generator(device=DEV).manual_seed(3))
    o1, r1, _, _, _ = env.step(a32.double().cpu().numpy())      # any other dtype is converted to float32
    o2, r2, _, _, _ = twin.step(a32)
    assert torch.equal(bits(o1), bits(o2)) and torch.equal(bits(r1), bits(r2)) and torch.equal(env.state, twin.state)
    hi = torch.as_tensor(env.action_space.high, device=DEV)
    bad = a32.clone()
    bad[3, 0] = torch.nextafter(hi[0], torch.tensor(float("inf"), device=DEV))
    with pytest.raises(AssertionError, match="invalid"):
        env.step(bad)                                           # check_actions compares in float32 against the inward bounds


# ---- 9. the NumPy adapter -----------------------------------------------------------------------------------------------------------
def test_numpy_vector_env():
    E_, T = 64, 3
    kw = dict(num_envs=E_, seed=6, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T, episode_stats=True)
    env = NumpyVectorEnv(ANM6EasyVec(io_dtype=F32, **kw))
    ref = NumpyVectorEnv(ANM6EasyVec(**kw))
    assert env.single_action_space.dtype == np.float32 and env.single_observation_space.dtype == np.float32
    assert env.action_space.low.dtype == np.float32 and env.observation_space.high.dtype == np.float32
    o, _ = env.reset(seed=6)
    orf, _ = ref.reset(seed=6)
    assert o.dtype == np.float32 and np.array_equal(o.view(np.int32), orf.astype(np.float32).view(np.int32))
    r_np = np.random.default_rng(0)
    lo, hi = env.single_action_space.low, env.single_action_space.high
    n_seen = 0
    for t in range(2 * T + 2):
        act = np.clip((lo + (hi - lo) * r_np.random((E_, len(lo)))).astype(np.float32), lo, hi)
        o, r, term, trunc, info = env.step(act.astype(np.float64))   # (the adapter takes the space's dtype for the actions)
        orf, rrf, termf, truncf, inforf = ref.step(act.astype(np.float64))
        assert o.dtype == np.float32 and r.dtype == np.float32 and term.dtype == bool and trunc.dtype == bool
        assert np.array_equal(o.view(np.int32), orf.astype(np.float32).view(np.int32))
        assert np.array_equal(r.view(np.int32), rrf.astype(np.float32).view(np.int32))
        assert np.array_equal(term, termf) and np.array_equal(trunc, truncf) and np.array_equal(info["_episode"], inforf["_episode"])
        for k in ("r", "d"):                                     # the statistics stay float64 and unchanged
            assert info["episode"][k].dtype == np.float64 and np.array_equal(info["episode"][k], inforf["episode"][k])
        assert np.array_equal(info["episode"]["l"], inforf["episode"]["l"])
        n_seen += int(info["_episode"].sum())
    assert n_seen >= E_
    with pytest.raises(AssertionError, match="invalid"):
        env.step(np.broadcast_to(hi.astype(np.float64) + 1.0, (E_, len(lo))))
