"""GPU tier: running observation / return normalisation kept on the device (``BatchedANMEnv(obs_norm="running",
reward_norm="running")``, ``anm_model_io_norm_update``; the specification is gym_anm_amd/io_norm.py).  Every comparison is
exact: float64 through ``int64`` views, float32 through ``int32`` views; no tolerance anywhere.
  1. the update alone, through the C ABI, on synthetic tensors;  2. through the environment, against a plain twin and the
  specification;  3. each part alone;  4. norm_training = False;  5. checkpoints;  6. masked reset();  7. HIP graph, nothing
  allocated;  8. the same batch twice;  9. refusals of the C ABI."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, io_affine, io_norm, networks, rng
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

from test_gpu_exo_noise import task_of
from test_gpu_io_f32 import F64_OUT, device_reset, f64_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.995
F32, F64 = torch.float32, torch.float64
BOTH = dict(obs_norm="running", reward_norm="running")
NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0),
        "mesh20": lambda: networks.synthetic_meshed_network(20, 3, 6)}
LIST3 = [("bus_v_magn", [1], "pu"), ("des_soc", "all", "MWh"), ("aux", "all")]


@functools.lru_cache(maxsize=None)
def noise_task(net):
    if net != "mesh20":
        return task_of(net)
    lo, hi = rng.default_exo_bounds(NetworkModel(NETS[net](), 0.25, 100))
    span = lo + hi
    ser = np.ascontiguousarray(span[:, None] * np.array([0.3, 0.45, 0.6, 0.5, 0.35])[None, :])
    return ser, np.ascontiguousarray(np.broadcast_to(0.2 * np.abs(span)[:, None], ser.shape)), lo, hi


def make_env(net, impl, mode, E_, seed, observation="state", **kw):
    if mode == "noise":
        ser, amp, low, high = noise_task(net)
        kw.update(exogenous="series_noise", series=ser, exo_noise=amp, exo_low=low, exo_high=high,
                  aux_bounds=np.array(((0, ser.shape[1] - 1),)))
    else:
        assert mode == "uniform"
        kw.update(exogenous="uniform", aux_bounds=np.array(((0, 1000),)))
    env = BatchedANMEnv(NETS[net](), observation, 1, 0.25, GAMMA, 100, costs_clipping=(1, 100), seed=seed, num_envs=E_,
                        device=DEV, tol=1e-6, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y))


def device_tables(env):
    """(scale, bias, reward_scale) as the device holds them"""
    D = env.observation_N
    o, r = env.obs_rms, env.ret_rms
    sc = o.scale.cpu().numpy() if o is not None else np.ones(D)
    bi = o.bias.cpu().numpy() if o is not None else np.full(D, -0.0)
    return sc, bi, (float(r.scale) if r is not None else 1.0)


def assert_state(env, st, tabs, where):
    d = env.norm_state()
    for k in ("cnt", "rcnt", "rmean", "rvar"):
        assert same(np.float64(d[k]), np.float64(st[k])), "%s: %s %r != %r" % (where, k, d[k], st[k])
    for k in ("mean", "var", "G", "t_seen"):
        assert same(d[k], np.asarray(st[k])), "%s: %s differs" % (where, k)
    assert d["n_updates"] == st["n_updates"] and d["n_skipped"] == st["n_skipped"], (where, d["n_updates"], d["n_skipped"], st["n_skipped"])
    sc, bi, rs = device_tables(env)
    assert same(sc, tabs[0]) and same(bi, tabs[1]) and same(np.float64(rs), np.float64(tabs[2])), "%s: the tables differ" % where


def start_tables(env):
    D = env.observation_N
    sc, bi = io_norm.tables(np.zeros(D), np.ones(D), env.norm_eps) if env._obs_norm else (np.ones(D), np.full(D, -0.0))
    return sc, bi, io_norm.reward_scale(1.0, env.norm_eps) if env._reward_norm else 1.0


# ---- 1. the update alone, through the C ABI, on synthetic tensors -------------------------------------------------------------------
def synthetic(E_, D, dtype, flags, u, seen, gen, nan_at=None):
    big = 1e150 if dtype == F64 else 1e30
    y = torch.randn((E_, D), generator=gen, dtype=F64) * (10.0 ** torch.randint(-3, 4, (D,), generator=gen).double()) + u
    y[:, 1] = 2.5                       # a constant column
    y[:, 2] = -0.0                      # all -0.0
    if D > 3:
        y[:, 3] = big * (1 + 0.25 * torch.rand(E_, generator=gen, dtype=F64))
    if nan_at is not None:
        y[nan_at, 0] = float("nan")
    term = {"none": torch.zeros(E_), "some": (torch.rand(E_, generator=gen) < 0.3).float(), "all": torch.ones(E_)}[flags].to(torch.uint8)
    if nan_at is not None:
        term[nan_at] = 0
    trunc = (torch.rand(E_, generator=gen) < 0.2).to(torch.uint8)
    pick = torch.randint(0, 4, (E_,), generator=gen)     # 0: nothing happened, 1: an autoreset, else: a step
    ts = torch.where(pick == 0, seen, torch.where(pick == 1, torch.zeros_like(seen), seen + 1)).to(torch.int32)
    r = torch.randn(E_, generator=gen, dtype=F64) * 3 - 1
    return y.to(dtype), r.to(dtype), term, trunc, ts


def call_update(env, y, r, term, trunc, ts):
    sim = env.simulator
    rc = sim.backend.lib.anm_model_io_norm_update(sim._handle, env.num_envs, y.data_ptr(), r.data_ptr(), term.data_ptr(),
                                                  trunc.data_ptr(), ts.data_ptr(), env._norm_ref,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    sim.backend.check(rc, "anm_model_io_norm_update")


# (1025: four groups of 256 rows and one row; 3001: 12 slabs padded to 64; 263 169: above 262 144 environments a group takes
# 1024 rows -- the other instantiation of k_norm_partial -- 257 full groups and one row, 258 slabs in aligned runs of 8)
UPDATE_CASES = [(e, d, t) for e in (1, 63, 65, 1025, 3001) for d in (18, 3) for t in (F64, F32)] + [(263169, 3, F32)]


@pytest.mark.parametrize("E_,D,dtype", UPDATE_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_update_alone_against_the_specification(E_, D, dtype):
    env = make_env("anm6", "thread", "uniform", E_, 5, observation="state" if D == 18 else LIST3, io_dtype=dtype, **BOTH)
    assert env.observation_N == D and env._norm_slabs.numel() == io_norm.slab_doubles(E_, D)
    first = env.norm_state()
    for flags in ("none", "some", "all", "nan") if E_ < 100000 else ("some",):
        env.load_norm_state(first)
        st = io_norm.initial_state(E_, D)
        tabs = start_tables(env)
        assert_state(env, st, tabs, "start")
        gen = torch.Generator().manual_seed(1000 * E_ + D)
        for u in range(3):
            nan_at = E_ // 2 if flags == "nan" and u == 1 else None
            y, r, term, trunc, ts = synthetic(E_, D, dtype, "some" if flags == "nan" else flags, u, torch.as_tensor(st["t_seen"]), gen, nan_at)
            before = {k: np.array(st[k], copy=True) for k in ("cnt", "mean", "var")}
            tabs = io_norm.update(st, y.numpy(), r.numpy(), term.numpy(), trunc.numpy(), ts.numpy(), tabs[:2], tabs[2], GAMMA, env.norm_eps)
            call_update(env, *(t.to(DEV) for t in (y, r, term, trunc, ts)))
            where = "E=%d D=%d %s %s update %d" % (E_, D, dtype, flags, u)
            assert_state(env, st, tabs, where)
            if flags == "all":          # n = 0: the observation part unchanged bit for bit
                assert all(same(before[k], np.asarray(st[k])) for k in before) and st["cnt"] == io_norm.COUNT0
            if nan_at is not None:      # the column with the counted NaN is skipped, the others update
                assert same(before["mean"][0], st["mean"][0]) and same(before["var"][0], st["var"][0])
                assert st["mean"][1] != before["mean"][1] and st["cnt"] > before["cnt"]
        # (D = 18: the 1e150 column overflows vo = vy / s^2 from the second update on and is skipped too -- by both sides)
        if flags == "nan":
            assert st["n_updates"] == 3 and (st["n_skipped"] == 1 if D == 3 else st["n_skipped"] >= 1)
        elif flags == "none":
            assert (st["n_skipped"] == 0 or D > 3) and st["cnt"] == ((io_norm.COUNT0 + E_) + E_) + E_
            assert st["mean"][2] == 0.0 and not np.signbit(st["mean"][2])
            if E_ > 1:
                assert st["rcnt"] > io_norm.COUNT0 and (st["var"] != 1.0).all() and np.isfinite(st["var"]).all()


# ---- 2. through the environment ----------------------------------------------------------------------------------------------------
def box_actions(env, gen):
    lo, hi = (torch.as_tensor(x, device=DEV) for x in (env.action_space.low, env.action_space.high))
    u = lo.double() + (hi.double() - lo.double()) * torch.rand((env.num_envs, lo.numel()), generator=gen, dtype=F64, device=DEV)
    return torch.minimum(torch.maximum(u.to(env.io_dtype), lo), hi).contiguous()


def expect_io(a, ob, rb, tabs):
    o = torch.as_tensor(io_affine.map_obs(ob.cpu().numpy(), tabs[0], tabs[1]), dtype=F64, device=DEV).to(a.io_dtype)
    r = torch.as_tensor(io_affine.map_reward(rb.cpu().numpy(), tabs[2]), dtype=F64, device=DEV).to(a.io_dtype)
    return o, r


def tsame(x, y):
    return same(x.cpu().numpy(), y.cpu().numpy())


def rollout(a, b, n_steps, seed, where, st=None, tabs=None, check_state=True):
    """A normalised, B plain: raw outputs equal, A's obs / reward the maps of B's under the tables of the specification, which
    follows A's stored rows; -> (st, tabs)"""
    oa, _ = device_reset(a)
    ob, _ = device_reset(b)
    st = io_norm.initial_state(a.num_envs, a.observation_N) if st is None else st
    tabs = start_tables(a) if tabs is None else tabs
    assert tsame(oa, expect_io(a, ob, b.reward, tabs)[0]), where + " reset: obs"
    st["G"][:], st["t_seen"][:] = 0.0, 0
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n_reset = 0
    for t in range(n_steps):
        u = box_actions(a, gen)
        ts_in = a.timestep.clone()
        oa, ra, _, _, _ = a.step(u)
        ob, rb, _, _, _ = b.step(u.double())
        w = "%s step %d" % (where, t)
        xa, xb = f64_outputs(a), f64_outputs(b)
        for k in F64_OUT:
            assert torch.equal(xa[k], xb[k]), "%s: %s differs" % (w, k)
        eo, er = expect_io(a, ob, rb, tabs)
        assert oa.dtype == a.io_dtype and tsame(oa, eo), w + ": obs is not map_obs of the plain mode's under the tables through t-1"
        assert tsame(ra, er), w + ": reward"
        if a.norm_training:
            tabs = io_norm.update(st, oa.cpu().numpy(), ra.cpu().numpy(), a.terminated.cpu().numpy(), a.truncated.cpu().numpy(),
                                  a.timestep.cpu().numpy(), tabs[:2], tabs[2], GAMMA, a.norm_eps, a._obs_norm, a._reward_norm)
        if check_state:
            assert_state(a, st, tabs, w)
        n_reset += int(((a.timestep == 0) & (ts_in > 0)).sum())
    return st, tabs, n_reset


ROLL = dict(autoreset=True, max_episode_steps=3)
PAIRS = [("anm6", "thread", "state", 65, F64), ("anm6", "thread", "state", 65, F32), ("anm6", "thread", "state", 1025, F64),
         ("anm6", "thread", "state", 1025, F32), ("anm6", "thread", LIST3, 65, F64), ("case30", "radial", "state", 9, F64),
         ("case30", "radial", "state", 41, F64), ("mesh20", "mesh", "state", 9, F64)]


@pytest.mark.parametrize("mode", ["uniform", "noise"])
@pytest.mark.parametrize("net,impl,observation,E_,dtype", PAIRS, ids=lambda v: "list3" if isinstance(v, list) else str(v).replace("torch.", ""))
def test_normalised_environment_against_plain_twin_and_specification(net, impl, observation, E_, dtype, mode):
    a = make_env(net, impl, mode, E_, 2718, observation=observation, io_dtype=dtype, **BOTH, **ROLL)
    b = make_env(net, impl, mode, E_, 2718, observation=observation, **ROLL)
    assert a.observation_space.dtype == (np.float32 if dtype == F32 else np.float64)
    assert np.all(np.isneginf(a.observation_space.low)) and np.all(np.isposinf(a.observation_space.high))
    assert a.io_map["action"] is None and a._norm_stats.dtype == F64
    st, tabs, n_reset = rollout(a, b, 8, 17, "%s %s %s" % (net, impl, mode))
    assert n_reset >= E_ and st["n_updates"] == 8 and st["cnt"] > io_norm.COUNT0 and st["rcnt"] > io_norm.COUNT0
    assert same(a.io_map["obs"][0], tabs[0]) and a.io_map["reward_scale"] == tabs[2]


# ---- 3. each part alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", ["obs_norm", "reward_norm"])
def test_each_part_alone_leaves_the_other_at_the_identity(part):
    a = make_env("anm6", "thread", "uniform", 65, 3, io_dtype=F32, **{part: "running"}, **ROLL)
    b = make_env("anm6", "thread", "uniform", 65, 3, **ROLL)
    st, tabs, _ = rollout(a, b, 5, 1, part)
    if part == "obs_norm":
        assert tabs[2] == 1.0 and a.ret_rms is None and st["rcnt"] == io_norm.COUNT0 and not st["G"].any() and (tabs[0] != 1).all()
    else:
        assert (tabs[0] == 1).all() and np.signbit(tabs[1]).all() and a.obs_rms is None and st["cnt"] == io_norm.COUNT0 and tabs[2] != 1.0
        assert np.array_equal(a.observation_space.low, b.observation_space.low.astype(np.float32))   # (the plain Box stays)
        assert bool(a._norm_t_seen.any())


# ---- 4. evaluation: frozen tables -----------------------------------------------------------------------------------------------------
def test_norm_training_false_freezes_tables_and_statistics():
    a = make_env("anm6", "thread", "uniform", 65, 3, **BOTH, **ROLL)
    b = make_env("anm6", "thread", "uniform", 65, 3, **ROLL)
    st, tabs, _ = rollout(a, b, 4, 1, "training")
    frozen = a.norm_state()
    a.norm_training = False
    rollout(a, b, 4, 2, "frozen", st=st, tabs=tabs, check_state=False)     # rows mapped by the frozen tables
    now = a.norm_state()
    for k in ("cnt", "mean", "var", "rcnt", "rmean", "rvar", "n_updates", "n_skipped"):
        assert same(np.asarray(frozen[k]), np.asarray(now[k])), k
    assert all(same(t, u) for t, u in zip(device_tables(a)[:2], tabs[:2])) and device_tables(a)[2] == tabs[2] and now["n_updates"] == 4


# ---- 5. checkpoints ---------------------------------------------------------------------------------------------------------------------
def test_norm_state_round_trip_continues_bit_identically():
    kw = dict(io_dtype=F32, **BOTH, **ROLL)
    a = make_env("anm6", "thread", "uniform", 65, 3, **kw)
    device_reset(a)
    gen = torch.Generator(device=DEV).manual_seed(5)
    acts = [box_actions(a, gen) for _ in range(6)]
    for u in acts[:3]:
        a.step(u)
    ck = a.norm_state()
    c = make_env("anm6", "thread", "uniform", 65, 3, **kw)
    device_reset(c)
    for u in acts[:3]:                   # the same trajectory, normalised by whatever: then the checkpoint
        c.norm_training = False
        c.step(u)
    c.norm_training = True
    c.load_norm_state(ck)
    assert all(same(np.asarray(ck[k]), np.asarray(c.norm_state()[k])) for k in ck)
    for u in acts[3:]:
        oa, ra, _, _, _ = a.step(u)
        oc, rc, _, _, _ = c.step(u)
        assert tsame(oa, oc) and tsame(ra, rc) and torch.equal(a.state, c.state)
        x, y = a.norm_state(), c.norm_state()
        assert all(same(np.asarray(x[k]), np.asarray(y[k])) for k in x)
        assert all(same(np.asarray(p), np.asarray(q)) for p, q in zip(device_tables(a), device_tables(c)))
    with pytest.raises(errors.ArgsError, match="mean and var"):
        c.load_norm_state(dict(ck, mean=np.zeros(3)))


# ---- 6. masked reset() ------------------------------------------------------------------------------------------------------------------
def test_masked_reset_zeroes_the_accumulators_of_its_rows_only():
    a = make_env("anm6", "thread", "uniform", 131, 9, **BOTH)
    device_reset(a)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(2):
        a.step(box_actions(a, gen))
    G, seen = a._norm_G.clone(), a._norm_t_seen.clone()
    stats = a._norm_stats.clone()
    assert bool((G != 0).any()) and bool((seen == 2).any())
    m = torch.arange(131, device=DEV) % 3 == 0
    device_reset(a, m)
    assert not bool(a._norm_G[m].any()) and not bool(a._norm_t_seen[m].any())
    assert torch.equal(a._norm_G[~m], G[~m]) and torch.equal(a._norm_t_seen[~m], seen[~m])
    assert torch.equal(a._norm_stats.view(torch.int64), stats.view(torch.int64))          # reset() does not update


# ---- 7. HIP graph: the step and the pair, nothing allocated ----------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_allocates_nothing():
    kw = dict(io_dtype=F32, **BOTH, **ROLL)
    env, twin = make_env("anm6", "thread", "uniform", 1025, 8, **kw), make_env("anm6", "thread", "uniform", 1025, 8, **kw)
    device_reset(env)
    device_reset(twin)
    gen = torch.Generator(device=DEV).manual_seed(6)
    acts = [box_actions(env, gen) for _ in range(3)]
    buf = acts[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(buf)
    torch.cuda.synchronize()
    assert not bool(env.timestep.any()) and env.norm_state()["n_updates"] == 0          # capture does not execute
    gc.collect()                         # (environments of earlier tests, freed by the cycle collector, would move the count)
    m0 = torch.cuda.memory_allocated()
    for t, u in enumerate(acts):
        buf.copy_(u)
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0
        o2, r2, _, _, _ = twin.step(u)
        assert tsame(env._state_obs, o2) and tsame(env.reward, r2) and torch.equal(env.state, twin.state), "replay %d" % t
        x, y = env.norm_state(), twin.norm_state()
        assert all(same(np.asarray(x[k]), np.asarray(y[k])) for k in x), "replay %d" % t
        assert all(same(np.asarray(p), np.asarray(q)) for p, q in zip(device_tables(env), device_tables(twin)))
    assert env.norm_state()["n_updates"] == 3
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    for u in acts:                       # eager steps from a preallocated tensor allocate nothing either
        buf.copy_(u)
        twin.step(buf)
        assert torch.cuda.memory_allocated() == m0


# ---- 8. the same batch twice ------------------------------------------------------------------------------------------------------------
def test_the_same_batch_twice_gives_identical_bits():
    """(two batch sizes that share a prefix of rows sum by different trees, by design: the tree is over the batch)"""
    runs = []
    for _ in range(2):
        a = make_env("anm6", "thread", "noise", 3001, 4, **BOTH, **ROLL)
        device_reset(a)
        gen = torch.Generator(device=DEV).manual_seed(2)
        for _ in range(5):
            o, r, _, _, _ = a.step(box_actions(a, gen))
        runs.append((a.norm_state(), device_tables(a), o.clone(), r.clone()))
    (x, tx, ox, rx), (y, ty, oy, ry) = runs
    assert all(same(np.asarray(x[k]), np.asarray(y[k])) for k in x) and all(same(np.asarray(p), np.asarray(q)) for p, q in zip(tx, ty))
    assert tsame(ox, oy) and tsame(rx, ry) and x["n_updates"] == 5


# ---- 9. refusals of the C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_carry_a_message():
    a = make_env("anm6", "thread", "uniform", 1025, 1, **BOTH)
    plain = make_env("anm6", "thread", "uniform", 8, 1)
    lib = a.simulator.backend.lib
    err = lambda: lib.anm_last_error()  # noqa: E731
    h = a.simulator._handle
    ptrs = (a._state_obs.data_ptr(), a.reward.data_ptr(), a._term_u8.data_ptr(), a._trunc_u8.data_ptr(), a.timestep.data_ptr())
    assert lib.anm_model_io_norm_update(plain.simulator._handle, 8, *ptrs, a._norm_ref, None) != 0 and b"anm_model_set_io_map" in err()
    assert lib.anm_model_io_norm_tables(plain.simulator._handle, a._norm_ref, None) != 0 and b"anm_model_set_io_map" in err()
    assert lib.anm_model_io_norm_update(h, 0, *ptrs, a._norm_ref, None) != 0 and b"num_envs < 1" in err()
    short = _lib.IoNorm.from_buffer_copy(a._norm_struct)
    short.n_slab_doubles = io_norm.slab_doubles(1024, a.observation_N)
    assert lib.anm_model_io_norm_update(h, 1025, *ptrs, C.byref(short), None) != 0 and b"slab buffer is too short" in err()
    assert lib.anm_model_io_norm_update(h, 1024, *ptrs, C.byref(short), None) == 0        # (one slab: enough for 1024 rows)
    bad = _lib.IoNorm.from_buffer_copy(a._norm_struct)
    bad.eps = 0.0
    assert lib.anm_model_io_norm_update(h, 1025, *ptrs, C.byref(bad), None) != 0 and b"eps" in err()
    assert lib.anm_model_io_norm_update(h, 1025, *ptrs, None, None) != 0 and b"null anm_io_norm" in err()
    torch.cuda.synchronize()
