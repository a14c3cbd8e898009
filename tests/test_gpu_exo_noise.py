"""GPU tier: the noisy time series (``BatchedANMEnv(exogenous="series_noise")``) -- every step each load and non-slack
generator gets its table value plus bounded noise from the counter-based RNG, clipped, inside the step kernels
(specification: gym_anm_amd/rng.py, exo_series_noise).  From the outside in:
  1. the rows of ``sample_init_state()`` against the specification, and the samplers inside the reset kernels against them;
  2. the mode equals the host-hook path it replaces (``next_vars`` returning the specification's draws), bit for bit;
  3. zero noise equals series mode, bit for bit, autoreset, time limit and statistics included;
  4. oracle replay with autoreset on ANM6; 5. float32 I/O, sharding, HIP graph, no allocation; 6. the distribution;
  7. what the mode refuses."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest
import torch
from scipy import stats

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.envs.anm6 import ANM6EasyVec, anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0)}
CASES = [("anm6", "thread"), ("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial"), ("case30", "mesh")]
E_ODD = 229       # 3 * 64 + 37: more than one block of environments, the last one partial
STATS = ("episode_return", "episode_discounted_return", "last_episode_return", "last_episode_discounted_return",
         "last_episode_length", "episodes_done")


@functools.lru_cache(maxsize=None)
def task_of(net):
    """(series, noise, low, high) in MW.  ANM6: ANM6Easy's table with +-25 % of |series| and the default ends (the solar
    farm's table reaches its p_max: the clip bites there).  The feeder: a made-up table of period 5 -- every environment
    wraps several times in 20 steps -- at 30 ... 60 % of every unit's range, amplitudes of 20 % of the range, and ends that
    bite on every third unit (5 % of the range around the unit's table values), never on the others (the whole range) and
    are infinite on unit 1."""
    model = NetworkModel(NETS[net](), 0.25, 100)
    lo, hi = rng.default_exo_bounds(model)
    if net == "anm6":
        ser = anm6easy_series()
        return ser, 0.25 * np.abs(ser), lo, hi
    span = lo + hi                                           # one end of every default interval is zero
    frac = np.array([0.3, 0.45, 0.6, 0.5, 0.35])
    unit = 1.0 - 0.02 * (np.arange(len(lo)) % 4)
    ser = np.ascontiguousarray(span[:, None] * unit[:, None] * frac[None, :])
    noise = np.ascontiguousarray(np.broadcast_to(0.2 * np.abs(span)[:, None], ser.shape))
    low, high = lo.copy(), hi.copy()
    tight = np.arange(len(lo)) % 3 == 0
    low[tight] = ser[tight].min(axis=1) - 0.05 * np.abs(span[tight])
    high[tight] = ser[tight].max(axis=1) + 0.05 * np.abs(span[tight])
    low[1], high[1] = -INF, INF
    return ser, noise, low, high


def make_env(net, impl, E_, seed, cls=BatchedANMEnv, mode="noise", noise=None, ends=None, **kw):
    ser, amp, low, high = task_of(net)
    if mode == "noise":
        low, high = (low, high) if ends is None else ends
        kw.update(exogenous="series_noise", exo_noise=amp if noise is None else noise, exo_low=low, exo_high=high, series=ser)
    elif mode == "series":
        kw.update(series=ser)
    env = cls(NETS[net](), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, ser.shape[1] - 1),)), costs_clipping=(1, 100),
              seed=seed, num_envs=E_, device=DEV, tol=1e-6, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def drawn_columns(model):
    D, nd = model.N_device, model.N_des
    fused = list(model.load_idx) + list(model.gen_idx) + [2 * D + nd + g for g in range(model.N_non_slack_gen)]
    loose = [D + k for k in model.gen_idx] + [2 * D + e for e in range(nd)]
    return fused, loose


def spec_draws(seed, envs, epochs, ts, auxs, task):
    """rng.exo_series_noise for arrays of keys, exactly: the Philox words by the vectorised generator (integers: bit for
    bit the scalar one's), the two fused multiply-adds and the clip by the scalar specification's own functions."""
    ser, amp, low, high = task
    envs, epochs, ts = (np.asarray(a, dtype=np.uint64) for a in (envs, epochs, ts))
    kw = rng.philox4x32_v(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), envs, epochs, np.uint64(rng.EXO_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))
    n = ser.shape[0]
    out = np.empty((len(envs), n))
    for j in range((n + 1) // 2):
        q = rng.philox4x32_v(key, (ts & np.uint64(rng.MASK)) | (np.uint64(j) << np.uint64(32)), np.uint64(0), np.uint64(rng.EXO_TAG))
        for h in range(2):
            i = 2 * j + h
            if i < n:
                u = rng.u01_v(q[..., 2 * h], q[..., 2 * h + 1])
                for e in range(len(envs)):
                    w = rng.fma(2.0, float(u[e]), -1.0)
                    out[e, i] = rng.noise_clip(rng.fma(float(amp[i, auxs[e]]), w, float(ser[i, auxs[e]])), float(low[i]), float(high[i]))
    return out


def test_the_batched_specification_is_the_scalar_one():
    task = task_of("case30")
    envs, epochs = np.array([0, (1 << 32) - 1, (1 << 33) + 9]), np.array([0, 3, 2**31 - 2])
    ts, auxs = np.array([0, 7, 123456]), np.array([0, 4, 2])
    got = spec_draws(11, envs, epochs, ts, auxs, task)
    for k in range(3):
        want = rng.exo_series_noise(11, int(envs[k]), int(epochs[k]), int(ts[k]), int(auxs[k]), *task)
        assert got[k].tobytes() == want.tobytes()


# ---- 1. the draws ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n_keys", [("anm6", 1500), ("case30", 229)])
def test_rows_of_the_sampler_against_the_specification(net, n_keys):
    SEED, OFF = 0x0123456789ABCDE, (1 << 32) - n_keys // 3            # (the environment index crosses 2^32)
    env = make_env(net, "radial", n_keys, SEED, env_offset=OFF)
    model, task = env.simulator.model, task_of(net)
    epochs = np.random.default_rng(3).integers(0, 2**31 - 1, n_keys).astype(np.int32)
    epochs[:8] = [0, 1, 2, 3, 2**31 - 2, 2**31 - 2, 7, 7]
    env._reset_count.copy_(torch.as_tensor(epochs))
    rows, raw = env.sample_init_state(raw=True)
    rows, raw = rows.cpu().numpy(), raw.cpu().numpy()
    fused, loose = drawn_columns(model)
    rest = [k for k in range(rows.shape[1] - 1) if k not in fused and k not in loose]
    D = model.N_device
    span = {D + k: max(abs(model.dev_q_min[k]), abs(model.dev_q_max[k])) for k in model.gen_idx}
    span.update({2 * D + e: max(abs(model.dev_soc_min[k]), abs(model.dev_soc_max[k])) for e, k in enumerate(model.des_idx)})
    period = task[0].shape[1]
    seen_aux, n_clipped = set(), 0
    for e in range(n_keys):
        want = rng.series_noise_init_state(model, *task, SEED, OFF + e, int(epochs[e]))
        npt.assert_array_equal(rows[e, fused], want[fused], err_msg="env %d" % e)      # the fused draws: exactly
        npt.assert_array_equal(rows[e, rest], 0.0)
        assert rows[e, -1] == want[-1] == (rng.philox4x32(SEED, OFF + e, int(epochs[e]), 0)[0] * period) >> 32
        for c in loose:                                                               # lo + (hi - lo) u: one rounding
            assert abs(rows[e, c] - want[c]) <= 2.0**-52 * max(span[c], 1e-300), (e, c)
        seen_aux.add(int(rows[e, -1]))
        # `raw` still holds the init sampler's blocks
        assert tuple(int(x) for x in raw[e, 0]) == tuple(rng.philox4x32(SEED, OFF + e, int(epochs[e]), 0))
    assert len(seen_aux) >= min(period, 50)
    x = rows[:, list(model.load_idx) + [2 * D + model.N_des + g for g in range(model.N_non_slack_gen)]]
    at_end = (x == task[2]) | (x == task[3])
    assert at_end.any() and not at_end.all(axis=0).any()          # the clip bites somewhere, and nowhere always
    lo_v = rng.series_noise_init_state_v(model, *task, SEED, OFF + np.arange(n_keys), epochs.astype(np.uint64))
    npt.assert_allclose(rows, lo_v, rtol=1e-15, atol=1e-14)
    assert int(env._reset_count.sum()) == int(epochs.astype(np.int64).sum())      # the epochs are not consumed


@pytest.mark.parametrize("net,impl", CASES)
def test_reset_kernels_draw_what_the_entry_point_draws(net, impl):
    a, b = make_env(net, impl, E_ODD, 99, env_offset=12345), make_env(net, impl, E_ODD, 99, env_offset=12345)
    for rnd in range(3):
        mask = None if rnd == 0 else (torch.rand(E_ODD, device=DEV) < 0.3)
        drawn = b.sample_init_state()
        todo = torch.ones(E_ODD, dtype=torch.bool, device=DEV) if mask is None else mask.clone()
        obs_a, _ = a.reset(options={"mask": mask})       # plain reset(): the device sampler in this mode
        for attempt in range(100):
            b._launch_reset(drawn.contiguous(), todo.to(torch.uint8))
            b._reset_count += todo.to(torch.int32)
            todo = todo & (b._conv_u8 == 0)
            if not bool(todo.any()):
                break
            drawn = b.sample_init_state()
        assert torch.equal(a._reset_count, b._reset_count)
        assert torch.equal(a.state, b.state) and torch.equal(a.simulator.soc, b.simulator.soc)
        assert torch.equal(obs_a, b.observation(b.state))
        assert not bool(a.timestep.any())
    assert int(a._reset_count.min()) >= 1


def test_reset_from_given_rows_starts_a_new_episode_too():
    env = make_env("anm6", "radial", E_ODD, 5)
    rows = env.sample_init_state()
    env.reset(options={"init_state": rows})
    assert bool((env._reset_count == 1).all())
    mask = torch.arange(E_ODD, device=DEV) % 3 == 0
    env.reset(options={"init_state": rows, "mask": mask})
    assert torch.equal(env._reset_count, 1 + mask.to(torch.int32))


# ---- 2. the mode equals the hook path it replaces ----------------------------------------------------------------------
class HookTask(BatchedANMEnv):
    """the same task through next_vars(): the specification's draws for step index timestep + 1 at the next table index --
    the state row alone does not replay the stream, so the hook reads ``self.timestep``"""

    def next_vars(self, s_t):
        period = self.spec_task[0].shape[1]
        aux1 = np.fmod(s_t[:, -1].cpu().numpy() + 1.0, float(period)).astype(np.int64)
        t1 = self.timestep.cpu().numpy().astype(np.int64) + 1
        x = spec_draws(self.rng_seed, self.env_offset + np.arange(self.num_envs), self.spec_epoch, t1, aux1, self.spec_task)
        return torch.as_tensor(np.concatenate((x, aux1[:, None].astype(np.float64)), axis=1), device=self.device)


@pytest.mark.parametrize("net,impl", CASES)
def test_the_mode_equals_the_hook_path_bit_for_bit(net, impl):
    E_, T, SEED, OFF = 256, 20, 4242, (1 << 32) - 100
    noi = make_env(net, impl, E_, SEED, env_offset=OFF)
    hook = make_env(net, impl, E_, SEED, cls=HookTask, mode="hook", env_offset=OFF)
    rows = noi.sample_init_state()
    noi.reset(options={"init_state": rows})
    hook.reset(options={"init_state": rows})
    hook.spec_task = task_of(net)
    hook.spec_epoch = (noi._reset_count - 1).cpu().numpy()
    assert not hook.spec_epoch.any()
    assert torch.equal(noi.state, hook.state) and torch.equal(noi.simulator.soc, hook.simulator.soc)
    gen = torch.Generator(device=DEV).manual_seed(7)
    period = hook.spec_task[0].shape[1]
    aux0 = noi.state[:, -1].clone()
    n_alive = 0
    for t in range(T):
        a = uniform_actions(noi, gen)
        on, rn, tn, _, _ = noi.step(a)
        oh, rh, th, _, _ = hook.step(a)
        for name, x, y in (("obs", on, oh), ("state", noi.state, hook.state), ("reward", rn, rh), ("e_loss", noi.e_loss, hook.e_loss),
                           ("penalty", noi.penalty, hook.penalty), ("terminated", tn, th),
                           ("nr_iters", noi.simulator.nr_iters, hook.simulator.nr_iters), ("soc", noi.simulator.soc, hook.simulator.soc)):
            assert torch.equal(x, y), "step %d: %s differs (%s, %s)" % (t, name, net, impl)
        alive = ~tn
        n_alive += int(alive.sum())
        assert bool((noi.state[alive, -1] == torch.fmod(aux0 + t + 1, period)[alive]).all())      # the table index wraps
        assert bool((noi.timestep[alive] == t + 1).all())
    print("%s %s: %d of %d environment-steps alive" % (net, impl, n_alive, E_ * T))
    assert n_alive > E_ * T // 4       # (the comparison is mostly about stepped environments, not absorbing ones)


# ---- 3. zero noise equals series mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_zero_noise_equals_series_mode_bit_for_bit(net, impl):
    ser = task_of(net)[0]
    n = ser.shape[0]
    kw = dict(autoreset=True, max_episode_steps=5, episode_stats=True)
    a = make_env(net, impl, E_ODD, 31, mode="series", **kw)
    b = make_env(net, impl, E_ODD, 31, noise=0.0, ends=(np.full(n, -INF), np.full(n, INF)), **kw)
    oa, _ = a.reset(options={"sampler": "device"})
    ob, _ = b.reset()
    gen = torch.Generator(device=DEV).manual_seed(5)
    n_reset = 0
    for t in range(31):
        if t:
            act = uniform_actions(a, gen)
            rc = a._reset_count.clone()
            oa, ob = a.step(act)[0], b.step(act)[0]
            n_reset += int((a._reset_count - rc).sum())
        for name, x, y in [("obs", oa, ob), ("state", a.state, b.state), ("reward", a.reward, b.reward), ("e_loss", a.e_loss, b.e_loss),
                           ("penalty", a.penalty, b.penalty), ("terminated", a.terminated, b.terminated),
                           ("truncated", a.truncated, b.truncated), ("soc", a.simulator.soc, b.simulator.soc),
                           ("timestep", a.timestep, b.timestep), ("reset_count", a._reset_count, b._reset_count),
                           ("nr_iters", a.simulator.nr_iters, b.simulator.nr_iters)] + [(k, getattr(a, k), getattr(b, k)) for k in STATS]:
            assert torch.equal(x, y), "step %d: %s differs (%s, %s)" % (t, name, net, impl)
    assert n_reset >= 4 * E_ODD and int(a.episodes_done.min()) >= 4      # (the limit of 5 re-initialises everybody)


# ---- 4. oracle replay ---------------------------------------------------------------------------------------------------------
def oracle_replay(net, env, T, n_random, n_collapsed, seed):
    """oracle_replay of tests/test_gpu_exo_uniform.py for this mode (same structure, same tolerances): a seeded sample of
    environments plus collapsed ones are replayed by OracleEnv(next_vars = the specification at the step index the replay
    keeps), restarted from rng.series_noise_init_state at each autoreset.  Returns (replayed, terminations, resets)."""
    import anm_oracle as O

    network, task = NETS[net](), task_of(net)
    period = task[0].shape[1]
    model, dev, E_ = env.simulator.model, env.device, env.num_envs
    env.reset(seed=seed)
    rc0 = env._reset_count.clone()
    state0, soc0 = env.state.clone(), env.simulator.soc.clone()
    gen = torch.Generator(device=dev).manual_seed(99)
    rec = {k: [] for k in ("a", "obs", "r", "term", "it", "rc", "el", "pen", "state")}
    for t in range(T):
        a = uniform_actions(env, gen)
        rec["rc"].append(env._reset_count.clone())
        obs, r, term, _, _ = env.step(a)
        for k, v in zip(("a", "obs", "r", "term", "it", "el", "pen", "state"),
                        (a, obs, r, term, env.simulator.nr_iters, env.e_loss, env.penalty, env.state)):
            rec[k].append(v.clone())
    collapsed = torch.nonzero(torch.stack(rec["term"])[: T - 2].any(dim=0))[:, 0].cpu().numpy()
    sample = np.unique(np.concatenate((np.random.default_rng(0).choice(E_, n_random, replace=False),
                                       collapsed if n_collapsed is None else collapsed[:n_collapsed])))
    idx = torch.as_tensor(sample, device=dev)
    R = {k: torch.stack([x[idx] for x in v]).cpu().numpy() for k, v in rec.items()}
    s0, c0, e0 = state0[idx].cpu().numpy(), soc0[idx].cpu().numpy(), (rc0[idx] - 1).cpu().numpy()
    n_reset = n_term = 0
    for j, e in enumerate(sample):
        ge = env.env_offset + int(e)
        epoch, tstep = [int(e0[j])], [0]       # the episode's epoch and its step index (the environment's `timestep`)

        def spec(state):
            aux1 = int(np.fmod(state[-1] + 1.0, float(period)))
            return np.concatenate((rng.exo_series_noise(seed, ge, epoch[0], tstep[0] + 1, aux1, *task), [aux1]))

        orc = O.OracleEnv(network, sparse=False, tol=1e-6, aux_bounds=((0, period - 1),), next_vars=spec)
        orc.load_state(s0[j], c0[j])
        for t in range(T):
            if orc.terminated:  # Gymnasium next-step autoreset: this call returns the first observation of a new episode
                epoch[0], tstep[0] = int(R["rc"][t][j]), 0
                o, conv = orc.reset_to(rng.series_noise_init_state(model, *task, seed, ge, epoch[0]))
                assert bool(R["term"][t][j]) == (not conv), (e, t)
                assert R["r"][t][j] == 0.0 and R["el"][t][j] == 0.0 and R["pen"][t][j] == 0.0
                n_reset += 1
                if not conv:     # a draw whose first power flow does not converge: drawn again at the next call
                    assert not R["obs"][t][j].any()
                    orc.terminated = True
                    continue
            else:
                o, r, term = orc.step(R["a"][t][j])
                tstep[0] += 1
                assert term == bool(R["term"][t][j]), (e, t)
                npt.assert_allclose(R["r"][t][j], r, rtol=1e-9, atol=1e-12)
                if term:
                    n_term += 1
                    assert not R["obs"][t][j].any()
                    continue
                npt.assert_allclose(R["el"][t][j], orc.e_loss, rtol=1e-9, atol=1e-12)
                npt.assert_allclose(R["pen"][t][j], orc.penalty, rtol=1e-9, atol=1e-10)
            npt.assert_allclose(R["obs"][t][j], o, rtol=0, atol=1e-9, err_msg="env %d step %d" % (e, t))
            assert int(R["it"][t][j]) == orc.last["n_iter"], (e, t)
    return len(sample), n_term, n_reset


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_oracle_replay_with_autoreset_on_anm6(impl):
    """Amplitude used: ANM6Easy's table with +-25 % of |series|, the starting value.  (Series mode alone collapses under
    uniformly random actions at batches of this size -- tests/test_gpu_headline.py asks for 32 terminations in 10 steps of
    65 536 environments -- so the reference path is expected to produce one here in 24 steps of 4 096; the assertion below
    holds the test to it.)"""
    env = make_env("anm6", impl, 4096, 1234, autoreset=True)
    n, n_term, n_reset = oracle_replay("anm6", env, 24, 48, 16, 1234)
    print("replayed %d environments: %d terminations, %d resets" % (n, n_term, n_reset))
    assert n >= 48 and n_term >= 1 and n_reset >= 1


# ---- 5. composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", CASES)
def test_float32_io_is_the_float64_run_rounded_once(net, impl):
    kw = dict(autoreset=True, max_episode_steps=7)
    a = make_env(net, impl, E_ODD, 8, **kw)
    b = make_env(net, impl, E_ODD, 8, io_dtype=torch.float32, **kw)
    oa, ob = a.reset()[0], b.reset()[0]
    gen = torch.Generator(device=DEV).manual_seed(2)
    for t in range(13):
        if t:
            act32 = uniform_actions(a, gen).float()      # (check_actions is off: the kernels project the set-points anyway)
            oa, ob = a.step(act32.double())[0], b.step(act32)[0]
        assert ob.dtype == torch.float32 and b.reward.dtype == torch.float32
        assert torch.equal(ob, oa.float()) and torch.equal(b.reward, a.reward.float()), t
        for name, x, y in (("state", a.state, b.state), ("e_loss", a.e_loss, b.e_loss), ("penalty", a.penalty, b.penalty),
                           ("terminated", a.terminated, b.terminated), ("truncated", a.truncated, b.truncated),
                           ("soc", a.simulator.soc, b.simulator.soc), ("timestep", a.timestep, b.timestep),
                           ("reset_count", a._reset_count, b._reset_count), ("nr_iters", a.simulator.nr_iters, b.simulator.nr_iters)):
            assert torch.equal(x, y), "step %d: %s" % (t, name)


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_two_shards_equal_the_whole_batch(impl):
    H0 = 101
    whole = make_env("anm6", impl, E_ODD, 77, autoreset=True, max_episode_steps=4)
    shards = [make_env("anm6", impl, n, 77, autoreset=True, max_episode_steps=4, env_offset=off) for off, n in ((0, H0), (H0, E_ODD - H0))]
    ow, _ = whole.reset(seed=77)
    assert torch.equal(ow, torch.cat([s.reset(seed=77)[0] for s in shards]))
    gen = torch.Generator(device=DEV).manual_seed(3)
    for t in range(10):
        a = uniform_actions(whole, gen)
        ow, rw, tw, _, _ = whole.step(a)
        outs = [s.step(a[lo_:hi_].contiguous()) for s, (lo_, hi_) in zip(shards, ((0, H0), (H0, E_ODD)))]
        for name, x, ys in (("obs", ow, [o[0] for o in outs]), ("reward", rw, [o[1] for o in outs]), ("terminated", tw, [o[2] for o in outs]),
                            ("state", whole.state, [s.state for s in shards]), ("soc", whole.simulator.soc, [s.simulator.soc for s in shards]),
                            ("reset_count", whole._reset_count, [s._reset_count for s in shards]),
                            ("timestep", whole.timestep, [s.timestep for s in shards]),
                            ("nr_iters", whole.simulator.nr_iters, [s.simulator.nr_iters for s in shards])):
            assert torch.equal(x, torch.cat(ys)), "step %d: %s" % (t, name)
    assert int(whole._reset_count.min()) >= 3          # (the limit of 4 re-initialised everybody twice)


@pytest.mark.parametrize("net,impl", CASES)
def test_a_captured_step_replays_what_eager_steps_compute_and_allocates_nothing(net, impl):
    eager, graphed = make_env(net, impl, E_ODD, 21, autoreset=True), make_env(net, impl, E_ODD, 21, autoreset=True)
    eager.reset()
    graphed.reset()
    gen = torch.Generator(device=DEV).manual_seed(4)
    acts = [uniform_actions(eager, gen) for _ in range(6)]
    a_buf = acts[0].clone()
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):       # the FIRST step after reset() is the captured one
            obs_g, rew_g, term_g, _, _ = graphed.step(a_buf)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    assert not bool(graphed.timestep.any())             # (capturing ran nothing)
    before = None
    for t, act in enumerate(acts):
        a_buf.copy_(act)
        g.replay()
        obs_e, rew_e, term_e, _, _ = eager.step(act)
        torch.cuda.synchronize()
        if t == 1:
            before = torch.cuda.memory_allocated(DEV)
        for name, x, y in (("obs", obs_e, obs_g), ("reward", rew_e, rew_g), ("terminated", term_e, term_g), ("state", eager.state, graphed.state),
                           ("timestep", eager.timestep, graphed.timestep), ("reset_count", eager._reset_count, graphed._reset_count)):
            assert torch.equal(x, y), "step %d: %s" % (t, name)
    assert torch.cuda.memory_allocated(DEV) == before     # no allocation over steps (the eager path included)


def test_anm6easyvec_takes_the_mode_through_its_keywords():
    env = ANM6EasyVec(num_envs=E_ODD, device=DEV, seed=3, tol=1e-6, exogenous="series_noise", exo_noise=0.5, autoreset=True)
    twin = make_env("anm6", env.simulator.impl, E_ODD, 3, noise=0.5, ends=rng.default_exo_bounds(env.simulator.model), autoreset=True)
    env.check_actions = False
    assert env.exo_noise.shape == anm6easy_series().shape and (env.exo_noise == 0.5).all()
    oe, ot = env.reset()[0], twin.reset()[0]            # the device sampler, not ANM6EasyVec.init_state
    assert torch.equal(env.state, twin.state)
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    env.step(a)
    twin.step(a)
    assert torch.equal(env.state, twin.state) and bool((env.timestep == 1).all())


# ---- 6. distribution -----------------------------------------------------------------------------------------------------
def test_the_noise_is_uniform_where_the_clip_cannot_bite():
    E_ = 16384
    ser, amp, low, high = task_of("case30")
    env = make_env("case30", "radial", E_, 31337)
    model = env.simulator.model
    D, nd = model.N_device, model.N_des
    cols = list(model.load_idx) + [2 * D + nd + g for g in range(model.N_non_slack_gen)]
    free = [i for i in range(len(cols)) if (ser[i] - amp[i] >= low[i]).all() and (ser[i] + amp[i] <= high[i]).all()]
    assert 1 in free and len(free) >= len(cols) // 2 and len(free) < len(cols)
    z, n_rows = [[] for _ in free], 0
    for epoch in range(13):                              # 13 x 16 384 = 212 992 draws per unit
        env._reset_count.fill_(epoch)
        rows = env.sample_init_state().cpu().numpy()
        aux = rows[:, -1].astype(np.int64)
        for k, i in enumerate(free):
            z[k].append((rows[:, cols[i]] - ser[i, aux]) / amp[i, aux])
        n_rows += E_
    assert n_rows >= 200000
    z = np.array([np.concatenate(c) for c in z])
    for k, i in enumerate(free):
        assert -1.0 - 1e-12 <= z[k].min() and z[k].max() < 1.0 + 1e-12, i
        assert stats.kstest(z[k], "uniform", args=(-1.0, 2.0)).pvalue > 1e-3, i
    c_ = np.corrcoef(z[:, :E_])
    assert np.abs(c_ - np.eye(len(free))).max() < 0.04
    # a unit whose ends bite sits on them with positive probability, and never beyond
    tight = [i for i in range(len(cols)) if i not in free]
    x = rows[:, [cols[i] for i in tight]]
    assert (x >= low[tight]).all() and (x <= high[tight]).all() and ((x == low[tight]) | (x == high[tight])).any()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_what_the_mode_refuses():
    from gym_anm_amd.envs.mixed import MixedBatchedANMEnv

    env = make_env("anm6", "radial", 64, 1)
    env.reset()
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    sim = env.simulator
    lib = sim.backend.lib
    n = sim.N_load + sim.N_non_slack_gen
    exo = torch.zeros((64, n), dtype=torch.float64, device=DEV)
    aux = torch.zeros((64, 1), dtype=torch.float64, device=DEV)
    with pytest.raises(errors.HipExtensionError, match="exo and aux_next must be NULL"):
        env._step_call(a.data_ptr(), exo.data_ptr(), aux.data_ptr())
    # a step without the timestep buffer
    env._step_call(a.data_ptr(), None, None)
    args = list(env._step_args)
    args[3] = None
    env._step_args = tuple(args)
    with pytest.raises(errors.HipExtensionError, match="timestep"):
        env._step_call(a.data_ptr(), None, None)
    env._step_args = None
    # a batch view and parameter classes: refused where they are bound
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(sim._handle, C.byref(view)) != 0 and b"series-noise" in lib.anm_last_error()
    cls = torch.zeros(64, dtype=torch.int32, device=DEV)
    assert lib.anm_model_bind_env_classes(sim._handle, cls.data_ptr(), 64) != 0 and b"series-noise" in lib.anm_last_error()
    desc, keep = _lib.network_desc(sim.model)
    descs = (C.POINTER(_lib.NetworkDesc) * 2)(C.pointer(desc), C.pointer(desc))
    assert lib.anm_model_set_classes(sim._handle, 2, descs) != 0 and b"parameter classes" in lib.anm_last_error()
    env.reset()
    env.step(a)
    # ... and the other way round: the mode set on a model that has a view bound (a series-mode model here)
    plain = make_env("anm6", "radial", 64, 1, mode="series")
    psim = plain.simulator
    ser, amp, low, high = task_of("anm6")
    slo, shi = plain._cfg_keep

    def cfg(cls=_lib.EnvConfigNoise, **b):
        arr = {k: np.ascontiguousarray(b.get(k, d), dtype=np.float64) for k, d in (("lo", low), ("hi", high), ("amp", amp), ("ser", ser))}
        c = cls(K=b.get("K", 1), gamma=0.9, clip_e_loss=1.0, clip_penalty=100.0, obs_low=_lib.as_c(slo, np.float64)[1],
                obs_high=_lib.as_c(shi, np.float64)[1],
                series=None if b.get("no_series") else arr["ser"].ctypes.data_as(_lib.c_double_p), period=0 if b.get("no_series") else ser.shape[1],
                exo_mode=_lib.EXO_SERIES_NOISE, exo_low=arr["lo"].ctypes.data_as(_lib.c_double_p), exo_high=arr["hi"].ctypes.data_as(_lib.c_double_p))
        if cls is _lib.EnvConfigNoise and not b.get("no_amp"):
            c.exo_noise = arr["amp"].ctypes.data_as(_lib.c_double_p)
        c._keep = arr
        return c

    assert lib.anm_model_bind_view(psim._handle, C.byref(view)) == 0
    c = cfg()
    assert lib.anm_model_set_env(psim._handle, C.byref(c)) != 0 and b"batch view" in lib.anm_last_error()
    assert lib.anm_model_bind_view(psim._handle, None) == 0
    # the task itself
    nan_amp, neg_amp, inf_amp = amp.copy(), amp.copy(), amp.copy()
    nan_amp[1, 3], neg_amp[2, 0], inf_amp[0, 5] = np.nan, -1e-300, INF
    nan_lo = low.copy()
    nan_lo[2] = np.nan
    bad = [(dict(K=2), b"K = 1"), (dict(no_series=True), b"needs a series"), (dict(no_amp=True), b"amplitude table"),
           (dict(cls=_lib.EnvConfigEpisode), b"amplitude table"), (dict(cls=_lib.EnvConfig), b"amplitude table"),
           (dict(amp=nan_amp), b"finite and >= 0"), (dict(amp=neg_amp), b"finite and >= 0"), (dict(amp=inf_amp), b"finite and >= 0"),
           (dict(lo=nan_lo), b"NaN"), (dict(lo=np.ones(n), hi=np.zeros(n)), b"exo_low <= exo_high")]
    for b, msg in bad:
        c = cfg(**b)
        assert lib.anm_model_set_env(psim._handle, C.byref(c)) != 0, b
        assert msg in lib.anm_last_error(), (b, lib.anm_last_error())
    # infinite ends are allowed
    c = cfg(lo=np.full(n, -INF), hi=np.full(n, INF))
    assert lib.anm_model_set_env(psim._handle, C.byref(c)) == 0
    # the public classes
    net6 = networks.anm6_network()
    with pytest.raises(errors.EnvInitializationError, match="parameter classes"):
        make_env("anm6", "radial", 64, 1, variants=[networks.anm6_network()], env_variant=np.zeros(64, dtype=np.int32))
    with pytest.raises(errors.EnvInitializationError, match="K = 1"):
        BatchedANMEnv(net6, "state", 2, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="series_noise", series=ser, exo_noise=1.0)
    with pytest.raises(errors.EnvInitializationError, match="series="):
        BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="series_noise", exo_noise=1.0)
    for bad_amp in (-1.0, np.nan, INF, np.ones(3)):
        with pytest.raises(errors.ArgsError):
            BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="series_noise", series=ser, exo_noise=bad_amp)
    with pytest.raises(errors.ArgsError, match="NaN"):
        BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="series_noise", series=ser, exo_noise=1.0, exo_low=nan_lo)
    with pytest.raises(errors.ArgsError):
        BatchedANMEnv(net6, "state", 1, 0.25, 0.995, 100, num_envs=4, device=DEV, series=ser, exo_low=low)      # ends without a mode
    with pytest.raises(errors.EnvInitializationError, match="series_noise"):
        MixedBatchedANMEnv([dict(network=net6, series=ser, exogenous="series_noise", exo_noise=1.0)], [0, 0, 0, 0], device=DEV)
