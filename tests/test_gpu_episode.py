"""GPU tier: the in-kernel episode time limit, truncation flag and episode statistics
(``BatchedANMEnv(max_episode_steps=, episode_stats=)``; the specification is gym_anm_amd/episode.py).
  1. truncation IS the autoreset path, bit for bit;  2. without autoreset the feature is bookkeeping only;
  3. oracle replay across truncations;  4. the statistics against the specification, bit for bit;
  5. the two-launch step equals the one-launch step;  6. shards equal the whole batch;  7. HIP-graph capture;
  8. resets clear what they touch;  9. refusals."""
import ctypes as C
import functools

import numpy as np
import numpy.testing as npt
import pytest
import torch

from gym_anm_amd import _lib, episode, errors, networks, rng
from gym_anm_amd.envs import ANM6EasyVec, NumpyVectorEnv
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.995

NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0)}
FAMILIES = [("anm6", "thread"), ("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial"), ("case30", "mesh")]
CASES = [(n, i, m) for n, i in FAMILIES for m in ("series", "uniform")]
OUTPUTS = ("obs", "state", "reward", "e_loss", "penalty", "terminated", "soc", "timestep", "reset_count", "nr_iters")
STATS = ("episode_return", "episode_discounted_return", "last_episode_return", "last_episode_discounted_return",
         "last_episode_length", "episodes_done")


@functools.lru_cache(maxsize=None)
def series_of(net):
    """a periodic table [n_load + n_gen, period] in MW: ANM6Easy's own for the 6-bus network; for the feeder a fixed table of
    seeded draws, every unit uniform over its range (loads [p_min, 0], generators [0, p_max]) -- the distribution of the
    uniform mode, so that this mode meets collapsing power flows too"""
    if net == "anm6":
        return anm6easy_series()
    from gym_anm_amd.model import NetworkModel

    lo, hi = rng.default_exo_bounds(NetworkModel(NETS[net](), 0.25, 100))
    period = 512
    u = np.random.default_rng(2024).random((len(lo), period))
    return np.ascontiguousarray(lo[:, None] + (hi - lo)[:, None] * u)


def make_env(net, impl, mode, E_, seed, **kw):
    if mode == "series":
        ser = series_of(net)
        kw.update(series=ser, aux_bounds=np.array(((0, ser.shape[1] - 1),)))
    else:
        kw.update(exogenous="uniform", aux_bounds=np.array(((0, 1000),)))
    env = BatchedANMEnv(NETS[net](), "state", 1, 0.25, GAMMA, 100, costs_clipping=(1, 100), seed=seed, num_envs=E_, device=DEV,
                        tol=1e-6, impl=impl, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def device_reset(env, mask=None):
    return env.reset(options={"sampler": "device", "mask": mask})


def outputs(env, obs):
    return dict(obs=obs, state=env.state, reward=env.reward, e_loss=env.e_loss, penalty=env.penalty, terminated=env.terminated,
                soc=env.simulator.soc, timestep=env.timestep, reset_count=env._reset_count, nr_iters=env.simulator.nr_iters)


def stats(env):
    return {k: getattr(env, k) for k in STATS}


# ---- 1. truncation is the autoreset path / 4. the statistics ----------------------------------------------------------------
T1, N1, E1 = 5, 23, 4096


@functools.lru_cache(maxsize=None)
def autoreset_rollout(net, impl, mode):
    """A: limit T1 + statistics, autoreset.  B: no limit, same seed and env_offset, `terminated |= timestep >= T1` set by a
    torch op before every step.  Every output is compared after every step; returns A's record (host arrays [N1, E1])."""
    SEED, OFF = 2718, (1 << 32) - 300
    a = make_env(net, impl, mode, E1, SEED, autoreset=True, env_offset=OFF, max_episode_steps=T1, episode_stats=True)
    b = make_env(net, impl, mode, E1, SEED, autoreset=True, env_offset=OFF)
    oa, _ = device_reset(a)
    ob, _ = device_reset(b)
    assert torch.equal(oa, ob) and not bool(a.truncated.any())
    gen = torch.Generator(device=DEV).manual_seed(17)
    rec = {k: [] for k in ("ts_in", "term_in", "r", "term", "trunc", "ts") + STATS}
    for t in range(N1):
        act = uniform_actions(a, gen)
        b._term_u8 |= (b.timestep >= T1).to(torch.uint8)
        rec["ts_in"].append(a.timestep.clone())
        rec["term_in"].append(a.terminated.clone())
        oa, ra, ta, tra, _ = a.step(act)
        ob, _, _, trb, _ = b.step(act)
        xa, xb = outputs(a, oa), outputs(b, ob)
        for k in OUTPUTS:
            assert torch.equal(xa[k], xb[k]), "step %d: %s differs (%s, %s, %s)" % (t, k, net, impl, mode)
        assert tra is a.truncated and tra.dtype == torch.bool and not bool(trb.any())
        assert torch.equal(tra, a.timestep >= T1), "step %d: truncated" % t
        assert int(a.timestep.max()) <= T1
        for k, v in zip(("r", "term", "trunc", "ts"), (ra, ta, tra, a.timestep)):
            rec[k].append(v.clone())
        for k, v in stats(a).items():
            rec[k].append(v.clone())
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


def end_events(rec):
    """(collapses, truncations that are no collapse) over a record: real steps only (a real step leaves timestep > 0)"""
    real = rec["ts"] > 0
    fresh = real & (rec["ts"] != rec["ts_in"])                # (the absorbing no-op step leaves timestep as it was)
    collapse = fresh & rec["term"]
    limit = fresh & ~rec["term"] & (rec["ts"] == T1)
    return collapse, limit


@pytest.mark.parametrize("net,impl,mode", CASES)
def test_truncation_is_the_autoreset_path_bit_for_bit(net, impl, mode):
    rec = autoreset_rollout(net, impl, mode)
    collapse, limit = end_events(rec)
    print("%s %s %s: %d truncations, %d natural collapses, %d failed draws"
          % (net, impl, mode, limit.sum(), collapse.sum(), (rec["term"] & (rec["ts"] == 0)).sum()))
    assert limit.sum() >= 1 and collapse.sum() >= 1            # both kinds of episode end occur


@pytest.mark.parametrize("net,impl,mode", CASES)
def test_statistics_follow_the_specification_bit_for_bit(net, impl, mode):
    rec = autoreset_rollout(net, impl, mode)
    n_end = 0
    for e in range(E1):
        tr = episode.EpisodeTracker(GAMMA, T1)
        for t in range(N1):
            assert tr.timestep == rec["ts_in"][t, e]
            term_out = bool(rec["term"][t, e])
            n0 = tr.n_done
            ev, term = tr.call(bool(rec["term_in"][t, e]), True, float(rec["r"][t, e]), term_out, reset_converged=not term_out)
            n_end += tr.n_done - n0
            assert term == term_out and tr.timestep == rec["ts"][t, e] and tr.truncated == bool(rec["trunc"][t, e]), (e, t, ev)
            want = (tr.ret, tr.disc_ret, tr.last_ret, tr.last_disc_ret, tr.last_len, tr.n_done)
            have = tuple(rec[k][t, e] for k in STATS)
            assert want == have, (e, t, ev, want, have)          # == on float64 (no NaN here): bit for bit, up to the sign of a zero
            assert all(np.signbit(x) == np.signbit(y) for x, y in zip(want[:4], have[:4])), (e, t, ev, want, have)
    collapse, limit = end_events(rec)
    assert rec["episodes_done"][-1].sum() == n_end == collapse.sum() + limit.sum()
    assert collapse.sum() >= 1 and limit.sum() >= 1


# ---- 2. without autoreset: bookkeeping only -------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl,mode", CASES)
def test_without_autoreset_the_feature_is_bookkeeping_only(net, impl, mode):
    T, E_, SEED = 4, 512, 31
    a = make_env(net, impl, mode, E_, SEED, max_episode_steps=T, episode_stats=True)
    b = make_env(net, impl, mode, E_, SEED)
    device_reset(a)
    device_reset(b)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for t in range(3 * T):
        act = uniform_actions(a, gen)
        oa, _, _, tra, _ = a.step(act)
        ob, _, _, trb, _ = b.step(act)
        xa, xb = outputs(a, oa), outputs(b, ob)
        for k in OUTPUTS:
            assert torch.equal(xa[k], xb[k]), "step %d: %s differs (%s, %s, %s)" % (t, k, net, impl, mode)
        # goes to 1 at step T and stays (a collapsed environment is absorbing: its timestep and its flag stay as they were)
        assert torch.equal(tra, a.timestep >= T) and not bool(trb.any())
        alive = ~a.terminated
        assert bool((a.timestep[alive] == t + 1).all()) and bool(tra[alive].all()) == (t + 1 >= T)
    assert int(a.timestep.max()) == 3 * T and not bool(a._reset_count.ne(b._reset_count).any())
    ts, term = a.timestep, a.terminated
    want = (ts >= T).to(torch.int32) + (term & (ts != T)).to(torch.int32)   # the limit once, and a collapse that is not that very step
    assert torch.equal(a.episodes_done, want)
    first = ~(term & (ts < T))                                  # did not collapse before the limit: one episode of length T ...
    assert bool((a.episodes_done[first] >= 1).all())
    only = first & ~term
    assert bool((a.last_episode_length[only] == T).all()) and bool((a.episodes_done[only] == 1).all())
    print("%s %s %s: %d of %d collapsed on the way" % (net, impl, mode, int(term.sum()), E_))


# ---- 3. oracle replay across truncations -------------------------------------------------------------------------------------
def oracle_replay(env, network, T_lim, T, n_random, n_collapsed, seed, make_oracle, init_state):
    """tests/test_gpu_exo_uniform.py::oracle_replay with a time limit: the oracle is restarted from the specification's draw
    of the recorded epoch at a collapse AND at a truncation"""
    E_, dev = env.num_envs, env.device
    rc0 = env._reset_count.clone()
    state0, soc0 = env.state.clone(), env.simulator.soc.clone()
    gen = torch.Generator(device=dev).manual_seed(99)
    rec = {k: [] for k in ("a", "obs", "r", "term", "trunc", "it", "rc", "el", "pen")}
    for t in range(T):
        a = uniform_actions(env, gen)
        rec["rc"].append(env._reset_count.clone())
        obs, r, term, trunc, _ = env.step(a)
        for k, v in zip(("a", "obs", "r", "term", "trunc", "it", "el", "pen"),
                        (a, obs, r, term, trunc, env.simulator.nr_iters, env.e_loss, env.penalty)):
            rec[k].append(v.clone())
    collapsed = torch.nonzero(torch.stack(rec["term"])[: T - 2].any(dim=0))[:, 0].cpu().numpy()
    sample = np.unique(np.concatenate((np.random.default_rng(0).choice(E_, n_random, replace=False), collapsed[:n_collapsed])))
    idx = torch.as_tensor(sample, device=dev)
    R = {k: torch.stack([x[idx] for x in v]).cpu().numpy() for k, v in rec.items()}
    s0, c0, e0 = state0[idx].cpu().numpy(), soc0[idx].cpu().numpy(), (rc0[idx] - 1).cpu().numpy()
    n_reset = n_term = n_trunc = 0
    for j, e in enumerate(sample):
        ge = env.env_offset + int(e)
        epoch = [int(e0[j])]
        orc = make_oracle(ge, epoch)
        orc.load_state(s0[j], c0[j])
        t_ep = 0
        for t in range(T):
            if orc.terminated or t_ep >= T_lim:  # next-step autoreset: this call returns the first observation of a new episode
                epoch[0] = int(R["rc"][t][j])
                o, conv = orc.reset_to(init_state(ge, epoch[0]))
                t_ep = 0
                assert bool(R["term"][t][j]) == (not conv), (e, t)
                assert not R["trunc"][t][j], (e, t)
                assert R["r"][t][j] == 0.0 and R["el"][t][j] == 0.0 and R["pen"][t][j] == 0.0
                n_reset += 1
                if not conv:     # a draw whose first power flow does not converge: drawn again at the next call
                    assert not R["obs"][t][j].any()
                    orc.terminated = True
                    continue
            else:
                o, r, term = orc.step(R["a"][t][j])
                t_ep += 1
                assert term == bool(R["term"][t][j]), (e, t)
                assert bool(R["trunc"][t][j]) == (t_ep >= T_lim), (e, t)
                n_trunc += int(t_ep >= T_lim)
                npt.assert_allclose(R["r"][t][j], r, rtol=1e-9, atol=1e-12)
                if term:
                    n_term += 1
                    assert not R["obs"][t][j].any()
                    continue
                npt.assert_allclose(R["el"][t][j], orc.e_loss, rtol=1e-9, atol=1e-12)
                npt.assert_allclose(R["pen"][t][j], orc.penalty, rtol=1e-9, atol=1e-10)
            npt.assert_allclose(R["obs"][t][j], o, rtol=0, atol=1e-9, err_msg="env %d step %d" % (e, t))
            assert int(R["it"][t][j]) == orc.last["n_iter"], (e, t)
    return len(sample), n_term, n_trunc, n_reset


@pytest.mark.parametrize("mode", ["series", "uniform"])
def test_oracle_replay_across_truncations(mode):
    import anm_oracle as O

    E_, T_lim, T, SEED = 4096, 8, 30, 1234
    network = networks.anm6_network()
    if mode == "series":
        env = ANM6EasyVec(num_envs=E_, seed=SEED, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T_lim)
        env.check_actions = False
        env.reset(seed=SEED)
        model, ser = env.simulator.model, env._series

        def make_oracle(ge, epoch):
            return O.OracleEnv(network, sparse=False, tol=1e-6)

        def init_state(ge, ep):
            return rng.series_init_state(model, ser, SEED, ge, ep)
    else:
        env = make_env("anm6", "thread", "uniform", E_, SEED, autoreset=True, max_episode_steps=T_lim)
        env.reset(seed=SEED)
        model, lo, hi = env.simulator.model, env.exo_low, env.exo_high

        def make_oracle(ge, epoch):
            def spec(state):
                t1 = int(state[-1]) + 1
                return np.concatenate((rng.exo_uniform(SEED, ge, epoch[0], t1, lo, hi), [t1]))

            return O.OracleEnv(network, sparse=False, tol=1e-6, aux_bounds=((0, 1000),), next_vars=spec)

        def init_state(ge, ep):
            return rng.uniform_init_state(model, SEED, ge, ep, lo, hi)
    n, n_term, n_trunc, n_reset = oracle_replay(env, network, T_lim, T, 48, 16, SEED, make_oracle, init_state)
    print("replayed %d environments: %d collapses, %d truncations, %d resets" % (n, n_term, n_trunc, n_reset))
    assert n >= 48 and n_term >= 1 and n_trunc >= 48 and n_reset >= n_trunc - n


# ---- 5. two-launch equals one-launch -----------------------------------------------------------------------------------------
def test_two_launch_step_equals_one_launch_step_with_the_feature_on():
    E_, T, SEED = 16384, 5, 4321
    envs = [ANM6EasyVec(num_envs=E_, seed=SEED, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T, episode_stats=True,
                        straggler_after=sa) for sa in (6, None)]
    two, one = envs
    assert two._ws is not None and one._ws is None and two._aux_index is not None
    for env in envs:
        env.check_actions = False
        env.reset(seed=SEED)
    gen = torch.Generator(device=DEV).manual_seed(8)
    n_trunc = n_term = 0
    for t in range(4 * T + 2):
        a = uniform_actions(two, gen)
        o2, _, term, trunc, _ = two.step(a)
        o1, _, _, _, _ = one.step(a)
        x2, x1 = outputs(two, o2), outputs(one, o1)
        for k in OUTPUTS:
            assert torch.equal(x2[k], x1[k]), "step %d: %s" % (t, k)
        assert torch.equal(two.truncated, one.truncated), "step %d: truncated" % t
        for k in STATS:
            assert torch.equal(getattr(two, k), getattr(one, k)), "step %d: %s" % (t, k)
        n_trunc += int(trunc.sum())
        n_term += int(term.sum())
    assert n_trunc >= E_ and n_term >= 1
    assert int(two.episodes_done.sum()) >= n_trunc


# ---- 6. shards ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl,mode", [("thread", "series"), ("radial", "uniform"), ("mesh", "series")])
def test_two_shards_equal_the_whole_batch(impl, mode):
    E_, H, SEED, T = 4096, 2048, 77, 4
    kw = dict(autoreset=True, max_episode_steps=T, episode_stats=True)
    whole = make_env("anm6", impl, mode, E_, SEED, **kw)
    shards = [make_env("anm6", impl, mode, H, SEED, env_offset=k * H, **kw) for k in range(2)]
    ow, _ = device_reset(whole)
    os_ = [device_reset(s)[0] for s in shards]
    assert torch.equal(ow, torch.cat(os_))
    gen = torch.Generator(device=DEV).manual_seed(3)
    for t in range(3 * T):
        a = uniform_actions(whole, gen)
        ow, _, _, trw, _ = whole.step(a)
        outs = [s.step(a[k * H:(k + 1) * H].contiguous()) for k, s in enumerate(shards)]
        xw, xs = outputs(whole, ow), [outputs(s, o[0]) for s, o in zip(shards, outs)]
        for k in OUTPUTS:
            assert torch.equal(xw[k], torch.cat([x[k] for x in xs])), "step %d: %s" % (t, k)
        assert torch.equal(trw, torch.cat([o[3] for o in outs])), "step %d: truncated" % t
        for k in STATS:
            assert torch.equal(getattr(whole, k), torch.cat([getattr(s, k) for s in shards])), "step %d: %s" % (t, k)
    assert int(whole.episodes_done.min()) >= 2


# ---- 7. HIP-graph capture ----------------------------------------------------------------------------------------------------
def test_the_first_step_after_reset_is_captured_into_a_graph():
    E_, T, SEED = 1024, 4, 21
    envs = [ANM6EasyVec(num_envs=E_, seed=SEED, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T, episode_stats=True)
            for _ in range(2)]
    env, twin = envs
    for e in envs:
        e.check_actions = False
        e.reset(seed=SEED)
    gen = torch.Generator(device=DEV).manual_seed(2)
    acts = [uniform_actions(env, gen) for _ in range(2 * T)]
    buf = acts[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # the very first step: one stream, one launch, nothing allocated, no synchronisation
        env.step(buf)
    torch.cuda.synchronize()
    assert not bool(env.timestep.any())                      # capture does not execute
    n_trunc = 0
    for t, a in enumerate(acts):
        buf.copy_(a)
        g.replay()
        o2, r2, t2, tr2, _ = twin.step(a)
        x, y = outputs(env, env._state_obs), outputs(twin, o2)
        for k in OUTPUTS:
            assert torch.equal(x[k], y[k]), "replay %d: %s" % (t, k)
        assert torch.equal(env.truncated, tr2)
        for k in STATS:
            assert torch.equal(getattr(env, k), getattr(twin, k)), "replay %d: %s" % (t, k)
        n_trunc += int(tr2.sum())
    assert n_trunc >= E_ and int(env.episodes_done.min()) >= 1


# ---- 8. resets clear what they touch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", FAMILIES)
def test_resets_clear_what_they_touch(net, impl):
    E_, T = 256, 3
    env = make_env(net, impl, "series", E_, 9, max_episode_steps=T, episode_stats=True)
    device_reset(env)
    gen = torch.Generator(device=DEV).manual_seed(4)
    for _ in range(T + 1):
        env.step(uniform_actions(env, gen))
    alive = ~env.terminated
    assert bool(env.truncated[alive].all()) and bool((env.episode_return[alive] != 0).all()) and bool(alive.any())
    before = {k: getattr(env, k).clone() for k in STATS}
    trunc0, disc0, ts0 = env.truncated.clone(), env._episode_discount.clone(), env.timestep.clone()
    m = torch.arange(E_, device=DEV) % 3 == 0
    device_reset(env, m)
    keep = ~m
    assert not bool(env.truncated[m].any()) and torch.equal(env.truncated[keep], trunc0[keep])
    assert not bool(env.timestep[m].any()) and torch.equal(env.timestep[keep], ts0[keep])
    assert not bool(env.episode_return[m].any()) and not bool(env.episode_discounted_return[m].any())
    assert bool((env._episode_discount[m] == 1.0).all()) and torch.equal(env._episode_discount[keep], disc0[keep])
    for k in ("episode_return", "episode_discounted_return"):
        assert torch.equal(getattr(env, k)[keep], before[k][keep]), k
    for k in ("last_episode_return", "last_episode_discounted_return", "last_episode_length", "episodes_done"):
        assert torch.equal(getattr(env, k), before[k]), k      # what finished stays on record
    # ... and a reset from rows the caller gives does the same
    rows = env.sample_init_state()
    env.step(uniform_actions(env, gen))
    m2 = torch.arange(E_, device=DEV) % 3 == 1
    env.reset(options={"init_state": rows, "mask": m2})
    assert not bool(env.truncated[m2].any()) and not bool(env.episode_return[m2].any()) and bool((env._episode_discount[m2] == 1.0).all())
    assert bool((env.episode_return[m] != 0).all())            # the rows of the first mask took a step since


# ---- the host-hook path: the flag and the statistics, no autoreset ----------------------------------------------------------------
class HookEasy(ANM6EasyVec):
    """ANM6Easy through next_vars() on the host: the general step with `exo` given"""

    def __init__(self, **kw):
        self.P_loads = anm6easy_series()[:3]
        self.P_maxs = anm6easy_series()[3:]
        BatchedANMEnv.__init__(self, networks.anm6_network(), "state", 1, 0.25, GAMMA, 100, aux_bounds=np.array([[0, 95]]),
                               costs_clipping=(1, 100), **kw)


def test_the_host_hook_path_keeps_the_flag_and_the_statistics():
    E_, T = 128, 3
    env = HookEasy(num_envs=E_, device=DEV, seed=3, tol=1e-6, max_episode_steps=T, episode_stats=True)
    env.check_actions = False
    env.reset(seed=3)
    gen = torch.Generator(device=DEV).manual_seed(1)
    trs = [episode.EpisodeTracker(GAMMA, T) for _ in range(E_)]
    term_in = np.zeros(E_, dtype=bool)
    for t in range(2 * T):
        _, r, term, trunc, _ = env.step(uniform_actions(env, gen))
        r, term, trunc, ts = r.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(), env.timestep.cpu().numpy()
        for e, tr in enumerate(trs):
            tr.call(bool(term_in[e]), False, float(r[e]), bool(term[e]))
            assert tr.truncated == bool(trunc[e]) and tr.timestep == int(ts[e])
        term_in = term
        have = {k: getattr(env, k).cpu().numpy() for k in STATS}
        for e, tr in enumerate(trs):
            assert (tr.ret, tr.disc_ret, tr.last_ret, tr.last_disc_ret, tr.last_len, tr.n_done) == tuple(have[k][e] for k in STATS), (t, e)
    assert int(env.episodes_done.sum()) >= E_ - int(term.sum())


# ---- the NumPy adapter -------------------------------------------------------------------------------------------------------------
def test_numpy_vector_env_reports_finished_episodes():
    E_, T = 256, 3
    env = NumpyVectorEnv(ANM6EasyVec(num_envs=E_, seed=6, tol=1e-6, autoreset=True, device=DEV, max_episode_steps=T, episode_stats=True))
    env.reset(seed=6)
    r_np = np.random.default_rng(0)
    lo, hi = env.single_action_space.low, env.single_action_space.high
    ret, n_seen = np.zeros(E_), 0
    fresh = np.zeros(E_, dtype=bool)     # rows whose next call re-initialises them
    for t in range(3 * T + 2):
        _, r, term, trunc, info = env.step(lo + (hi - lo) * r_np.random((E_, len(lo))))
        ended = info["_episode"]
        assert ended.dtype == bool and ended.shape == (E_,)
        npt.assert_array_equal(ended, (term | trunc) & ~fresh)
        ret = np.where(fresh, 0.0, ret + r)
        npt.assert_allclose(info["episode"]["r"][ended], ret[ended], rtol=1e-12)
        assert (info["episode"]["l"][ended] <= T).all() and (info["episode"]["l"][~ended] == 0).all()
        assert np.isfinite(info["episode"]["d"]).all() and (info["episode"]["d"][~ended] == 0).all()
        n_seen += int(ended.sum())
        fresh = (term | trunc)
    assert n_seen >= 2 * E_
    plain = NumpyVectorEnv(ANM6EasyVec(num_envs=4, seed=6, autoreset=True, device=DEV))
    plain.reset(seed=6)
    assert "episode" not in plain.step(np.zeros((4, len(lo))) + (lo + hi) / 2)[4]


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_what_the_feature_refuses():
    env = make_env("anm6", "radial", "series", 64, 1, max_episode_steps=5)
    device_reset(env)
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    sim = env.simulator
    lib = sim.backend.lib
    # a batch view on a model with a limit: refused where it is bound, and the error names the view
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(sim._handle, C.byref(view)) != 0
    assert b"batch view" in lib.anm_last_error() and b"episode" in lib.anm_last_error()
    env.step(a)                                                    # the model is as it was
    # ... and a limit or buffers on a model that has a view bound
    plain = make_env("anm6", "radial", "series", 64, 1)
    psim = plain.simulator
    assert lib.anm_model_bind_view(psim._handle, C.byref(view)) == 0
    ser = series_of("anm6")
    bufs = _lib.EpisodeBuffers(truncated=env._trunc_u8.data_ptr())

    def cfg(**kw):
        return _lib.EnvConfigEpisode(K=1, gamma=GAMMA, clip_e_loss=1.0, clip_penalty=100.0, obs_low=None, obs_high=None,
                              series=ser.ctypes.data_as(_lib.c_double_p), period=ser.shape[1], **kw)

    for kw in (dict(max_episode_steps=5), dict(episode=C.pointer(bufs))):
        assert lib.anm_model_set_env(psim._handle, C.byref(cfg(**kw))) != 0, kw
        assert b"batch view" in lib.anm_last_error(), kw
    assert lib.anm_model_bind_view(psim._handle, None) == 0
    # an unknown tail marker; a negative limit; halves of a pair of buffers
    odd = cfg(max_episode_steps=5)
    C.c_int32.from_address(C.addressof(odd) + 4).value = 7
    assert lib.anm_model_set_env(psim._handle, C.byref(odd)) != 0 and b"tail" in lib.anm_last_error()
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg(max_episode_steps=-1))) != 0
    assert b"max_episode_steps" in lib.anm_last_error()
    half = _lib.EpisodeBuffers(ep_disc_return=env.reward.data_ptr())
    assert lib.anm_model_set_env(psim._handle, C.byref(cfg(episode=C.pointer(half)))) != 0
    assert b"ep_discount" in lib.anm_last_error()
    # a limit without the timestep buffer at step time
    args = list(env._step_args)
    args[3] = None
    rc = lib.anm_step_f64(sim._handle, env.num_envs, a.data_ptr(), None, None, *args, 0, env.rng_seed, env.env_offset,
                          env._reset_count_ptr, env._aux_index_ptr, env._ws_ref, env._opts_ref, None)
    assert rc != 0 and b"timestep" in lib.anm_last_error()
    # the public classes
    with pytest.raises(errors.ArgsError, match="max_episode_steps"):
        make_env("anm6", "radial", "series", 64, 1, max_episode_steps=0)
    from gym_anm_amd.envs import MixedBatchedANMEnv

    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv([dict(network=networks.anm6_network(), series=anm6easy_series())], [0, 0, 0, 0], device=DEV, max_episode_steps=5)
    # parameter classes are independent of the feature: allowed
    ok = make_env("anm6", "radial", "series", 64, 1, max_episode_steps=2, variants=[networks.anm6_network()],
                  env_variant=np.zeros(64, dtype=np.int32))
    device_reset(ok)
    for _ in range(2):
        _, _, _, trunc, _ = ok.step(a)
    assert bool(trunc[~ok.terminated].all())
