"""GPU tier: the uniform exogenous mode (``BatchedANMEnv(exogenous="uniform")``) -- loads and generator potentials drawn
inside the step kernels, P_i = fma(hi_i - lo_i, u_i, lo_i) MW, from the counter-based RNG.  From the outside in:
  1. the draws: the rows of ``sample_init_state()`` against the specification gym_anm_amd/rng.py, bit for bit, and the
     samplers inside the reset kernels of every family against those rows;
  2. the mode equals the host-hook path it replaces (``next_vars`` returning the specification's draws), bit for bit;
  3. oracle replay with autoreset on ANM6; 4. the 30-bus feeder at 16 384 environments against the oracle;
  5. sharding; 6. the distribution of the draws; 7. what the mode refuses."""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest
import torch
from scipy import stats

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.envs.anm_env import BatchedANMEnv

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AUX_BOUNDS = ((0, 1000),)          # above every step count used here: the bounds clip the observation only

NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0)}
CASES = [("anm6", "thread"), ("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial"), ("case30", "mesh")]


def make_env(net, impl, E_, seed, cls=BatchedANMEnv, exogenous="uniform", **kw):
    env = cls(NETS[net](), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(AUX_BOUNDS), costs_clipping=(1, 100), seed=seed,
              num_envs=E_, device=DEV, tol=1e-6, impl=impl, exogenous=exogenous, **kw)
    assert env.simulator.impl == impl
    env.check_actions = False
    return env


def model_base(env):
    return float(env.simulator.model.baseMVA)


def drawn_columns(model):
    """columns of a state row that hold the fused draws (load P, generator P and P_max), generator Q / storage SoC (affine
    maps the kernels contract as they please) and the step index"""
    D, nd = model.N_device, model.N_des
    fused = list(model.load_idx) + list(model.gen_idx) + [2 * D + nd + g for g in range(model.N_non_slack_gen)]
    loose = [D + k for k in model.gen_idx] + [2 * D + e for e in range(nd)]
    return fused, loose


# ---- 1. the draws --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,n_keys,custom", [("anm6", 10000, True), ("case30", 1500, False)])
def test_rows_of_the_sampler_against_the_specification(net, n_keys, custom):
    SEED, OFF = 0x0123456789ABCDE, (1 << 32) - n_keys // 3            # (the environment index crosses 2^32)
    kw = {}
    if custom:    # non-default ends, a degenerate interval among them
        kw = dict(exo_low=np.array([-4.5, -19.25, -1.0, 0.5, 7.0]), exo_high=np.array([-0.125, 0.0, -1.0, 29.75, 41.0]))
    env = make_env(net, "radial", n_keys, SEED, env_offset=OFF, **kw)
    model = env.simulator.model
    epochs = np.random.default_rng(3).integers(0, 2**31 - 1, n_keys).astype(np.int32)
    epochs[:8] = [0, 1, 2, 3, 2**31 - 2, 2**31 - 2, 7, 7]
    env._reset_count.copy_(torch.as_tensor(epochs))
    rows = env.sample_init_state().cpu().numpy()
    fused, loose = drawn_columns(model)
    rest = [k for k in range(rows.shape[1]) if k not in fused and k not in loose]
    span = {D_ + k: max(abs(model.dev_q_min[k]), abs(model.dev_q_max[k])) for D_ in [model.N_device] for k in model.gen_idx}
    span.update({2 * model.N_device + e: max(abs(model.dev_soc_min[k]), abs(model.dev_soc_max[k])) for e, k in enumerate(model.des_idx)})
    for e in range(n_keys):
        want = rng.uniform_init_state(model, SEED, OFF + e, int(epochs[e]), env.exo_low, env.exo_high)
        npt.assert_array_equal(rows[e, fused], want[fused], err_msg="env %d" % e)      # the fma draws: exactly
        npt.assert_array_equal(rows[e, rest], 0.0)                                    # zeros and aux = 0: exactly
        for c in loose:                                                               # lo + (hi - lo) u: one rounding
            assert abs(rows[e, c] - want[c]) <= 2.0**-52 * max(span[c], 1e-300), (e, c)
    lo_v = rng.uniform_init_state_v(model, SEED, OFF + np.arange(n_keys), epochs.astype(np.uint64), env.exo_low, env.exo_high)
    npt.assert_allclose(rows, lo_v, rtol=1e-15, atol=1e-14)
    assert int(env._reset_count.sum()) == int(epochs.astype(np.int64).sum())      # the epochs are not consumed


@pytest.mark.parametrize("net,impl", CASES)
def test_reset_kernels_draw_what_the_entry_point_draws(net, impl):
    E_ = 2048
    a, b = make_env(net, impl, E_, 99, env_offset=12345), make_env(net, impl, E_, 99, env_offset=12345)
    for rnd in range(3):
        mask = None if rnd == 0 else (torch.rand(E_, device=DEV) < 0.3)
        drawn = b.sample_init_state()
        todo = torch.ones(E_, dtype=torch.bool, device=DEV) if mask is None else mask.clone()
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
        assert not bool(a.state[:, -1].any())
    assert int(a._reset_count.min()) >= 1


def test_reset_from_given_rows_starts_a_new_episode_too():
    env = make_env("anm6", "radial", 512, 5)
    rows = env.sample_init_state()
    env.reset(options={"init_state": rows})
    assert bool((env._reset_count == 1).all())
    mask = torch.arange(512, device=DEV) % 3 == 0
    env.reset(options={"init_state": rows, "mask": mask})
    assert torch.equal(env._reset_count, 1 + mask.to(torch.int32))


# ---- 2. the mode equals the hook path it replaces ----------------------------------------------------------------------
class HookTask(BatchedANMEnv):
    """the same task through next_vars(): the specification's draws for step t + 1, aux = t + 1"""

    def next_vars(self, s_t):
        t = s_t[:, -1].cpu().numpy().astype(np.int64)
        out = np.zeros((self.num_envs, len(self.spec_low) + 1))
        for e in range(self.num_envs):
            out[e, :-1] = rng.exo_uniform(self.rng_seed, self.env_offset + e, int(self.spec_epoch[e]), int(t[e]) + 1,
                                          self.spec_low, self.spec_high)
            out[e, -1] = t[e] + 1
        return torch.as_tensor(out, device=self.device)


@pytest.mark.parametrize("net,impl", CASES)
def test_the_mode_equals_the_hook_path_bit_for_bit(net, impl):
    E_, T, SEED, OFF = 256, 20, 4242, (1 << 32) - 100
    uni = make_env(net, impl, E_, SEED, env_offset=OFF)
    hook = make_env(net, impl, E_, SEED, cls=HookTask, exogenous=None, env_offset=OFF)
    rows = uni.sample_init_state()
    uni.reset(options={"init_state": rows})
    hook.reset(options={"init_state": rows})
    hook.spec_low, hook.spec_high = uni.exo_low, uni.exo_high
    hook.spec_epoch = (uni._reset_count - 1).cpu().numpy()
    assert not hook.spec_epoch.any()
    assert torch.equal(uni.state, hook.state) and torch.equal(uni.simulator.soc, hook.simulator.soc)
    gen = torch.Generator(device=DEV).manual_seed(7)
    n_alive = 0
    for t in range(T):
        a = uniform_actions(uni, gen)
        ou, ru, tu, _, _ = uni.step(a)
        oh, rh, th, _, _ = hook.step(a)
        for name, x, y in (("obs", ou, oh), ("state", uni.state, hook.state), ("reward", ru, rh), ("e_loss", uni.e_loss, hook.e_loss),
                           ("penalty", uni.penalty, hook.penalty), ("terminated", tu, th),
                           ("nr_iters", uni.simulator.nr_iters, hook.simulator.nr_iters), ("soc", uni.simulator.soc, hook.simulator.soc)):
            assert torch.equal(x, y), "step %d: %s differs (%s, %s)" % (t, name, net, impl)
        n_alive += int((~tu).sum())
        alive = ~tu
        assert bool((uni.state[alive, -1] == t + 1).all())
    assert n_alive > E_ * T // 2       # (most environments are still being stepped, not sitting in the absorbing state)


# ---- 3. / 4. oracle replay -------------------------------------------------------------------------------------------------
def oracle_replay(net, env, T, n_random, n_collapsed, seed):
    """the twin of parity_common.headline_replay for this mode: a seeded sample of environments plus collapsed ones are
    replayed by OracleEnv(next_vars = the specification), restarted from rng.uniform_init_state at each autoreset.
    Returns (replayed, terminations, resets, rec)."""
    import anm_oracle as O

    network = NETS[net]()
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
    lo, hi = env.exo_low, env.exo_high
    n_reset = n_term = 0
    for j, e in enumerate(sample):
        ge = env.env_offset + int(e)
        epoch = [int(e0[j])]

        def spec(state):
            t1 = int(state[-1]) + 1
            return np.concatenate((rng.exo_uniform(seed, ge, epoch[0], t1, lo, hi), [t1]))

        orc = O.OracleEnv(network, sparse=False, tol=1e-6, aux_bounds=AUX_BOUNDS, next_vars=spec)
        orc.load_state(s0[j], c0[j])
        for t in range(T):
            if orc.terminated:  # Gymnasium next-step autoreset: this call returns the first observation of a new episode
                epoch[0] = int(R["rc"][t][j])
                o, conv = orc.reset_to(rng.uniform_init_state(model, seed, ge, epoch[0], lo, hi))
                assert bool(R["term"][t][j]) == (not conv), (e, t)
                assert R["r"][t][j] == 0.0 and R["el"][t][j] == 0.0 and R["pen"][t][j] == 0.0
                n_reset += 1
                if not conv:     # a draw whose first power flow does not converge: drawn again at the next call
                    assert not R["obs"][t][j].any()
                    orc.terminated = True
                    continue
            else:
                o, r, term = orc.step(R["a"][t][j])
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
    return len(sample), n_term, n_reset, rec


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_oracle_replay_with_autoreset_on_anm6(impl):
    env = make_env("anm6", impl, 4096, 1234, autoreset=True)
    n, n_term, n_reset, _ = oracle_replay("anm6", env, 24, 48, 16, 1234)
    print("replayed %d environments: %d terminations, %d resets" % (n, n_term, n_reset))
    assert n >= 48 and n_term >= 1 and n_reset >= 1


def test_the_feeder_at_its_bench_size_against_the_oracle():
    """config 4: the 30-bus feeder, 16 384 environments, impl radial, 12 steps; 48 seeded environments plus every collapsed one"""
    E_, T, SEED = 16384, 12, 2024
    env = make_env("case30", "radial", E_, SEED, autoreset=True)
    n, n_term, n_reset, rec = oracle_replay("case30", env, T, 48, None, SEED)
    iters = torch.stack(rec["it"]).double()
    print("replayed %d environments: %d terminations, %d resets; mean Newton iterations %.2f, collapsed share %.2e"
          % (n, n_term, n_reset, float(iters.mean()), float(torch.stack(rec["term"]).double().mean())))
    assert n >= 48
    # state rows of the whole batch: load dev_p and gen_p_max are the vectorised specification for every environment that
    # has not been reset on the way, within the project's injection tolerance: 1e-12 relative to the base power, i.e. 1e-12
    # p.u. absolute (parity_common.check_transition_against_golden) = 1e-12 baseMVA in the MW of a state row.  (Relative to
    # the VALUE it cannot hold for a specification that is itself one rounding of lo + (hi - lo) u off: a draw of 2e-4 MW
    # on [-10, 0] carries the rounding of a number near 10, 4e-12 of the draw.)
    inj_tol = 1e-12 * model_base(env)
    model = env.simulator.model
    D, nd = model.N_device, model.N_des
    first_epoch = (rec["rc"][0] - 1).cpu().numpy().astype(np.uint64)
    never_reset = ~torch.stack(rec["term"]).any(dim=0).cpu().numpy()
    assert never_reset.mean() > 0.9
    envs = np.arange(E_, dtype=np.uint64)
    for t in (0, 5, T - 1):
        want = rng.exo_uniform_v(SEED, envs, first_epoch, np.uint64(t + 1), env.exo_low, env.exo_high)
        st = rec["state"][t].cpu().numpy()
        npt.assert_array_equal(st[never_reset, -1], t + 1)
        for s, k in enumerate(model.load_idx):
            npt.assert_allclose(st[never_reset, k], want[never_reset, s], rtol=0, atol=inj_tol)
        for g in range(model.N_non_slack_gen):
            npt.assert_allclose(st[never_reset, 2 * D + nd + g], want[never_reset, model.N_load + g], rtol=0, atol=inj_tol)


# ---- 5. sharding -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_two_shards_equal_the_whole_batch(impl):
    E_, H, SEED = 16384, 8192, 77
    whole = make_env("anm6", impl, E_, SEED, autoreset=True)
    shards = [make_env("anm6", impl, H, SEED, autoreset=True, env_offset=k * H) for k in range(2)]
    ow, _ = whole.reset(seed=SEED)
    os_ = [s.reset(seed=SEED)[0] for s in shards]
    assert torch.equal(ow, torch.cat(os_))
    gen = torch.Generator(device=DEV).manual_seed(3)
    n_reset = 0
    for t in range(10):
        a = uniform_actions(whole, gen)
        rc = whole._reset_count.clone()
        ow, rw, tw, _, _ = whole.step(a)
        outs = [s.step(a[k * H:(k + 1) * H].contiguous()) for k, s in enumerate(shards)]
        n_reset += int((whole._reset_count - rc).sum())
        for name, x, ys in (("obs", ow, [o[0] for o in outs]), ("reward", rw, [o[1] for o in outs]), ("terminated", tw, [o[2] for o in outs]),
                            ("state", whole.state, [s.state for s in shards]), ("soc", whole.simulator.soc, [s.simulator.soc for s in shards]),
                            ("reset_count", whole._reset_count, [s._reset_count for s in shards]),
                            ("nr_iters", whole.simulator.nr_iters, [s.simulator.nr_iters for s in shards])):
            assert torch.equal(x, torch.cat(ys)), "step %d: %s" % (t, name)
    assert n_reset >= 1


# ---- 6. distribution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial")])
def test_every_unit_is_uniform_on_its_interval(net, impl):
    E_ = 16384
    env = make_env(net, impl, E_, 31337)
    model = env.simulator.model
    lo, hi = env.exo_low, env.exo_high
    D, nd = model.N_device, model.N_des
    cols = list(model.load_idx) + [2 * D + nd + g for g in range(model.N_non_slack_gen)]
    rows = env.sample_init_state().cpu().numpy()             # the step stream at index 0: the draws themselves
    for i, c in enumerate(cols):
        x = rows[:, c]
        assert lo[i] <= x.min() and x.max() < hi[i], i
        assert stats.kstest(x, "uniform", args=(lo[i], hi[i] - lo[i])).pvalue > 1e-3, i
    c_ = np.corrcoef(rows[:, cols].T)
    assert np.abs(c_ - np.eye(len(cols))).max() < 0.04
    # ... and along an episode: the rows of step 3 (clip(draw / baseMVA) * baseMVA: the draw within two roundings)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(1)
    for t in range(3):
        _, _, term, _, _ = env.step(uniform_actions(env, gen))
    alive = (~term).cpu().numpy()
    st = env.state.cpu().numpy()[alive]
    print("alive at step 3: %d of %d" % (alive.sum(), E_))
    assert alive.mean() > 0.9
    if alive.mean() > 0.999:       # (conditioning on survival would bias the marginals where collapses are not rare)
        for i, c in enumerate(cols):
            x = st[:, c]
            assert lo[i] * (1 + 1e-12) <= x.min() and x.max() <= hi[i] * (1 + 1e-12), i
            assert stats.kstest(x, "uniform", args=(lo[i], hi[i] - lo[i])).pvalue > 1e-3, i
    assert abs(np.corrcoef(rows[alive, cols[0]], st[:, cols[0]])[0, 1]) < 0.04      # step 0 against step 3


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_what_the_mode_refuses():
    env = make_env("anm6", "radial", 64, 1)
    env.reset()
    a = uniform_actions(env, torch.Generator(device=DEV).manual_seed(1))
    exo = torch.zeros((64, 5), dtype=torch.float64, device=DEV)
    aux = torch.zeros((64, 1), dtype=torch.float64, device=DEV)
    with pytest.raises(errors.HipExtensionError, match="exo and aux_next must be NULL"):
        env._step_call(a.data_ptr(), exo.data_ptr(), aux.data_ptr())
    sim = env.simulator
    lib = sim.backend.lib
    # a batch view
    view = _lib.BatchView(env_index=None)
    assert lib.anm_model_bind_view(sim._handle, C.byref(view)) == 0
    with pytest.raises(errors.HipExtensionError, match="batch view"):
        env._step_call(a.data_ptr(), None, None)
    with pytest.raises(errors.HipExtensionError, match="batch view"):
        env.reset()
    assert lib.anm_model_bind_view(sim._handle, None) == 0
    env.reset()
    env.step(a)
    # the task itself: K = 1, no series, finite ordered ends, no parameter classes
    n = sim.N_load + sim.N_non_slack_gen
    bad = [dict(K=2), dict(series=np.zeros((n, 4)), period=4), dict(lo=np.full(n, -np.inf)), dict(lo=np.ones(n), hi=np.zeros(n))]
    for b in bad:
        lo, hi = (np.ascontiguousarray(b.get(k, d), dtype=np.float64) for k, d in (("lo", env.exo_low), ("hi", env.exo_high)))
        ser = b.get("series")
        cfg = _lib.EnvConfig(K=b.get("K", 1), gamma=0.9, clip_e_loss=1.0, clip_penalty=100.0, obs_low=None, obs_high=None,
                             series=None if ser is None else ser.ctypes.data_as(_lib.c_double_p), period=b.get("period", 0),
                             exo_mode=_lib.EXO_UNIFORM, exo_low=lo.ctypes.data_as(_lib.c_double_p), exo_high=hi.ctypes.data_as(_lib.c_double_p))
        assert lib.anm_model_set_env(sim._handle, C.byref(cfg)) != 0, b
        assert b"uniform exogenous mode" in lib.anm_last_error(), b
    with pytest.raises(errors.EnvInitializationError, match="parameter classes"):
        make_env("anm6", "radial", 64, 1, variants=[networks.anm6_network()], env_variant=np.zeros(64, dtype=np.int32))
    with pytest.raises(errors.EnvInitializationError, match="K = 1"):
        BatchedANMEnv(networks.anm6_network(), "state", 0, 0.25, 0.995, 100, num_envs=4, device=DEV, exogenous="uniform")
