"""GPU tier: guard bands around every per-environment buffer -- the kernels write only their rows (tests/guard_common.py).

Every case builds A under the guarded allocator and B plain, from the same seed and with the same arguments, and runs
both through the same short closed loop: a device reset, six steps with actions over the whole Box (some environments are
marked terminated on the way in: the in-kernel reset where the case has autoreset, the absorbing row where not), a
masked device reset, ``sample_init_state(raw=True)``, a masked reset from given rows and a step after it.  Two assertions,
after the reset and after every call:
  * ``registry.check()`` is empty: no byte of a guard changed (the WRITE side);
  * every output of A equals B's bit for bit: 0xFF guards read as NaN / -1 / 255, so a read past the rows that matters shows
    as a difference (the READ side).
Batch sizes are the smallest at which a tail exists: 1, 63, 65, 165 (thread-per-environment family: two full wavefronts and
a partial one) and 1, 9, 41 (lane-group families); every case runs at every size of its family.  Which kernel a case
launches is read off launch_step / anm_reset_f64 / launch_lane_groups in csrc/anm_capi.hip and named in the case's id; for
k_step_rows_map and k_step_general_fc under the map the name is asserted from the profiler."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, networks
from gym_anm_amd.agents import MPCAgentExpected, MPCAgentPerfect, MPCAgentPerfectChain, MPCAgentPerfectStream
from gym_anm_amd.envs import ANM6EasyVec, MixedBatchedANMEnv
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.simulator import BatchedSimulator

from guard_common import GuardRegistry
from test_gpu_io_f32 import LIST_OBS, NETS, STATS, device_reset, f64_outputs
from test_gpu_io_map import FULL_MAP, ROLL, make_env, unit_actions
from test_gpu_mixed_env import make_tasks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SEED = 2718
E_OF = {"thread": (1, 63, 65, 165), "radial": (1, 9, 41), "mesh": (1, 9, 41)}
GROUP_FAMILIES = [("anm6", "radial"), ("anm6", "mesh"), ("case30", "radial"), ("case30", "mesh")]


# ---- the pair, its outputs, the closed loop ---------------------------------------------------------------------------------
def pair(build):
    reg = GuardRegistry()
    with reg.guarding():
        a = build()
    b = build()
    for env in (a, b):
        env.check_actions = False
    return reg, a, b


def assert_guarded(reg, *tensors):
    """these tensors of A are payloads of the registry: the case guards what it says it guards"""
    payloads = {g.payload.data_ptr() for g in reg.buffers if g.nbytes}
    for t in tensors:
        assert t is None or t.numel() == 0 or t.data_ptr() in payloads, (tuple(t.shape), t.dtype)


def bits(x):
    return x.contiguous().view(torch.uint8)


def outputs(env, obs):
    """everything a kernel writes for this environment, by name (the raw buffers too: rows a kernel leaves unwritten are the
    same on both sides)"""
    sim = env.simulator
    out = dict(f64_outputs(env), obs=obs, reward=env.reward, state_buf=env._state_buf, state_obs=env._state_obs, conv=env._conv_u8)
    if env.episode_stats:
        out.update({k: getattr(env, k) for k in STATS}, episode_discount=env._episode_discount)
    for name, t in (("exo_z", env.exo_z), ("exo_forecast", env.exo_forecast), ("aux_index", env._aux_index), ("state_same", env._state_same),
                    ("obs_buf", env._obs_buf), ("full", sim.full if (env._need_full or env._need_full_reset) else None)):
        if t is not None:
            out[name] = t
    return out


RAW = ("state_buf", "state_same")      # which rows are left unwritten: the same only where both sides launch the same kernels


def same(a, b, oa, ob, where, raw=True):
    xa, xb = outputs(a, oa), outputs(b, ob)
    assert list(xa) == list(xb)
    for k in xa:
        if k in RAW and not raw:
            continue
        assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape and torch.equal(bits(xa[k]), bits(xb[k])), \
            "%s: %s of the guarded environment differs from the plain one's" % (where, k)


def env_tensors(env):
    sim = env.simulator
    return [env._state_buf, env._state_obs, env.reward, env.e_loss, env.penalty, env._term_u8, env.timestep, env._conv_u8, env._reset_count,
            env._trunc_u8, env.exo_z, env.exo_forecast, env._aux_index, env._state_same, env._obs_buf if env._obs_fused else None,
            sim.soc, sim.full, sim.nr_iters] + ([getattr(env, k) for k in STATS] + [env._episode_discount] if env.episode_stats else [])


def actions(env, gen):
    """over the whole Box, in the environment's io_dtype; under the map u in [-1.25, 1.25] (a fifth meets the clamp)"""
    if env._map_act is not None:
        return unit_actions(env, gen)
    lo, hi = (torch.as_tensor(x, device=DEV) for x in (env.action_space.low, env.action_space.high))
    u = lo.double() + (hi.double() - lo.double()) * torch.rand((env.num_envs, lo.numel()), generator=gen, dtype=F64, device=DEV)
    return torch.minimum(torch.maximum(u.to(env.io_dtype), lo), hi).contiguous()


def both_reset(reg, a, b, where, raw=True, **options):
    """the same reset() on A -- the tensors it is handed guarded, and what the call allocates itself -- and on B"""
    with reg.guarding():
        oa, _ = a.reset(options={k: reg.like(v) if torch.is_tensor(v) else v for k, v in options.items()})
    ob, _ = b.reset(options=dict(options))
    same(a, b, oa, ob, where, raw)
    reg.assert_intact(where)


def both_step(reg, a, b, u, where, raw=True):
    oa, ob = a.step(reg.like(u))[0], b.step(u)[0]
    same(a, b, oa, ob, where, raw)
    reg.assert_intact(where)


def exercise(reg, a, b, where, n_steps=6, rows=None):
    E_ = a.num_envs
    assert_guarded(reg, *env_tensors(a))
    if rows is None:
        both_reset(reg, a, b, where + ": reset", sampler="device")
    else:
        both_reset(reg, a, b, where + ": reset", init_state=rows)
    gen = torch.Generator(device=DEV).manual_seed(17)
    for t in range(n_steps):
        if t == 2:                       # terminated on the way in: reset inside the kernel (autoreset) or the absorbing row
            for env in (a, b):
                env._term_u8[::4] = 1
        both_step(reg, a, b, actions(a, gen), "%s: step %d" % (where, t))
    if a.autoreset:
        assert int(a._reset_count.min()) >= 1, where
    idx = torch.arange(E_, device=DEV)
    if rows is None:
        both_reset(reg, a, b, where + ": masked reset (device sampler)", sampler="device", mask=idx % 3 == 0)
        with reg.guarding():
            rows_a, words_a = a.sample_init_state(raw=True)
        rows, words_b = b.sample_init_state(raw=True)
        assert torch.equal(bits(rows_a), bits(rows)) and torch.equal(words_a, words_b), where + ": sample_init_state"
        reg.assert_intact(where + ": sample_init_state")
    both_reset(reg, a, b, where + ": masked reset (given rows)", init_state=rows, mask=idx % 2 == 0)
    both_step(reg, a, b, actions(a, gen), where + ": step after the resets")


def run_case(build, family, where, **kw):
    for E_ in E_OF[family]:
        reg, a, b = pair(lambda: build(E_))
        exercise(reg, a, b, "%s, E = %d" % (where, E_), **kw)


# ---- the thread-per-environment family -----------------------------------------------------------------------------------------
def easy(E_, **kw):
    return ANM6EasyVec(num_envs=E_, device=DEV, seed=SEED, tol=1e-6, **kw)


def thread_env(mode, **kw):
    return lambda E_: make_env("anm6", "thread", mode, E_, SEED, **kw)


THREAD_CASES = {
    # the coalesced-row kernels (series mode, "state" observation)
    "k_step_rows": lambda E_: easy(E_, autoreset=True),
    "k_step_rows_ep": lambda E_: easy(E_, **ROLL),
    "k_step_rows_io32": lambda E_: easy(E_, io_dtype=F32, autoreset=True),
    "k_step_rows_io32-ep": lambda E_: easy(E_, io_dtype=F32, **ROLL),
    "k_step_rows_map-f64": lambda E_: easy(E_, **FULL_MAP, **ROLL),
    "k_step_rows_map-f32": lambda E_: easy(E_, io_dtype=F32, **FULL_MAP, **ROLL),
    # the general step kernel
    "k_step_general-uniform": thread_env("uniform", **ROLL),
    "k_step_general-uniform-f32": thread_env("uniform", io_dtype=F32, **ROLL),
    "k_step_general-list": thread_env("series", observation=LIST_OBS, **ROLL),
    "k_step_general-list-f32": thread_env("series", observation=LIST_OBS, io_dtype=F32, **ROLL),
    "k_step_general-track_full": thread_env("series", track_full=True, **ROLL),
    "k_step_general-uniform-map": thread_env("uniform", **FULL_MAP, **ROLL),
    "k_step_general-list-map-f32": thread_env("series", observation=LIST_OBS, io_dtype=F32, **FULL_MAP, **ROLL),
}
# the general step kernel with the forecast: white and AR(1) noise, H = 3, both dtypes, with and without the map
THREAD_CASES.update({"k_step_general_fc-%s-%s%s" % (mode, "f32" if dtype == F32 else "f64", "-map" if maps else ""):
                     thread_env(mode, io_dtype=dtype, **maps, **ROLL)
                     for mode in ("noise", "noise_corr") for dtype in (F64, F32) for maps in ({}, FULL_MAP)})


@pytest.mark.parametrize("case", sorted(THREAD_CASES))
def test_thread_family_writes_only_its_rows(case):
    build = THREAD_CASES[case]
    probe = build(2)
    if case == "k_step_rows":
        assert probe._state_same is not None            # the fast path with the rows it leaves unwritten
    if case.startswith("k_step_rows"):
        assert probe._aux_index is not None and not probe._need_full and probe._gather is None
    else:
        assert probe._aux_index is None or probe._need_full or probe._obs_fused
    assert (probe.forecast_horizon is not None) == case.startswith("k_step_general_fc")
    run_case(build, "thread", case)


class HookTask(BatchedANMEnv):
    """K = 2 auxiliary variables and a next_vars() hook: the general step kernel fed with exo and aux rows from the host side"""

    def next_vars(self, s_t):
        tab = torch.as_tensor(anm6easy_series(), device=s_t.device)
        t = torch.remainder(s_t[:, -2] + 1, 96).long()
        w = 0.5 + 0.5 * torch.cos(0.3 * (s_t[:, -1] + 1.0))
        return torch.cat((tab[:3, t].T, tab[3:, t].T * w[:, None], t[:, None].double(), (s_t[:, -1] + 1.0)[:, None]), 1)


def hook_rows(E_):
    tab, r = anm6easy_series(), np.random.default_rng(12)
    s0, t0 = np.zeros((E_, 19)), r.integers(0, 96, E_)
    s0[:, [1, 3, 5]], s0[:, [2, 4]], s0[:, 15:17] = tab[:3, t0].T, tab[3:, t0].T, tab[3:, t0].T
    s0[:, 14], s0[:, 17], s0[:, 18] = r.uniform(0, 100, E_), t0, r.integers(0, 50, E_)
    return torch.as_tensor(s0, device=DEV)


def test_thread_family_hook_task_with_two_aux_variables():
    """k_step_general, host-hook task, K = 2 (no autoreset: the device sampler needs a series-mode task)"""
    for E_ in E_OF["thread"]:
        build = lambda: HookTask(networks.anm6_network(), "state", 2, 0.25, 0.995, 100, aux_bounds=np.array([[0, 95], [0, 1e6]]),  # noqa: E731
                                 costs_clipping=(1, 100), seed=SEED, num_envs=E_, device=DEV, tol=1e-6, impl="thread",
                                 max_episode_steps=3, episode_stats=True)
        reg, a, b = pair(build)
        assert a.state_N == 19 and a._aux_index is None
        exercise(reg, a, b, "hook task, E = %d" % E_, rows=hook_rows(E_))


def kernel_names(env):
    from torch.profiler import ProfilerActivity, profile

    env.check_actions = False
    device_reset(env)
    u = actions(env, torch.Generator(device=DEV).manual_seed(1))
    env.step(u)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        env.step(u)
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if "k_step" in e.key or "k_radial" in e.key or "k_mesh" in e.key]


def test_the_matrix_launches_the_kernels_it_names():
    """once for k_step_rows_map and once for k_step_general_fc under the map: the cases above cannot fall back to another
    kernel without this failing (the other names follow from the same dispatch)"""
    for case, kernel in (("k_step_rows_map-f32", "k_step_rows_map"), ("k_step_general_fc-noise_corr-f64-map", "k_step_general_fc")):
        reg = GuardRegistry()
        with reg.guarding():
            env = THREAD_CASES[case](65)
        names = kernel_names(env)
        print(case, names)
        assert len(names) == 1 and kernel in names[0], names
        reg.assert_intact(case)


# ---- the two-launch step ---------------------------------------------------------------------------------------------------------
# searched with the unguarded one-launch twin over seeds 0 ... 39 at E = 165 (device reset, the 8 steps of the test): seeds 3, 7,
# 9, 19, 27 and 36 leave 4 solves running after 6 iterations in one step, no seed more; seed 9 does in the very first step
SEED_STRAGGLERS = 9
R_SMALL = 3


@pytest.mark.parametrize("small", [False, True], ids=["as-constructed", "small-workspace"])
def test_two_launch_step(small):
    """k_step_rows_ep stopping at 6 iterations, k_step_stragglers, k_step_scatter: A (two launches, guarded) against the
    one-launch twin, bit for bit as tests/test_gpu_parity.py has it.  small: the workspace is a guarded buffer of exactly
    8 + R rec + (R + 1) // 2 doubles for R = 3 records, so the guard begins where the stated capacity ends -- and at E = 165
    some step leaves MORE than 3 solves running after 6 iterations (asserted from the twin's nr_iters)."""
    for E_ in E_OF["thread"]:
        kw = dict(num_envs=E_, device=DEV, seed=SEED_STRAGGLERS, tol=1e-6, **ROLL)
        reg = GuardRegistry()
        with reg.guarding():
            two = ANM6EasyVec(straggler_after=6, **kw)
        one = ANM6EasyVec(straggler_after=None, **kw)
        assert two._ws is not None and one._ws is None
        assert_guarded(reg, two._ws_buf, *env_tensors(two))
        if small:
            rec = two.simulator.backend.lib.anm_step_ws_record_doubles()
            n = 8 + R_SMALL * rec + (R_SMALL + 1) // 2
            two._ws_buf = reg.zeros(n, dtype=F64, device=DEV)
            two._ws = _lib.StepWs(two._ws_buf.data_ptr(), n, 6, -1)
            two._ws_ref = C.byref(two._ws)
        for env in (two, one):
            env.check_actions = False
        where = "two-launch step (%s), E = %d" % ("small workspace" if small else "as constructed", E_)
        both_reset(reg, two, one, where + ": reset", raw=False, sampler="device")
        gen = torch.Generator(device=DEV).manual_seed(6)
        most = 0
        for t in range(8):
            both_step(reg, two, one, actions(two, gen), "%s: step %d" % (where, t), raw=False)
            most = max(most, int((one.simulator.nr_iters > 6).sum()))
        print("%s: at most %d solves still running after 6 iterations in one step" % (where, most))
        if E_ == 165:
            assert most > R_SMALL, most


# ---- the lane-group families ---------------------------------------------------------------------------------------------------------
GROUP_MODES = {"series": dict(mode="series"), "uniform": dict(mode="uniform"), "noise_corr-forecast": dict(mode="noise_corr"),
               "list": dict(mode="series", observation=LIST_OBS)}


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("maps", [{}, FULL_MAP], ids=["plain", "IoMapped"])
@pytest.mark.parametrize("task", sorted(GROUP_MODES))
@pytest.mark.parametrize("net,impl", GROUP_FAMILIES)
def test_lane_group_families_write_only_their_rows(net, impl, task, maps, dtype):
    """k_radial / k_mesh, plain and IoMapped<JT>: step (mode 2), the reset kernels, the masked resets"""
    kw = dict(GROUP_MODES[task])
    mode = kw.pop("mode")
    run_case(lambda E_: make_env(net, impl, mode, E_, SEED, io_dtype=dtype, **kw, **maps, **ROLL), impl,
             "%s %s %s %s %s" % (net, impl, task, "mapped" if maps else "plain", dtype))


# ---- the unfused list observation: anm_gather_obs_f64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial")])
def test_unfused_list_observation(net, impl):
    def build(E_):
        env = make_env(net, impl, "series", E_, SEED, observation=LIST_OBS, fuse_observation=False, autoreset=True, max_episode_steps=3)
        assert not env._obs_fused and env._need_full
        return env

    run_case(build, impl, "unfused list %s %s" % (net, impl))


# ---- a mixed batch: k_step_view ----------------------------------------------------------------------------------------------------
def mixed_outputs(env):
    return dict(state=env.state, obs=env._obs, soc=env.soc, reward=env.reward, e_loss=env.e_loss, penalty=env.penalty, terminated=env._term_u8,
                conv=env._conv_u8, timestep=env.timestep, nr_iters=env.nr_iters, reset_count=env._reset_count, truncated=env._truncated)


def test_mixed_batch_writes_only_its_rows():
    """k_step_view: two thread-family tasks of different topologies (ANM6 and the 3-bus loop), 9 environments.  The constructor
    of MixedBatchedANMEnv allocates every array a kernel writes through torch.zeros; torch.as_tensor makes only what the
    kernels read (row indices, action bounds).  Guards stand around the whole padded arrays."""
    tasks, env_task = make_tasks()[:2], np.arange(9) % 2
    kw = dict(device=DEV, seed=SEED, tol=1e-6, autoreset=True, streams=False)
    reg = GuardRegistry()
    with reg.guarding():
        a = MixedBatchedANMEnv(tasks, env_task, **kw)
    b = MixedBatchedANMEnv(tasks, env_task, **kw)
    assert a.impls == ["thread", "thread"] and a.tasks[0].simulator.model.N_bus != a.tasks[1].simulator.model.N_bus
    assert_guarded(reg, *mixed_outputs(a).values())

    def check(where):
        xa, xb = mixed_outputs(a), mixed_outputs(b)
        for k in xa:
            assert torch.equal(bits(xa[k]), bits(xb[k])), "%s: %s differs" % (where, k)
        reg.assert_intact(where)

    for env in (a, b):
        env.check_actions = False
    with reg.guarding():
        a.reset(seed=SEED)
    b.reset(seed=SEED)
    check("reset")
    lo, hi = torch.as_tensor(a.action_space.low, device=DEV), torch.as_tensor(a.action_space.high, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for t in range(7):
        if t == 2:
            for env in (a, b):
                env._term_u8[::4] = 1
        u = lo + (hi - lo) * torch.rand((9, a.A), generator=gen, dtype=F64, device=DEV)
        a.step(reg.like(u))
        b.step(u)
        check("step %d" % t)
    assert int(a._reset_count.max()) >= 2
    mask = torch.arange(9, device=DEV) % 3 == 0
    with reg.guarding():
        a.reset(options={"mask": reg.like(mask)})
    b.reset(options={"mask": mask})
    check("masked reset")


# ---- Simulator.transition (mode 0) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,impl", [("anm6", "thread")] + GROUP_FAMILIES)
def test_transition_writes_only_its_rows(net, impl):
    for E_ in E_OF[impl]:
        reg = GuardRegistry()
        kw = dict(num_envs=E_, device=DEV, tol=1e-8, impl=impl)
        with reg.guarding():
            a = BatchedSimulator(NETS[net](), 0.25, 100, **kw)
        b = BatchedSimulator(NETS[net](), 0.25, 100, **kw)
        assert a.impl == impl
        m, r = a.model, np.random.default_rng(E_)
        U = lambda lo, hi: torch.as_tensor(lo + (hi - lo) * r.random((E_, len(lo))), device=DEV)  # noqa: E731
        base = m.baseMVA
        pl = U(m.dev_p_min[m.load_idx] * base, 0 * m.dev_p_max[m.load_idx])
        pp = U(0 * m.dev_p_max[m.gen_idx], m.dev_p_max[m.gen_idx] * base)
        ps = U(m.dev_p_min[m.setp_idx] * base, m.dev_p_max[m.setp_idx] * base)
        qs = U(m.dev_q_min[m.setp_idx] * base, m.dev_q_max[m.setp_idx] * base)
        pl[-1] *= 40.0                                   # one hopeless case: the solve runs to its cap
        soc = U(m.dev_soc_min[m.des_idx], m.dev_soc_max[m.des_idx])
        a.soc.copy_(soc)
        b.soc.copy_(soc)
        names = ("full", "soc", "reward", "e_loss", "penalty", "_conv_u8", "nr_iters")
        assert_guarded(reg, *(getattr(a, k) for k in names))
        a.transition(*(reg.like(x) for x in (pl, pp, ps, qs)))
        b.transition(pl, pp, ps, qs)
        for k in names:
            assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), "%s %s E = %d: %s" % (net, impl, E_, k)
        reg.assert_intact("transition %s %s E = %d" % (net, impl, E_))


# ---- k_mpc ---------------------------------------------------------------------------------------------------------------------------
N_MPC = 3
RHO = (0.9, 0.5, 0.0, 0.8, 0.99)
NOISE = dict(exogenous="series_noise", exo_noise=2.0)
MPC_CASES = {"perfect": (MPCAgentPerfect, {}), "stream": (MPCAgentPerfectStream, NOISE), "chain": (MPCAgentPerfectChain, dict(NOISE, exo_corr=RHO)),
             "expected": (MPCAgentExpected, dict(NOISE, exo_corr=RHO))}


def mpc_batches(N):
    """k_mpc solves one environment on G lanes, G the power of two >= N, 64 / G environments per block: one environment, and
    the smallest batch with a full block and a partial one"""
    G = 1
    while G < N:
        G *= 2
    return 1, 64 // G + 1


@pytest.mark.parametrize("kind", sorted(MPC_CASES))
def test_mpc_writes_only_its_rows(kind):
    cls, task = MPC_CASES[kind]
    assert mpc_batches(N_MPC) == (1, 17)
    for E_ in mpc_batches(N_MPC):
        reg, ea, eb = pair(lambda: easy(E_, **task))
        with reg.guarding():
            ga = cls(ea.simulator, ea.action_space, ea.gamma, safety_margin=0.92, planning_steps=N_MPC)
        gb = cls(eb.simulator, eb.action_space, eb.gamma, safety_margin=0.92, planning_steps=N_MPC)
        for g, env in ((ga, ea), (gb, eb)):
            g.warn_unconverged = False
            g.solver.keep_solution = g.solver.keep_trace = True
            assert g._fused(env)
        where = "MPC %s, E = %d" % (kind, E_)
        both_reset(reg, ea, eb, where + ": reset", sampler="device")
        for t in range(3):
            with reg.guarding():                          # (the solver's buffers are allocated by its first call)
                ua = ga.act(ea)
                ga.solver.solve(*ga.forecast(ea), ea.simulator.soc)   # the unfused entry point: it also writes `solution`
            ub = gb.act(eb)
            gb.solver.solve(*gb.forecast(eb), eb.simulator.soc)
            sa, sb = ga.solver, gb.solver
            assert_guarded(reg, sa.u0, sa.objective, sa.iters, sa.info, sa.solution, sa.trace, sa._action)
            assert sa.solution.shape[:2] == (E_, N_MPC) and sa.trace.shape[0] == E_ and not bool(torch.isnan(sa.trace[:, 0]).all())
            for k in ("u0", "objective", "iters", "info", "solution", "trace", "_action"):
                assert torch.equal(bits(getattr(sa, k)), bits(getattr(sb, k))), "%s step %d: %s" % (where, t, k)
            assert torch.equal(bits(ua), bits(ub)), where
            reg.assert_intact("%s: act %d" % (where, t))
            both_step(reg, ea, eb, ua, "%s: step %d" % (where, t))
