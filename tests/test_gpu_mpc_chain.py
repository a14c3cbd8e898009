"""GPU tier: ``MPCAgentPerfectChain`` -- the perfect-forecast MPC agent of the series-noise task with correlated noise
(``exogenous="series_noise", exo_corr=rho``).  Its forecast is the step kernels' AR(1) recurrence rolled forward from the
environment's noise states ``exo_z`` by a sweep over the lanes of the solve (``anm_mpc_act_chain_f64``, csrc/anm_mpc.hpp:
Act mode 4; specification: gym_anm_amd/rng.py, exo_forecast_corr).
  1. the one-launch act() equals forecast() -> solve -> scaling / clipping in torch, bit for bit, in closed loop, for every
     shape of a group; 2. without correlation it is the stream agent; 3. the forecast is what the environment then draws;
  4. the same across in-kernel resets; 5. sharding, float32 environments, HIP graph, exo_z untouched; 6. what is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, errors, networks
from gym_anm_amd.agents import MPCAgentPerfectChain, MPCAgentPerfectStream
from gym_anm_amd.envs.anm6 import ANM6EasyVec
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ODD = 67          # one wavefront of environments and a partial one at N = 1; 3 x 16 + 3 groups of four lanes at N = 3, 4
RHO = (0.9, 0.5, 0.0, 0.0, 0.99)


def make_env(E_, seed, corr=RHO, **kw):
    """ANM6Easy in series-noise mode (amplitude 2 MW) with correlated noise"""
    env = ANM6EasyVec(num_envs=E_, device=DEV, seed=seed, tol=1e-6, exogenous="series_noise", exo_noise=2.0, exo_corr=corr, **kw)
    env.check_actions = False
    return env


def sine_task(net, period=96):
    """daily sine profiles for every load and generator of a network (as bench.py builds them for the 30-bus feeder), MW"""
    m = NetworkModel(net, 0.25, 100)
    r, t = np.random.default_rng(3), np.arange(period) / period
    rows = [m.dev_p_min[k] * m.baseMVA * (0.25 + 0.3 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.load_idx]
    rows += [m.dev_p_max[k] * m.baseMVA * (0.1 + 0.45 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.gen_idx]
    return np.array(rows)


def make_net_env(net, E_, seed, **kw):
    ser = sine_task(net)
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, ser.shape[1] - 1),)), costs_clipping=(1, 100),
                        seed=seed, num_envs=E_, device=DEV, tol=1e-6, series=ser, exogenous="series_noise",
                        exo_noise=0.1 * np.abs(ser).max(axis=1), exo_corr=0.8, **kw)
    env.check_actions = False
    return env


class Unfused(MPCAgentPerfectChain):
    def _fused(self, env):
        return False


def agents(env, N, **kw):
    fused = MPCAgentPerfectChain(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N, **kw)
    plain = Unfused(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N, **kw)
    assert fused._fused(env) and not plain._fused(env)
    fused.warn_unconverged = plain.warn_unconverged = False
    return fused, plain


def assert_same_act(fused, plain, env, what):
    a, b = fused.act(env), plain.act(env)
    assert a.shape == b.shape == (env.num_envs, env.action_space.shape[0])
    assert torch.equal(a, b), (what, float((a - b).abs().max()))
    for name in ("u0", "objective", "iters", "info"):
        assert torch.equal(getattr(fused.solver, name), getattr(plain.solver, name)), (what, name)
    return a


def check_fused_act(env, steps=6, horizons=(1, 3), **kw):
    """identical bits, step after step in closed loop (both paths perform the same operations)"""
    for N in horizons:
        fused, plain = agents(env, N, **kw)
        for t in range(steps):
            a = assert_same_act(fused, plain, env, (N, t))
            env.step(a.clone())
    return fused


# ---- 1. fused = unfused ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [True, False])
def test_fused_act_equals_the_unfused_path_on_anm6(autoreset):
    """N = 1: one thread per environment, a partial wavefront; N = 3: groups of four lanes, the fourth idle"""
    env = make_env(E_ODD, 5, autoreset=autoreset)
    env.reset()
    fused = check_fused_act(env)
    assert bool(fused.last_converged.all()) or not autoreset
    assert float(env.exo_z.abs().max()) > 0.5


@pytest.mark.parametrize("N", [4, 16, 17, 33])
def test_fused_act_equals_the_unfused_path_for_every_shape_of_a_group(N):
    """4: full groups side by side inside a DPP row; 16: a whole row; 17: a group that crosses a row; 33: three rows"""
    env = make_env(5, 6, autoreset=True)
    env.reset()
    check_fused_act(env, steps=3, horizons=(N,))


def test_fused_act_equals_the_unfused_path_for_one_environment():
    env = make_env(1, 8, autoreset=True)
    env.reset()
    check_fused_act(env)


def test_fused_act_equals_the_unfused_path_on_the_30_bus_feeder():
    env = make_net_env(networks.synthetic_radial_network(30, 0), 9, 6, autoreset=True)
    env.reset()
    check_fused_act(env, horizons=(3,))


def test_fused_act_equals_the_unfused_path_through_a_size_class(monkeypatch):
    """a meshed 14-bus network nobody compiled anything for: it steps in generic mode and its MPC kernel is the size class
    s1 it is padded into (8 loads, 2 generators) -- the generators' units and the rows of exo_z follow the network's own
    counts -- with hipcc hidden"""
    monkeypatch.setattr(codegen, "hipcc_path", lambda: None)
    env = make_net_env(networks.synthetic_meshed_network(14, 0, 3), 5, 7, autoreset=True)
    assert env.simulator.backend.generic
    env.reset()
    fused = check_fused_act(env)
    assert fused.solver.backend.size_class == "s1"


# ---- 2. the anchor -----------------------------------------------------------------------------------------------------------
def test_without_correlation_the_chain_agent_is_the_stream_agent():
    """exo_corr=0.0 runs the chain (z' = fma(0, z, w) = w); exo_corr=None is the uncorrelated task: same seed, same bits"""
    chain_env, plain_env = make_env(E_ODD, 9, corr=0.0, autoreset=True), make_env(E_ODD, 9, corr=None, autoreset=True)
    chain_env.reset()
    plain_env.reset()
    chain = agents(chain_env, 3)[0]
    stream = MPCAgentPerfectStream(plain_env.simulator, plain_env.action_space, plain_env.gamma, safety_margin=0.92, planning_steps=3)
    stream.warn_unconverged = False
    assert chain_env.exo_z is not None and plain_env.exo_z is None
    for t in range(6):
        a, b = chain.act(chain_env), stream.act(plain_env)
        assert torch.equal(a, b), t
        chain_env.step(a.clone())
        plain_env.step(b.clone())
        assert torch.equal(chain_env.state, plain_env.state), t


# ---- 3. the forecast is the future -----------------------------------------------------------------------------------------
def drawn_state_columns(model):
    D, nd = model.N_device, model.N_des
    return list(model.load_idx), [2 * D + nd + g for g in range(model.N_non_slack_gen)]


def test_the_forecast_is_what_the_environment_then_draws():
    N = 4
    env = make_env(E_ODD, 12, autoreset=False)
    env.reset()
    model = env.simulator.model
    fused, plain = agents(env, N)
    pl, pg = plain.forecast(env)                                       # [E, n, N] p.u.
    assert pl.shape == (E_ODD, model.N_load, N) and pg.shape == (E_ODD, model.N_non_slack_gen, N)
    want_l, want_g = (pl * model.baseMVA).cpu().numpy(), (pg * model.baseMVA).cpu().numpy()
    lcols, gcols = drawn_state_columns(model)
    gen = torch.Generator(device=DEV).manual_seed(2)
    for j in range(N):
        env.step(uniform_actions(env, gen))
        alive = ~env.terminated.cpu().numpy()
        s = env.state.cpu().numpy()
        np.testing.assert_allclose(s[alive][:, lcols], want_l[alive, :, j], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(s[alive][:, gcols], want_g[alive, :, j], rtol=1e-12, atol=1e-12)
    assert int(alive.sum()) >= 60, int(alive.sum())                   # (the comparison is not empty)
    assert np.ptp(want_l) > 1.0 and np.ptp(want_g) > 1.0              # ... and not of constants: the forecast spans more than 1 MW


# ---- 4. across resets ------------------------------------------------------------------------------------------------------
def test_across_in_kernel_resets():
    """episode limit 3, autoreset: every environment is re-initialised inside the step kernel every fourth step and its chain
    starts again from z = w(step 0) of the new epoch; the forecast follows, so it is again what the environment draws, for the
    stages inside the episode"""
    N, LIMIT = 2, 3
    env = make_env(E_ODD, 13, autoreset=True, max_episode_steps=LIMIT)
    env.reset()
    model = env.simulator.model
    lcols, gcols = drawn_state_columns(model)
    fused, plain = agents(env, N)
    rc0 = env._reset_count.clone()
    pending, checked_after_reset = [], 0       # (forecast MW [E, n, N], timestep, reset count) of earlier steps
    for t in range(8):
        a = assert_same_act(fused, plain, env, t)
        pl, pg = plain.forecast(env)
        pending.append((torch.cat((pl, pg), 1) * model.baseMVA, env.timestep.clone(), env._reset_count.clone()))
        env.step(a.clone())
        state = env.state
        now = torch.cat((state[:, lcols], state[:, gcols]), 1)
        for f, t_k, rc_k in pending:
            for j in range(N):
                hit = (env._reset_count == rc_k) & (env.timestep == t_k + 1 + j) & ~env.terminated
                if bool(hit.any()):
                    torch.testing.assert_close(now[hit], f[hit][:, :, j], rtol=1e-12, atol=1e-12)
                    checked_after_reset += int((hit & (rc_k > rc0)).sum())
        pending = pending[-N:]
    assert int((env._reset_count - rc0).min()) >= 2 and checked_after_reset >= 2 * 60


# ---- 5. sharding, float32 environments, HIP graph, exo_z ---------------------------------------------------------------------
def test_two_shards_act_like_the_whole_batch():
    H0 = 34
    whole = make_env(E_ODD, 14, autoreset=True)
    shards = [make_env(H0, 14, autoreset=True, env_offset=0), make_env(E_ODD - H0, 14, autoreset=True, env_offset=H0)]
    for env in [whole] + shards:
        env.reset()
    ag_w = agents(whole, 3)[0]
    ag_s = [agents(env, 3)[0] for env in shards]
    for t in range(3):
        a = ag_w.act(whole)
        parts = [ag.act(env) for ag, env in zip(ag_s, shards)]
        assert torch.equal(a, torch.cat(parts)), t
        whole.step(a.clone())
        for env, p in zip(shards, parts):
            env.step(p.clone())
        assert torch.equal(whole.state, torch.cat([env.state for env in shards]))


def test_a_float32_environment_gets_the_actions_of_its_float64_twin():
    e64, e32 = make_env(E_ODD, 15, autoreset=True), make_env(E_ODD, 15, autoreset=True, io_dtype=torch.float32)
    e64.reset()
    e32.reset()
    a64, a32 = agents(e64, 3)[0], agents(e32, 3)[0]
    for t in range(3):
        x, y = a64.act(e64), a32.act(e32)
        assert x.dtype == y.dtype == torch.float64 and torch.equal(x, y), t
        act = x.float()                                   # one float32 action for both: the states stay twins
        e64.step(act.double())
        e32.step(act)
        assert torch.equal(e64.state, e32.state)


def test_a_captured_act_replays_what_eager_calls_compute():
    eager_env, graph_env = make_env(E_ODD, 16, autoreset=True), make_env(E_ODD, 16, autoreset=True)
    eager_env.reset()
    graph_env.reset()
    eager, graphed = agents(eager_env, 3)[0], agents(graph_env, 3)[0]
    for ag in (eager, graphed):
        ag.reuse_action_buffer = True
    first = graphed.act(graph_env).clone()               # (buffers and the device copies of the tables exist before the capture)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            out = graphed.act(graph_env)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    for t in range(5):
        g.replay()
        a = eager.act(eager_env)
        torch.cuda.synchronize()
        assert torch.equal(a, out), t
        if t == 0:
            assert torch.equal(a, first)
        for name in ("u0", "objective", "iters", "info"):
            assert torch.equal(getattr(eager.solver, name), getattr(graphed.solver, name)), (t, name)
        eager_env.step(a.clone())
        graph_env.step(out.clone())
    assert int(eager_env.timestep.max()) > 0 and not torch.equal(out, first)


def test_act_only_reads_the_noise_states():
    env = make_env(E_ODD, 17, autoreset=True)
    env.reset()
    env.step(uniform_actions(env, torch.Generator(device=DEV).manual_seed(3)))
    fused, plain = agents(env, 3)
    before = env.exo_z.clone()
    assert float(before.abs().max()) > 0.5
    fused.act(env)
    plain.act(env)
    torch.cuda.synchronize()
    assert torch.equal(env.exo_z, before)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def call_chain(agent, env, null_struct=False, **changes):
    """anm_mpc_act_chain_f64 as BatchedDCOPF makes the call, with fields of the anm_mpc_chain replaced"""
    sv = agent.solver
    agent.act(env)                                        # (buffers, device copies)
    lo, hi, amp, rho, innov = sv._chain_dev
    f = dict(exo_mode=_lib.EXO_SERIES_NOISE, rng_seed=int(env.rng_seed), env_offset=0, timestep=env.timestep.data_ptr(),
             reset_count=env._reset_count.data_ptr(), exo_low=lo.data_ptr(), exo_high=hi.data_ptr(), exo_noise=amp.data_ptr(),
             exo_rho=rho.data_ptr(), exo_innov=innov.data_ptr(), exo_z=env.exo_z.data_ptr())
    series, period = changes.pop("series", sv._series_dev.data_ptr()), changes.pop("period", int(sv._series_dev.shape[1]))
    num_envs = changes.pop("num_envs", env.num_envs)
    f.update(changes)
    st = _lib.MpcChain(**f)
    rc = sv.backend.lib.anm_mpc_act_chain_f64(
        sv._handle, num_envs, env._state_buf.data_ptr(), None, None, int(env._state_buf.shape[1]), None, series, period,
        env.simulator.soc.data_ptr(), agent._lo.data_ptr(), agent._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(),
        sv.objective.data_ptr(), sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), None if null_struct else C.byref(st), None)
    return rc, sv.backend.lib.anm_last_error()


def test_what_is_refused():
    env = make_env(4, 18)
    env.reset()
    ag = agents(env, 2)[0]
    assert call_chain(ag, env)[0] == 0 and call_chain(ag, env, num_envs=0)[0] == 0
    rc, err = call_chain(ag, env, null_struct=True)
    assert rc != 0 and b"anm_mpc_chain" in err
    for changes, msg in ((dict(exo_mode=_lib.EXO_UNIFORM), b"exo_mode"), (dict(exo_mode=_lib.EXO_HOST), b"exo_mode"), (dict(exo_mode=3), b"exo_mode"),
                         (dict(exo_rho=None), b"exo_rho"), (dict(exo_innov=None), b"exo_innov"), (dict(exo_z=None), b"exo_z"),
                         (dict(timestep=None), b"timestep"), (dict(reset_count=None), b"reset_count"), (dict(exo_low=None), b"exo_low"),
                         (dict(exo_high=None), b"exo_high"), (dict(exo_noise=None), b"exo_noise"), (dict(series=None), b"series"),
                         (dict(period=0), b"period")):
        rc, err = call_chain(ag, env, **changes)
        assert rc != 0 and msg in err and b"anm_mpc_act_chain_f64" in err, (changes, err)
    # anm_mpc_act_f64 keeps refusing forecast 4 (and 3)
    sv = ag.solver
    for forecast in (_lib.MPC_FORECAST_CHAIN, _lib.MPC_FORECAST_STREAM):
        rc = sv.backend.lib.anm_mpc_act_f64(
            sv._handle, 4, forecast, env._state_buf.data_ptr(), None, None, int(env._state_buf.shape[1]), None, None, 0,
            env.simulator.soc.data_ptr(), ag._lo.data_ptr(), ag._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(),
            sv.objective.data_ptr(), sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), None)
        assert rc != 0 and b"unknown forecast" in sv.backend.lib.anm_last_error()
    # the agent on an uncorrelated, a uniform and a host-hook task
    plain = make_env(4, 18, corr=None)
    uniform = BatchedANMEnv(networks.anm6_network(), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, 1000),)), costs_clipping=(1, 100),
                            seed=18, num_envs=4, device=DEV, tol=1e-6, exogenous="uniform")
    host = ANM6EasyVec(num_envs=4, device=DEV, seed=1)
    for other, match in ((plain, "MPCAgentPerfectStream"), (uniform, "series_noise"), (host, "series_noise")):
        other.reset()
        with pytest.raises(errors.ArgsError, match=match):
            MPCAgentPerfectChain(other.simulator, other.action_space, other.gamma, planning_steps=2)
        for call in (ag.act, ag.forecast, lambda e: ag.solver.act(4, e, ag._lo, ag._hi)):
            with pytest.raises(errors.ArgsError, match="series_noise"):
                call(other)
    # ... and the stream agent keeps refusing the correlated task, now naming this one
    with pytest.raises(errors.ArgsError, match="MPCAgentPerfectChain"):
        MPCAgentPerfectStream(env.simulator, env.action_space, env.gamma, planning_steps=2)
