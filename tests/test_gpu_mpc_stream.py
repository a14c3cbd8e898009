"""GPU tier: ``MPCAgentPerfectStream`` -- the perfect-forecast MPC agent of the tasks whose loads and generator potentials
are drawn inside the step kernels (``exogenous="uniform"`` / ``"series_noise"``).  Its forecast is the tasks' own Philox
stream evaluated ahead by the lanes of the solve (``anm_mpc_act_stream_f64``, csrc/anm_mpc.hpp: Act mode 3; specification:
gym_anm_amd/rng.py, exo_forecast).
  1. the one-launch act() equals forecast() -> solve -> scaling / clipping in torch, bit for bit, in closed loop;
  2. the forecast is the future: what the environment then draws; 3. the same across in-kernel resets;
  4. sharding, float32 environments, HIP graph; 5. what is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, errors, networks
from gym_anm_amd.agents import MPCAgentPerfectStream
from gym_anm_amd.envs.anm6 import ANM6EasyVec
from gym_anm_amd.envs.anm_env import BatchedANMEnv

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ODD = 67          # one wavefront of environments and a partial one at N = 1; 3 x 16 + 3 groups of four lanes at N = 3, 4
NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0),
        "mesh14": lambda: networks.synthetic_meshed_network(14, 0, 3)}


def make_env(mode, E_, seed, net="anm6", **kw):
    """ANM6 in uniform mode / in series-noise mode (ANM6Easy's tables, amplitude 2 MW), default ends; other networks: uniform"""
    if mode == "noise":
        assert net == "anm6"
        env = ANM6EasyVec(num_envs=E_, device=DEV, seed=seed, tol=1e-6, exogenous="series_noise", exo_noise=2.0, **kw)
    else:
        env = BatchedANMEnv(NETS[net](), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, 1000),)), costs_clipping=(1, 100),
                            seed=seed, num_envs=E_, device=DEV, tol=1e-6, exogenous="uniform", **kw)
    env.check_actions = False
    return env


class Unfused(MPCAgentPerfectStream):
    def _fused(self, env):
        return False


def agents(env, N, **kw):
    fused = MPCAgentPerfectStream(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N, **kw)
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
    """the scheme of tests/test_mpc.py (check_fused_act): identical bits, step after step in closed loop"""
    for N in horizons:
        fused, plain = agents(env, N, **kw)
        for t in range(steps):
            a = assert_same_act(fused, plain, env, (N, t))
            env.step(a.clone())
    return fused


# ---- 1. fused = unfused ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_fused_act_equals_the_unfused_path_on_anm6(mode):
    env = make_env(mode, E_ODD, 5, autoreset=True)
    env.reset()
    fused = check_fused_act(env)
    assert bool(fused.last_converged.all())


def test_fused_act_equals_the_unfused_path_on_the_30_bus_feeder():
    env = make_env("uniform", 9, 6, net="case30", autoreset=True)
    env.reset()
    check_fused_act(env, horizons=(3,))


def test_fused_act_equals_the_unfused_path_through_a_size_class(monkeypatch):
    """a meshed 14-bus network nobody compiled anything for: it steps in generic mode and its MPC kernel is the size class
    s1 it is padded into (8 loads, 2 generators) -- the generators' units follow the network's own loads -- with hipcc hidden"""
    monkeypatch.setattr(codegen, "hipcc_path", lambda: None)
    env = make_env("uniform", 5, 7, net="mesh14", autoreset=True)
    assert env.simulator.backend.generic
    env.reset()
    fused = check_fused_act(env)
    assert fused.solver.backend.size_class == "s1"


@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_fused_act_equals_the_unfused_path_for_one_environment(mode):
    env = make_env(mode, 1, 8, autoreset=True)
    env.reset()
    check_fused_act(env)


# ---- 2. the forecast is the future -----------------------------------------------------------------------------------------
def drawn_state_columns(model):
    D, nd = model.N_device, model.N_des
    return list(model.load_idx), [2 * D + nd + g for g in range(model.N_non_slack_gen)]


@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_the_forecast_is_what_the_environment_then_draws(mode):
    N = 4
    env = make_env(mode, E_ODD, 12, autoreset=False)
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
    assert np.abs(want_l).max() > 1.0 and np.ptp(want_g, axis=2).max() > 1.0      # ... and not of constants


# ---- 3. across resets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_across_in_kernel_resets(mode):
    """episode limit 3, autoreset: every environment is re-initialised inside the step kernel every fourth step; the forecast
    follows the new epoch and step index, so it is again what the environment draws, for the stages inside the episode"""
    N, LIMIT = 2, 3
    env = make_env(mode, E_ODD, 13, autoreset=True, max_episode_steps=LIMIT)
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


# ---- 4. sharding, float32 environments, HIP graph ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_two_shards_act_like_the_whole_batch(mode):
    H0 = 34
    whole = make_env(mode, E_ODD, 14, autoreset=True)
    shards = [make_env(mode, H0, 14, autoreset=True, env_offset=0), make_env(mode, E_ODD - H0, 14, autoreset=True, env_offset=H0)]
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


@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_a_float32_environment_gets_the_actions_of_its_float64_twin(mode):
    e64, e32 = make_env(mode, E_ODD, 15, autoreset=True), make_env(mode, E_ODD, 15, autoreset=True, io_dtype=torch.float32)
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


@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_a_captured_act_replays_what_eager_calls_compute(mode):
    eager_env, graph_env = make_env(mode, E_ODD, 16, autoreset=True), make_env(mode, E_ODD, 16, autoreset=True)
    eager_env.reset()
    graph_env.reset()
    eager, graphed = agents(eager_env, 3)[0], agents(graph_env, 3)[0]
    for ag in (eager, graphed):
        ag.reuse_action_buffer = True
    first = graphed.act(graph_env).clone()               # (buffers and the device copies of the ends exist before the capture)
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


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def call_stream(agent, env, **changes):
    """anm_mpc_act_stream_f64 as BatchedDCOPF makes the call, with fields of the anm_mpc_stream replaced"""
    sv = agent.solver
    agent.act(env)                                        # (buffers, device copies)
    lo, hi, amp = sv._exo_dev
    f = dict(exo_mode=_lib.EXO_SERIES_NOISE if env._noisy else _lib.EXO_UNIFORM, rng_seed=int(env.rng_seed), env_offset=0,
             timestep=env.timestep.data_ptr(), reset_count=env._reset_count.data_ptr(), exo_low=lo.data_ptr(), exo_high=hi.data_ptr(),
             exo_noise=None if amp is None else amp.data_ptr())
    f.update(changes)
    st = _lib.MpcStream(**f)
    ser = getattr(sv, "_series_dev", None) if env._noisy else None
    rc = sv.backend.lib.anm_mpc_act_stream_f64(
        sv._handle, env.num_envs, env._state_buf.data_ptr(), None, None, int(env._state_buf.shape[1]), None,
        None if ser is None else ser.data_ptr(), 0 if ser is None else int(ser.shape[1]), env.simulator.soc.data_ptr(),
        agent._lo.data_ptr(), agent._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(), sv.objective.data_ptr(),
        sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), C.byref(st), None)
    return rc, sv.backend.lib.anm_last_error()


def test_what_is_refused():
    uni, noi = make_env("uniform", 4, 17), make_env("noise", 4, 17)
    uni.reset()
    noi.reset()
    ag_u, ag_n = agents(uni, 2)[0], agents(noi, 2)[0]
    assert call_stream(ag_u, uni)[0] == 0 and call_stream(ag_n, noi)[0] == 0
    # anm_mpc_act_f64 keeps refusing forecast 3
    sv = ag_u.solver
    rc = sv.backend.lib.anm_mpc_act_f64(
        sv._handle, 4, _lib.MPC_FORECAST_STREAM, uni._state_buf.data_ptr(), None, None, int(uni._state_buf.shape[1]), None, None, 0,
        uni.simulator.soc.data_ptr(), ag_u._lo.data_ptr(), ag_u._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(),
        sv.objective.data_ptr(), sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), None)
    assert rc != 0 and b"unknown forecast" in sv.backend.lib.anm_last_error()
    for env, ag, changes, msg in ((uni, ag_u, dict(timestep=None), b"timestep"), (uni, ag_u, dict(reset_count=None), b"reset_count"),
                                  (uni, ag_u, dict(exo_low=None), b"exo_low"), (uni, ag_u, dict(exo_high=None), b"exo_high"),
                                  (uni, ag_u, dict(exo_mode=_lib.EXO_HOST), b"exo_mode"), (uni, ag_u, dict(exo_mode=3), b"exo_mode"),
                                  (noi, ag_n, dict(exo_noise=None), b"exo_noise"),
                                  (uni, ag_u, dict(exo_mode=_lib.EXO_SERIES_NOISE), b"series")):
        rc, err = call_stream(ag, env, **changes)
        assert rc != 0 and msg in err, (changes, err)
    # the agent on a task that is not drawn inside the kernels (ANM6Easy: the host hook / series mode)
    host = ANM6EasyVec(num_envs=4, device=DEV, seed=1)
    host.reset(seed=1)
    with pytest.raises(errors.ArgsError, match="drawn inside the step kernels"):
        MPCAgentPerfectStream(host.simulator, host.action_space, host.gamma, planning_steps=2)
    for call in (ag_u.act, ag_u.forecast, lambda e: ag_u.solver.act(3, e, ag_u._lo, ag_u._hi)):
        with pytest.raises(errors.ArgsError, match="exogenous"):
            call(host)
    # ... and the perfect agent of the series-mode tasks on a task without tables
    from gym_anm_amd.agents import MPCAgentPerfect

    with pytest.raises(errors.ArgsError, match="MPCAgentPerfectStream"):
        MPCAgentPerfect(uni.simulator, uni.action_space, uni.gamma, planning_steps=2).act(uni)
