"""GPU tier: ``MPCAgentExpected`` -- the conditional-mean forecast MPC agent of the tasks drawn inside the step kernels
(``exogenous="uniform"``, ``"series_noise"`` with and without ``exo_corr=``).  Its forecast is the step kernels' AR(1)
recurrence with the innovation at its mean, rolled forward from the environment's noise states ``exo_z`` by a sweep over the
lanes of the solve, without any draw (``anm_mpc_act_expect_f64``, csrc/anm_mpc.hpp: Act mode 5; specification:
gym_anm_amd/rng.py, exo_forecast_expected).
  1. the one-launch act() equals forecast() -> solve -> scaling / clipping in torch, bit for bit, in closed loop, for every
     shape of a group and every kind of task; 2. the anchors: exo_corr=0.0 is exo_corr=None, and without noise states the
     agent is the profile agent; 3. exo_z untouched, float32 environments, HIP graph; 4. what is refused; 5. the perfect
     agents are what they were."""
import ctypes as C

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, errors, networks
from gym_anm_amd.agents import MPCAgentExpected, MPCAgentPerfect, MPCAgentPerfectChain, MPCAgentPerfectStream
from gym_anm_amd.envs.anm6 import ANM6EasyVec
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

from parity_common import uniform_actions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ODD = 67          # one wavefront of environments and a partial one at N = 1; 3 x 16 + 3 groups of four lanes at N = 3, 4
RHO = (0.9, 0.5, 0.0, 0.8, 0.99)
WIDE_HIGH = [0, 0, 0, 40, 50]    # ends no entry of ANM6Easy's tables lies outside of (its solar table reaches 36.75 MW)


def make_env(E_, seed, corr=RHO, **kw):
    """ANM6Easy in series-noise mode (amplitude 2 MW), with correlated noise unless corr is None"""
    env = ANM6EasyVec(num_envs=E_, device=DEV, seed=seed, tol=1e-6, exogenous="series_noise", exo_noise=2.0, exo_corr=corr, **kw)
    env.check_actions = False
    return env


def make_uniform_env(E_, seed, **kw):
    env = BatchedANMEnv(networks.anm6_network(), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, 1000),)), costs_clipping=(1, 100),
                        seed=seed, num_envs=E_, device=DEV, tol=1e-6, exogenous="uniform", **kw)
    env.check_actions = False
    return env


def sine_task(net, period=96):
    """daily sine profiles for every load and generator of a network, MW"""
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


class Unfused(MPCAgentExpected):
    def _fused(self, env):
        return False


def agents(env, N, **kw):
    fused = MPCAgentExpected(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N, **kw)
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
    """N = 1: one thread per environment, a partial wavefront; N = 3: groups of four lanes, the fourth idle; 12 steps"""
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


@pytest.mark.parametrize("kind", ["correlated", "uncorrelated", "uniform"])
def test_fused_act_equals_the_unfused_path_on_each_kind_of_task(kind):
    env = {"correlated": lambda: make_env(E_ODD, 9, autoreset=True), "uncorrelated": lambda: make_env(E_ODD, 9, corr=None, autoreset=True),
           "uniform": lambda: make_uniform_env(E_ODD, 9, autoreset=True)}[kind]()
    env.reset()
    assert (env.exo_z is not None) == (kind == "correlated")
    check_fused_act(env, steps=4, horizons=(3,))


def test_the_single_environment_wrapper():
    """a NumPy-facing single-environment class holds its batch of one as ``vec``: act() goes through it, as in the chain agent"""
    env = make_env(1, 8, autoreset=True)
    env.reset()
    fused = agents(env, 3)[0]
    want = fused.act(env)[0].cpu().numpy()
    wrapper = type("Wrapper", (), {"vec": env})()
    got = fused.act(wrapper)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and (got == want).all()


# ---- 2. the anchors --------------------------------------------------------------------------------------------------------
def test_zero_correlation_is_no_correlation():
    """exo_corr=0.0 runs the sweep (fma(0, z, +0.0) = +0.0 whatever z holds); exo_corr=None skips it: same seed, same bits"""
    zero_env, none_env = make_env(E_ODD, 9, corr=0.0, autoreset=True), make_env(E_ODD, 9, corr=None, autoreset=True)
    zero_env.reset()
    none_env.reset()
    zero, none = agents(zero_env, 3)[0], agents(none_env, 3)[0]
    assert zero_env.exo_z is not None and none_env.exo_z is None
    for t in range(6):
        a, b = zero.act(zero_env), none.act(none_env)
        assert torch.equal(a, b), t
        for name in ("u0", "objective", "iters", "info"):
            assert torch.equal(getattr(zero.solver, name), getattr(none.solver, name)), (t, name)
        zero_env.step(a.clone())
        none_env.step(b.clone())
        assert torch.equal(zero_env.state, none_env.state), t
    assert bool((zero_env.exo_z < 0).any()) and float(zero_env.exo_z.abs().max()) > 0.5


def test_without_noise_states_the_agent_is_the_profile_agent():
    """exo_corr=None: every stage maps a noise of +0.0, fma(amp, +0.0, table) = table, and with ends no table entry lies
    outside of the clip passes it on: MPCAgentPerfect's forecast on the same environment, bit for bit"""
    env = make_env(E_ODD, 10, corr=None, autoreset=True, exo_high=WIDE_HIGH)
    env.reset()
    ser = env._series
    assert (ser <= env.exo_high[:, None]).all() and (ser >= env.exo_low[:, None]).all() and float(ser[3].max()) > 30.0
    expected = agents(env, 3)[0]
    profile = MPCAgentPerfect(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=3)
    profile.warn_unconverged = False
    assert profile._fused(env)
    for t in range(6):
        a, b = expected.act(env), profile.act(env)
        assert torch.equal(a, b), t
        for name in ("u0", "objective", "iters", "info"):
            assert torch.equal(getattr(expected.solver, name), getattr(profile.solver, name)), (t, name)
        env.step(a.clone())


# ---- 3. exo_z, float32 environments, HIP graph -------------------------------------------------------------------------------
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


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def call_expect(agent, env, null_struct=False, **changes):
    """anm_mpc_act_expect_f64 as BatchedDCOPF makes the call, with fields of the anm_mpc_expect replaced"""
    sv = agent.solver
    agent.act(env)                                        # (buffers, device copies)
    lo, hi, amp, rho = sv._expect_dev
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    f = dict(exo_mode=_lib.EXO_SERIES_NOISE if env._noisy else _lib.EXO_UNIFORM, exo_low=lo.data_ptr(), exo_high=hi.data_ptr(),
             exo_noise=ptr(amp), exo_rho=ptr(rho), exo_z=ptr(env.exo_z))
    has_series = getattr(sv, "_series_dev", None) is not None and env._noisy
    series = changes.pop("series", sv._series_dev.data_ptr() if has_series else None)
    period = changes.pop("period", int(sv._series_dev.shape[1]) if has_series else 0)
    num_envs = changes.pop("num_envs", env.num_envs)
    f.update(changes)
    st = _lib.MpcExpect(**f)
    rc = sv.backend.lib.anm_mpc_act_expect_f64(
        sv._handle, num_envs, env._state_buf.data_ptr(), None, None, int(env._state_buf.shape[1]), None, series, period,
        env.simulator.soc.data_ptr(), agent._lo.data_ptr(), agent._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(),
        sv.objective.data_ptr(), sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), None if null_struct else C.byref(st), None)
    return rc, sv.backend.lib.anm_last_error()


def test_what_is_refused():
    env = make_env(4, 18)
    env.reset()
    ag = agents(env, 2)[0]
    assert call_expect(ag, env)[0] == 0 and call_expect(ag, env, num_envs=0)[0] == 0 and call_expect(ag, env, num_envs=-3)[0] == 0
    assert call_expect(ag, env, exo_rho=None, exo_z=None)[0] == 0          # (no noise states: a valid call)
    rc, err = call_expect(ag, env, null_struct=True)
    assert rc != 0 and b"anm_mpc_expect" in err
    for changes, msg in ((dict(exo_mode=_lib.EXO_HOST), b"exo_mode"), (dict(exo_mode=3), b"exo_mode"), (dict(exo_mode=-1), b"exo_mode"),
                         (dict(exo_low=None), b"exo_low"), (dict(exo_high=None), b"exo_high"), (dict(exo_noise=None), b"exo_noise"),
                         (dict(series=None), b"series"), (dict(period=0), b"period"), (dict(exo_rho=None), b"exo_rho and exo_z"),
                         (dict(exo_z=None), b"exo_rho and exo_z"), (dict(exo_mode=_lib.EXO_UNIFORM), b"uniform mode"),
                         (dict(exo_mode=_lib.EXO_UNIFORM, series=None, period=0, exo_noise=None), b"uniform mode")):
        rc, err = call_expect(ag, env, **changes)
        assert rc != 0 and msg in err and b"anm_mpc_act_expect_f64" in err, (changes, err)
    uniform = make_uniform_env(4, 18)
    uniform.reset()
    ag_u = agents(uniform, 2)[0]
    assert call_expect(ag_u, uniform)[0] == 0
    for changes in (dict(exo_rho=ag.solver._expect_dev[3].data_ptr()), dict(exo_z=env.exo_z.data_ptr()),
                    dict(exo_rho=ag.solver._expect_dev[3].data_ptr(), exo_z=env.exo_z.data_ptr())):
        rc, err = call_expect(ag_u, uniform, **changes)
        assert rc != 0 and (b"uniform mode" in err or b"exo_rho and exo_z" in err) and b"anm_mpc_act_expect_f64" in err, (changes, err)
    # anm_mpc_act_f64 refuses forecast 5, like 3 and 4
    sv = ag.solver
    for forecast in (_lib.MPC_FORECAST_EXPECT, _lib.MPC_FORECAST_CHAIN, _lib.MPC_FORECAST_STREAM):
        rc = sv.backend.lib.anm_mpc_act_f64(
            sv._handle, 4, forecast, env._state_buf.data_ptr(), None, None, int(env._state_buf.shape[1]), None, None, 0,
            env.simulator.soc.data_ptr(), ag._lo.data_ptr(), ag._hi.data_ptr(), sv._action.data_ptr(), sv.u0.data_ptr(),
            sv.objective.data_ptr(), sv.iters.data_ptr(), sv.info.data_ptr(), C.byref(sv.opts), None)
        assert rc != 0 and b"unknown forecast" in sv.backend.lib.anm_last_error()
    # the agent on a series-mode (host-hook) task
    host = ANM6EasyVec(num_envs=4, device=DEV, seed=1)
    host.reset()
    with pytest.raises(errors.ArgsError, match="MPCAgentPerfect.*MPCAgentConstant"):
        MPCAgentExpected(host.simulator, host.action_space, host.gamma, planning_steps=2)
    for call in (ag.act, ag.forecast):
        with pytest.raises(errors.ArgsError, match="MPCAgentPerfect.*MPCAgentConstant"):
            call(host)
    with pytest.raises(errors.ArgsError, match="uniform"):
        ag.solver.act(5, host, ag._lo, ag._hi)


# ---- 5. the perfect agents are what they were ------------------------------------------------------------------------------
def test_the_perfect_agents_on_their_own_tasks():
    for env, cls in ((make_env(E_ODD, 20, corr=None, autoreset=True), MPCAgentPerfectStream), (make_env(E_ODD, 20, autoreset=True), MPCAgentPerfectChain)):
        env.reset()
        fused = cls(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=3)
        plain = type("UnfusedPerfect", (cls,), {"_fused": lambda self, env: False})(
            env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=3)
        fused.warn_unconverged = plain.warn_unconverged = False
        assert fused._fused(env)
        assert_same_act(fused, plain, env, cls.__name__)
