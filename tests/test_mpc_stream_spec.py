"""CPU tier: the perfect forecast of the tasks drawn inside the step kernels (``MPCAgentPerfectStream``) -- its specification
(gym_anm_amd/rng.py: exo_forecast, exo_forecast_v) against the draws of the two modes it looks ahead in, and the forecast
gather of the MPC kernel itself (csrc/anm_mpc.hpp: act_forecast in mode ANM_MPC_FORECAST_STREAM), compiled for the host into
a stand-alone program, against the specification, bit for bit."""
import os
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest

from gym_anm_amd import codegen, errors, networks, rng
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.model import NetworkModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "hostsim", "_build")
INF = float("inf")

SEED = 0x0123456789ABCDE
OFFSET = (1 << 32) - 2               # the global index of environment 2 sets bit 32
# per environment: (timestep, reset_count, table index).  t = 0 and reset_count = 1 (epoch 0), the table index at period - 1
# (wraps in stage 0) and inside (50: the solar farm's table then exceeds its p_max), a large step index, a large epoch
ENVS = [(0, 1, 95), (0, 1, 0), (7, 3, 94), (123456, 2**31 - 1, 50), (2, 9, 17)]
N = 5


def anm6_task():
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo, hi = rng.default_exo_bounds(model)
    ser = anm6easy_series()
    return model, ser, 0.25 * np.abs(ser), lo, hi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_fma_v_is_the_correctly_rounded_fused_multiply_add():
    r = np.random.default_rng(0)
    n = 4000
    a = r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)
    b = r.random(n)
    c = -a * b * (1 + r.standard_normal(n) * 10.0 ** r.integers(-17, 1, n))    # cancellation down to the last bits
    c[:50], a[50:100], c[50:75] = 0.0, 0.0, -0.0
    b[100:150], c[100:150] = 0.5, -0.5 * a[100:150]                             # exact zeros
    a[150:160], c[150:160] = 1e-300, 1e-310                                     # outside the range of the expansions
    got = rng.fma_v(a, b, c)
    want = np.array([rng.fma(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])
    assert (bits(got) == bits(want)).all()
    assert (bits(a * b + c) != bits(want)).sum() > 100          # (the plain expression is not the fused one here)


@pytest.mark.parametrize("mode", ["uniform", "noise"])
def test_stage_i_is_the_draw_of_step_t_plus_1_plus_i(mode):
    model, ser, amp, lo, hi = anm6_task()
    period = ser.shape[1]
    assert any(a == period - 1 for _, _, a in ENVS)
    t, rc, aux = (np.array(x) for x in zip(*ENVS))
    kw = dict(series=ser, noise=amp, aux=aux) if mode == "noise" else {}
    got = rng.exo_forecast_v(SEED, OFFSET, rc, t, N, lo, hi, **kw)
    assert got.shape == (len(ENVS), len(lo), N)
    for e, (t_e, rc_e, aux_e) in enumerate(ENVS):
        env, epoch = OFFSET + e, (rc_e - 1) & 0xFFFFFFFF
        kw_e = dict(series=ser, noise=amp, aux=aux_e) if mode == "noise" else {}
        scalar = rng.exo_forecast(SEED, env, epoch, t_e, N, lo, hi, **kw_e)
        for i in range(N):
            if mode == "noise":
                want = rng.exo_series_noise(SEED, env, epoch, t_e + 1 + i, (aux_e + 1 + i) % period, ser, amp, lo, hi)
            else:
                want = rng.exo_uniform(SEED, env, epoch, t_e + 1 + i, lo, hi)
            assert (bits(scalar[:, i]) == bits(want)).all() and (bits(got[e, :, i]) == bits(want)).all(), (e, i)
    assert OFFSET + 2 == 1 << 32


def test_hand_worked_values():
    """seed 1, environment 2, epoch 0, t = 0, two units with the ends [-4, 0] and [0, 8], two stages.  The episode key is
    words 0, 1 of philox(1; (2, 0, 0, 0xFFFFFFFF)) = 0x711bfe117cc7f52e; block 0 of step 1 under it is
    (8ccd537b 86e4e97d fec28dab f799c885), of step 2 (269c75c1 3347ab2f a639bd4a 0e2cea74); a unit's 53-bit integer is
    (word pair) >> 11, u = k 2^-53, and with ends whose difference is a power of two the map is exact:
    -4 + 4 u = -4 (2^53 - k) 2^-53 and 8 u."""
    assert rng.philox4x32(0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]       # Random123's known answer
    assert rng.episode_key(1, 2, 0) == 0x711BFE117CC7F52E
    k = {(0, 0): 4954031897238685, (1, 0): 8963569726976825, (0, 1): 1358509835184373, (1, 1): 5848541411001757}   # (unit, stage)
    assert k[(0, 0)] == 0x8CCD537B86E4E97D >> 11 and k[(1, 1)] == 0xA639BD4A0E2CEA74 >> 11
    got = rng.exo_forecast(1, 2, 0, 0, 2, [-4.0, 0.0], [0.0, 8.0])
    gotv = rng.exo_forecast_v(1, 2, [1], [0], 2, [-4.0, 0.0], [0.0, 8.0])[0]
    for i in range(2):
        assert Fraction(got[0, i]) == Fraction(-4 * (2**53 - k[(0, i)]), 2**53)
        assert Fraction(got[1, i]) == Fraction(8 * k[(1, i)], 2**53)
    assert (bits(got) == bits(gotv)).all()
    assert abs(got[0, 0] + 1.79996789) < 1e-8 and abs(got[1, 1] - 5.19454827) < 1e-8


def test_zero_amplitude_and_infinite_ends_give_the_table_columns():
    """... which is what MPCAgentPerfect.forecast gathers: columns aux + 1 ... aux + N (mod period) of the table"""
    model, ser, amp, lo, hi = anm6_task()
    period = ser.shape[1]
    t, rc, aux = (np.array(x) for x in zip(*ENVS))
    n = ser.shape[0]
    got = rng.exo_forecast_v(SEED, OFFSET, rc, t, N, np.full(n, -INF), np.full(n, INF), series=ser, noise=np.zeros_like(ser), aux=aux)
    idx = (aux[:, None] + 1 + np.arange(N)[None, :]) % period            # agents/mpc.py: MPCAgentPerfect.forecast
    want = ser[:, idx].transpose(1, 0, 2)
    assert (bits(got) == bits(want)).all()
    one = rng.exo_forecast(SEED, OFFSET, 0, 0, N, np.full(n, -INF), np.full(n, INF), series=ser, noise=np.zeros_like(ser), aux=95)
    assert (bits(one) == bits(want[0])).all()


# ---- the kernel's own gather, compiled for the host ----------------------------------------------------------------------
def build_program(kind, sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    if kind == "anm6":
        topo = NetworkModel(networks.anm6_network(), 0.25, 100).topology()
        text = codegen.emit_header(topo, codegen.topology_name(topo))
    else:
        text = codegen.mpc_class_header(kind)
    hdr = os.path.join(OUT, "mpc_stream_check_%s.h" % kind)
    if not os.path.exists(hdr) or open(hdr).read() != text:
        open(hdr, "w").write(text)
    exe = os.path.join(OUT, "mpc_stream_check_%s%s" % (kind, "_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "mpc_stream_check.cpp")
    deps = [src, hdr, os.path.join(ROOT, "include", "anm_mi355x.h")] + [
        os.path.join(codegen.CSRC, f) for f in os.listdir(codegen.CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-ftemplate-depth=4096", "-ffp-contract=off"] + flags +
                             ['-DANM_TOPO_HEADER="%s"' % hdr, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run_program(exe, mode, envs, n_stage, nl, ng, base, lo, hi, ser=None, amp=None, use_aux_index=False):
    period = 0 if ser is None else ser.shape[1]
    words = [{"uniform": 1, "noise": 2}[mode], SEED, OFFSET, len(envs), n_stage, nl, ng, period, int(bits([base])[0]), int(use_aux_index)]
    for row in envs:
        words += list(row)
    for arr in (lo, hi) + (() if ser is None else (ser, amp)):
        words += [int(w) for w in bits(arr).reshape(-1)]
    res = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
    out = np.array([int(x, 16) for x in res.stdout.split()], dtype=np.uint64)
    return out.reshape(len(envs), n_stage, nl + ng).transpose(0, 2, 1)     # [E, unit, stage]


def check_program(exe):
    model, ser, amp, lo, hi = anm6_task()
    nl, ng, base = model.N_load, model.N_non_slack_gen, float(model.baseMVA)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1], hi2[1], hi2[4] = -INF, INF, INF                     # infinite ends: no clip on that side
    for mode, task, aux_index in (("uniform", (lo, hi), False), ("noise", (lo, hi, ser, amp), False), ("noise", (lo2, hi2, ser, amp), True)):
        got = run_program(exe, mode, ENVS, N, nl, ng, base, *task, use_aux_index=aux_index)
        for e, (t_e, rc_e, aux_e) in enumerate(ENVS):
            kw = dict(series=task[2], noise=task[3], aux=aux_e) if mode == "noise" else {}
            want = rng.exo_forecast(SEED, OFFSET + e, (rc_e - 1) & 0xFFFFFFFF, t_e, N, task[0], task[1], **kw) / base
            assert (got[e] == bits(want)).all(), (mode, e)
        if mode == "noise":                                      # (the clip bites somewhere, and not everywhere)
            raw = got.view(np.float64) * base
            assert (raw[:, 3, :] == hi[3]).any() and (raw[:, 3, :] < hi[3]).any()


@pytest.mark.parametrize("kind", ["anm6", "s1"])
def test_the_kernels_gather_in_stream_mode_is_the_specification(kind):
    """mpc::act_forecast in mode 3 over (environment, stage, unit), for a generated topology (ANM6) and for a padded size
    class that serves it (s1: 8 loads, 2 generators -- the generators' units start at the NETWORK's number of loads)"""
    check_program(build_program(kind))


def test_the_gather_under_the_address_and_undefined_behaviour_sanitizers():
    """the same stand-alone program (nothing here is loaded into Python) built with -fsanitize=address,undefined"""
    probe = os.path.join(OUT, "san_probe")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    check_program(build_program("s1", sanitize=True))


# ---- the agents' refusals that need no device ------------------------------------------------------------------------------
def test_perfect_agent_without_tables_names_the_stream_agent():
    from gym_anm_amd.agents.mpc import MPCAgentPerfect

    agent = object.__new__(MPCAgentPerfect)
    with pytest.raises(errors.ArgsError, match="MPCAgentPerfectStream"):
        agent.forecast(types.SimpleNamespace(_series=None))
    with pytest.raises(errors.ArgsError, match="MPCAgentPerfectStream"):
        agent.forecast(object())


def test_stream_agent_refuses_a_simulator_that_is_not_in_a_drawn_mode():
    import sys

    sys.path.insert(0, HERE)
    from hostsim_backend import hostsim_backend

    import gym_anm_amd
    from gym_anm_amd.agents import MPCAgentPerfectStream
    from gym_anm_amd.envs import ANM6EasyVec

    assert gym_anm_amd.MPCAgentPerfectStream is MPCAgentPerfectStream and "MPCAgentPerfectStream" in dir(gym_anm_amd)
    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    env = ANM6EasyVec(num_envs=2, device="cpu", seed=5, _backend=be)
    assert env.simulator.exogenous == "host"
    with pytest.raises(errors.ArgsError, match="drawn inside the step kernels"):
        MPCAgentPerfectStream(env.simulator, env.action_space, env.gamma, planning_steps=2)
    agent = object.__new__(MPCAgentPerfectStream)
    with pytest.raises(errors.ArgsError, match="exogenous"):
        agent.forecast(env)
    with pytest.raises(errors.ArgsError, match="exogenous"):
        agent.act(env)
