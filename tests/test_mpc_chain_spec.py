"""CPU tier: the perfect forecast of the series-noise task with correlated noise (``MPCAgentPerfectChain``) -- its
specification (gym_anm_amd/rng.py: exo_forecast_corr, exo_forecast_corr_v) against the step of the mode it looks ahead in, and
the sweep of the MPC kernel itself (csrc/anm_mpc.hpp: chain_sweep / act_chain_value), compiled for the host into a stand-alone
program that runs it as k_mpc does -- one thread per lane of a wavefront -- against the specification, bit for bit."""
import ctypes as C
import os
import re
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest

from gym_anm_amd import _lib, codegen, errors, networks, rng
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.model import NetworkModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "hostsim", "_build")

SEED = 0x0123456789ABCDE
OFFSET = (1 << 32) - 2               # the global index of environment 2 sets bit 32
# per environment: (timestep, reset_count, table index).  t = 0 and reset_count = 1 (epoch 0), the table index at period - 1
# (wraps in stage 0) and inside, a large step index, a large epoch
ENVS = [(0, 1, 95), (0, 1, 0), (7, 3, 94), (123456, 2**31 - 1, 50), (2, 9, 17), (11, 2, 93), (95, 4, 1), (3, 1, 60)]
N = 5
RHO = np.array((0.9, 0.5, 0.0, 0.0, 0.99))


def anm6_task():
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo, hi = rng.default_exo_bounds(model)
    ser = anm6easy_series()
    return model, ser, 0.25 * np.abs(ser), lo, hi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def start_states(n_env, n_exo, seed=0):
    """noise states as an episode may hold them: inside the chain's bound, both signs, a zero"""
    z = np.random.default_rng(seed).uniform(-1.5, 1.5, (n_env, n_exo))
    z[0, 0] = 0.0
    return z


# ---- the specification ---------------------------------------------------------------------------------------------------
def test_stage_i_is_the_step_applied_i_plus_1_times():
    model, ser, amp, lo, hi = anm6_task()
    period, innov = ser.shape[1], rng.exo_innovation(RHO)
    assert len(ENVS) == 8 and any(a == period - 1 for _, _, a in ENVS) and any(t == 0 and rc == 1 for t, rc, _ in ENVS)
    assert OFFSET + 2 == 1 << 32
    t, rc, aux = (np.array(x) for x in zip(*ENVS))
    z0 = start_states(len(ENVS), len(lo))
    got_v = rng.exo_forecast_corr_v(SEED, OFFSET, rc, t, N, aux, z0, ser, amp, RHO, innov, lo, hi)
    assert got_v.shape == (len(ENVS), len(lo), N)
    for e, (t_e, rc_e, aux_e) in enumerate(ENVS):
        env, epoch = OFFSET + e, (rc_e - 1) & 0xFFFFFFFF
        got = rng.exo_forecast_corr(SEED, env, epoch, t_e, N, aux_e, z0[e], ser, amp, RHO, innov, lo, hi)
        z = z0[e].copy()
        for i in range(N):                                    # an independent loop over the step of the mode
            want, z = rng.exo_series_corr(SEED, env, epoch, (t_e + 1 + i) & 0xFFFFFFFF, (aux_e + 1 + i) % period, z, ser, amp, RHO,
                                          innov, lo, hi)
            assert (bits(got[:, i]) == bits(want)).all(), (e, i)
        assert (bits(got_v[e]) == bits(got)).all(), e          # the vectorised form: exact
    # (the chain matters: the uncorrelated units aside, the forecast is not the stream forecast)
    plain = rng.exo_forecast_v(SEED, OFFSET, rc, t, N, lo, hi, series=ser, noise=amp, aux=aux)
    assert (bits(got_v[:, 2:4]) == bits(plain[:, 2:4])).all() and (bits(got_v[:, 0]) != bits(plain[:, 0])).any()


def test_two_stages_worked_by_hand():
    """seed 1, environment 2, epoch 0, t = 0, two units, two stages: the episode key and the blocks of steps 1 and 2 are
    those of tests/test_mpc_stream_spec.py (test_hand_worked_values); a unit's 53-bit integer k gives u = k 2^-53 and
    w = 2 u - 1 = (2 k - 2^53) 2^-53 exactly.  With rho = 1/2, c = the double nearest sqrt(3)/2 and z = 1/4 the recurrence
    and the map are worked in exact rationals, each statement rounded once to a double (float(Fraction) rounds correctly):
    t = rd(c w), z' = rd(z / 2 + t), x = rd(amp z' + mean), no clip (infinite ends), at table indices 2 and 0 (period 3)."""
    assert rng.episode_key(1, 2, 0) == 0x711BFE117CC7F52E
    k = {(0, 0): 4954031897238685, (1, 0): 8963569726976825, (0, 1): 1358509835184373, (1, 1): 5848541411001757}   # (unit, stage)
    ser = np.array(((1.0, 2.0, 3.0), (-4.0, -5.0, -6.0)))
    amp = np.array(((0.5, 0.25, 3.0), (1.5, 0.75, 0.125)))
    rho, z0 = np.array((0.5, 0.5)), np.array((0.25, 0.25))
    innov = rng.exo_innovation(rho)
    assert innov[0] == 0.75 ** 0.5
    inf = float("inf")
    got = rng.exo_forecast_corr(1, 2, 0, 0, 2, 1, z0, ser, amp, rho, innov, [-inf, -inf], [inf, inf])
    rd = lambda q: Fraction(float(q))   # noqa: E731
    for u in range(2):
        z = Fraction(z0[u])
        for i, aux in enumerate((2, 0)):
            w = Fraction(2 * k[(u, i)] - 2**53, 2**53)
            t = rd(Fraction(innov[u]) * w)
            z = rd(Fraction(1, 2) * z + t)
            x = rd(Fraction(amp[u, aux]) * z + Fraction(ser[u, aux]))
            assert Fraction(got[u, i]) == x, (u, i)
    gotv = rng.exo_forecast_corr_v(1, 2, [1], [0], 2, [1], z0[None], ser, amp, rho, innov, [-inf, -inf], [inf, inf])[0]
    assert (bits(got) == bits(gotv)).all()
    assert abs(got[0, 0] - 3.634849) < 1e-5     # (u = 0.55, w = 0.1, z' = 0.125 + 0.866 * 0.1 = 0.2116, x = 3 + 3 z')


def test_without_correlation_the_chain_forecast_is_the_stream_forecast():
    """rho = 0: z' = fma(0, z, w) = w whatever z was -- exo_forecast of the uncorrelated task, bit for bit"""
    model, ser, amp, lo, hi = anm6_task()
    n = len(lo)
    rho = np.zeros(n)
    innov = rng.exo_innovation(rho)
    assert (innov == 1.0).all()
    t, rc, aux = (np.array(x) for x in zip(*ENVS))
    want_v = rng.exo_forecast_v(SEED, OFFSET, rc, t, N, lo, hi, series=ser, noise=amp, aux=aux)
    for seed_z, scale in ((1, 1.0), (2, 1e6), (3, 0.0)):
        z0 = start_states(len(ENVS), n, seed_z) * scale
        got_v = rng.exo_forecast_corr_v(SEED, OFFSET, rc, t, N, aux, z0, ser, amp, rho, innov, lo, hi)
        assert (bits(got_v) == bits(want_v)).all()
        for e, (t_e, rc_e, aux_e) in enumerate(ENVS[:3]):
            got = rng.exo_forecast_corr(SEED, OFFSET + e, rc_e - 1, t_e, N, aux_e, z0[e], ser, amp, rho, innov, lo, hi)
            want = rng.exo_forecast(SEED, OFFSET + e, rc_e - 1, t_e, N, lo, hi, series=ser, noise=amp, aux=aux_e)
            assert (bits(got) == bits(want)).all()


# ---- the kernel's own sweep, compiled for the host -----------------------------------------------------------------------
def build_program(kind, sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    if kind == "anm6":
        topo = NetworkModel(networks.anm6_network(), 0.25, 100).topology()
        text = codegen.emit_header(topo, codegen.topology_name(topo))
    else:
        text = codegen.mpc_class_header(kind)
    hdr = os.path.join(OUT, "mpc_chain_check_%s.h" % kind)
    if not os.path.exists(hdr) or open(hdr).read() != text:
        open(hdr, "w").write(text)
    exe = os.path.join(OUT, "mpc_chain_check_%s%s" % (kind, "_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "mpc_chain_check.cpp")
    deps = [src, hdr, os.path.join(ROOT, "include", "anm_mi355x.h")] + [
        os.path.join(codegen.CSRC, f) for f in os.listdir(codegen.CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-ftemplate-depth=4096", "-ffp-contract=off", "-pthread"] + flags +
                             ['-DANM_TOPO_HEADER="%s"' % hdr, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run_program(exe, envs, n_stage, nl, ng, base, lo, hi, rho, innov, z, ser, amp):
    words = [SEED, OFFSET, len(envs), n_stage, nl, ng, ser.shape[1], int(bits([base])[0])]
    for row in envs:
        words += list(row)
    for arr in (lo, hi, rho, innov, z, ser, amp):
        words += [int(w) for w in bits(arr).reshape(-1)]
    res = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
    out = np.array([int(x, 16) for x in res.stdout.split()], dtype=np.uint64)
    return out.reshape(len(envs), n_stage, nl + ng).transpose(0, 2, 1)     # [E, unit, stage]


# horizon -> environments: N = 1 one thread per environment (a whole wavefront and a partial one); 3: an idle fourth lane per
# group; 4: full groups side by side in a row; 16: a row; 17, 33: groups across two and three rows (with idle lanes behind)
HORIZONS = {1: 67, 3: 19, 4: 19, 16: 5, 17: 3, 33: 3}


def check_program(exe, horizons=HORIZONS):
    model, ser, amp, lo, hi = anm6_task()
    nl, ng, base = model.N_load, model.N_non_slack_gen, float(model.baseMVA)
    innov = rng.exo_innovation(RHO)
    clipped = 0
    for n_stage, n_env in horizons.items():
        envs = [(t + 3 * (k // len(ENVS)), rc + k // len(ENVS), (aux + k // len(ENVS)) % ser.shape[1])
                for k in range(n_env) for t, rc, aux in [ENVS[k % len(ENVS)]]]
        z0 = start_states(n_env, nl + ng, n_stage)
        got = run_program(exe, envs, n_stage, nl, ng, base, lo, hi, RHO, innov, z0, ser, amp)
        for e, (t_e, rc_e, aux_e) in enumerate(envs):
            want = rng.exo_forecast_corr(SEED, OFFSET + e, (rc_e - 1) & 0xFFFFFFFF, t_e, n_stage, aux_e, z0[e], ser, amp, RHO,
                                         innov, lo, hi) / base
            assert (got[e] == bits(want)).all(), (n_stage, e)
        raw = got.view(np.float64) * base
        clipped += int((raw[:, 3, :] == hi[3]).sum())
        assert (raw[:, 3, :] < hi[3]).any()
    assert clipped > 0                                       # (the clip bites somewhere, and not everywhere)


@pytest.mark.parametrize("kind", ["anm6", "s1"])
def test_the_kernels_sweep_is_the_specification(kind):
    """mpc::act_chain_value over a wavefront of host threads, for a generated topology (ANM6) and for a padded size class
    that serves it (s1: 8 loads, 2 generators -- the generators' units and the rows of exo_z follow the NETWORK's counts)"""
    check_program(build_program(kind))


def test_the_sweep_under_the_address_and_undefined_behaviour_sanitizers():
    """the same stand-alone program (nothing here is loaded into Python) built with -fsanitize=address,undefined"""
    probe = os.path.join(OUT, "san_probe")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    check_program(build_program("s1", sanitize=True))


# ---- the agent's refusals that need no device ------------------------------------------------------------------------------
def test_the_constructor_refuses_a_task_without_correlated_noise():
    from gym_anm_amd.agents import MPCAgentPerfectChain

    for mode in ("uniform", "host", None):
        with pytest.raises(errors.ArgsError, match="series_noise"):
            MPCAgentPerfectChain(types.SimpleNamespace(exogenous=mode, exo_corr=None), None, 0.995)
    with pytest.raises(errors.ArgsError, match="MPCAgentPerfectStream"):
        MPCAgentPerfectChain(types.SimpleNamespace(exogenous="series_noise", exo_corr=None), None, 0.995)
    agent = object.__new__(MPCAgentPerfectChain)
    for call in (agent.act, agent.forecast):
        with pytest.raises(errors.ArgsError, match="MPCAgentPerfectStream"):
            call(types.SimpleNamespace(exogenous="series_noise", exo_corr=None))
        with pytest.raises(errors.ArgsError, match="series_noise"):
            call(types.SimpleNamespace(exogenous="uniform", exo_corr=None))


# ---- exports and the C ABI ---------------------------------------------------------------------------------------------------
def test_exports_and_abi():
    import gym_anm_amd
    from gym_anm_amd import agents
    from gym_anm_amd.agents import mpc

    assert gym_anm_amd.MPCAgentPerfectChain is agents.MPCAgentPerfectChain is mpc.MPCAgentPerfectChain
    assert "MPCAgentPerfectChain" in dir(gym_anm_amd) and mpc.MPCAgentPerfectChain.FUSED_FORECAST == 4 == _lib.MPC_FORECAST_CHAIN
    # anm_mpc_chain is anm_mpc_stream grown at its tail
    assert issubclass(_lib.MpcChain, _lib.MpcStream)
    for name, _ in _lib.MpcStream._fields_:
        assert getattr(_lib.MpcChain, name).offset == getattr(_lib.MpcStream, name).offset
    assert C.sizeof(_lib.MpcChain) == C.sizeof(_lib.MpcStream) + 24
    assert [getattr(_lib.MpcChain, k).offset - C.sizeof(_lib.MpcStream) for k in ("exo_rho", "exo_innov", "exo_z")] == [0, 8, 16]
    assert "anm_mpc_act_chain_f64" in _lib.ABI and "anm_mpc_act_chain_f64" in _lib.GPU_ONLY and "anm_mpc_act_chain_f64" in _lib.MPC_ABI
    assert _lib.ABI["anm_mpc_act_chain_f64"][1][:-2] == _lib.ABI["anm_mpc_act_stream_f64"][1][:-2]
    text = open(os.path.join(ROOT, "include", "anm_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct anm_mpc_chain \{(.*?)\} anm_mpc_chain;", code, flags=re.S)
    assert m and [s.strip() for s in m.group(1).split(";") if s.strip()] == [
        "anm_mpc_stream exo", "const double* exo_rho", "const double* exo_innov", "const double* exo_z"]
    assert re.search(r"^#define ANM_MPC_FORECAST_CHAIN 4$", code, flags=re.M)
    assert re.search(r"const anm_mpc_opts\* opts,\s*const anm_mpc_chain\* exo, void\* stream\);", code)
