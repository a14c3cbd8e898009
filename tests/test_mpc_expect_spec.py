"""CPU tier: the expected forecast of the tasks drawn inside the step kernels (``MPCAgentExpected``) -- its specification
(gym_anm_amd/rng.py: exo_forecast_expected, exo_forecast_expected_v) worked by hand, against its anchors and against what it
claims to be (the conditional mean of the chain forecast), and the value function of the MPC kernel itself (csrc/anm_mpc.hpp:
act_expect_value over chain_sweep), compiled for the host into a stand-alone program that runs it as k_mpc does -- one thread
per lane of a wavefront -- against the specification, bit for bit."""
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

RHO = np.array((0.9, 0.5, 0.0, 0.8, 0.99))


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
def test_two_stages_worked_by_hand():
    """one unit, two stages, in exact rationals, each statement rounded once to a double (float(Fraction) rounds correctly):
    zb_0 = rd(rho z), zb_1 = rd(rho zb_0), x_i = rd(amp_i zb_i + mean_i), no clip (infinite ends), at table indices 2 and 0
    (aux = 1, period 3).  rho = the double nearest 0.8 and z = the double nearest 0.3: neither product is a double."""
    ser, amp = np.array(((1.0, 2.0, 3.0),)), np.array(((0.5, 0.25, 3.0),))
    rho, z = np.array((0.8,)), np.array((0.3,))
    inf = float("inf")
    got = rng.exo_forecast_expected(2, [-inf], [inf], aux=1, z=z, series=ser, noise=amp, rho=rho)
    rd = lambda q: Fraction(float(q))   # noqa: E731
    zb, exact = Fraction(z[0]), []
    for i, at in enumerate((2, 0)):
        prod = Fraction(rho[0]) * zb
        zb = rd(prod)
        exact.append(prod == zb)
        assert Fraction(got[0, i]) == rd(Fraction(amp[0, at]) * zb + Fraction(ser[0, at])), i
    assert exact == [False, False]
    gotv = rng.exo_forecast_expected_v(1, 2, [-inf], [inf], aux=[1], z=z[None], series=ser, noise=amp, rho=rho)[0]
    assert (bits(got) == bits(gotv)).all()
    assert abs(got[0, 0] - (3.0 + 3.0 * 0.24)) < 1e-12 and abs(got[0, 1] - (1.0 + 0.5 * 0.192)) < 1e-12
    # the clip is the mode's compare-select
    clipped = rng.exo_forecast_expected(2, [1.05], [3.5], aux=1, z=z, series=ser, noise=amp, rho=rho)
    assert clipped[0, 0] == 3.5 and clipped[0, 1] == got[0, 1]
    assert rng.exo_forecast_expected(2, [3.8], [9.0], aux=1, z=z, series=ser, noise=amp, rho=rho)[0, 1] == 3.8


@pytest.mark.parametrize("n_stage", [1, 3, 17])
def test_the_vectorised_form_is_the_scalar_form(n_stage):
    model, ser, amp, lo, hi = anm6_task()
    period, n = ser.shape[1], len(lo)
    # the table index comes from the state row: wraps in stage 0 (period - 1), inside the horizon, never
    state = np.zeros((6, 9))
    state[:, -1] = (period - 1, period - 2, 0, 50, period - n_stage, 17)
    aux = state[:, -1].astype(np.int64)
    z = start_states(len(aux), n, n_stage)
    for kw in (dict(aux=aux, z=z, series=ser, noise=amp, rho=RHO), dict(aux=aux, series=ser, noise=amp), dict()):
        got = rng.exo_forecast_expected_v(len(aux), n_stage, lo, hi, **kw)
        assert got.shape == (len(aux), n, n_stage)
        for e in range(len(aux)):
            one = {k: (v[e] if k in ("aux", "z") else v) for k, v in kw.items()}
            assert (bits(got[e]) == bits(rng.exo_forecast_expected(n_stage, lo, hi, **one))).all(), (sorted(kw), e)
    # the table index of stage i is (aux + 1 + i) % period: without noise states and inside the ends, the table itself
    wide = rng.exo_forecast_expected_v(len(aux), n_stage, lo - 1e6, hi + 1e6, aux=aux, series=ser, noise=amp)
    for e in range(len(aux)):
        assert (wide[e] == ser[:, (aux[e] + 1 + np.arange(n_stage)) % period]).all()


def test_anchors():
    model, ser, amp, lo, hi = anm6_task()
    n, n_stage = len(lo), 5
    aux = np.array((95, 0, 94, 50))
    plain = rng.exo_forecast_expected_v(len(aux), n_stage, lo, hi, aux=aux, series=ser, noise=amp)
    # rho = 0 is exo_corr=None, for any finite z: fma(0, z, +0.0) = +0.0
    for seed_z, scale in ((1, 1.0), (2, -1e6), (3, 1e250)):
        z = start_states(len(aux), n, seed_z) * scale
        z[1] = -np.abs(z[1])
        got = rng.exo_forecast_expected_v(len(aux), n_stage, lo, hi, aux=aux, z=z, series=ser, noise=amp, rho=np.zeros(n))
        assert (bits(got) == bits(plain)).all()
        one = rng.exo_forecast_expected(n_stage, lo, hi, aux=aux[1], z=z[1], series=ser, noise=amp, rho=np.zeros(n))
        assert (bits(one) == bits(plain[1])).all()
    # z = 0 is the None form, whatever rho is
    got = rng.exo_forecast_expected_v(len(aux), n_stage, lo, hi, aux=aux, z=np.zeros((len(aux), n)), series=ser, noise=amp, rho=RHO)
    assert (bits(got) == bits(plain)).all()
    assert not np.signbit(ser).any() or (ser[np.signbit(ser)] != 0).all()     # (the tables hold no negative zero)
    # the uniform mode: the map at u = 0.5, every stage
    uni = rng.exo_forecast_expected_v(3, n_stage, lo, hi)
    want = np.array([rng.fma(float(h) - float(l), 0.5, float(l)) for l, h in zip(lo, hi)])
    assert (bits(uni) == bits(np.broadcast_to(want[None, :, None], uni.shape))).all()
    assert (bits(rng.exo_forecast_expected(n_stage, lo, hi)) == bits(np.broadcast_to(want[:, None], (n, n_stage)))).all()


def test_meaning_the_mean_of_the_chain_forecast():
    """the expected forecast is the mean of what the correlated task draws from the same noise states: over M environments
    (their draws are independent) the mean of the chain forecast lies within 5 standard errors of it at every stage and
    unit.  With ends the noise cannot reach and amplitude 1, stage i is table + z_i with z_i = rho^(i+1) z + c sum_k rho^k w,
    Var w = 1/3: standard error sqrt((1 - rho^(2(i+1))) / 3) / sqrt(M).  (Worst deviation found: 2.81 standard errors.)"""
    M, n_stage, rho_s = 4000, 6, 0.8
    ser = anm6easy_series()
    n = ser.shape[0]
    amp, rho = np.ones_like(ser), np.full(n, rho_s)
    lo, hi = np.full(n, -1e6), np.full(n, 1e6)
    z = np.tile(np.linspace(-0.9, 0.9, n), (M, 1))
    aux = np.full(M, 10)
    chain = rng.exo_forecast_corr_v(1234, 0, np.full(M, 3), np.full(M, 7), n_stage, aux, z, ser, amp, rho, rng.exo_innovation(rho), lo, hi)
    want = rng.exo_forecast_expected_v(M, n_stage, lo, hi, aux=aux, z=z, series=ser, noise=amp, rho=rho)
    assert (bits(want) == bits(want[:1])).all()
    se = np.sqrt((1.0 - rho_s ** (2 * (np.arange(n_stage) + 1))) / 3.0) / np.sqrt(M)
    dev = np.abs(chain.mean(axis=0) - want[0]) / se[None, :]
    print("worst deviation: %.2f standard errors" % dev.max())
    assert (dev < 5.0).all(), dev


def test_usefulness_the_noise_state_is_worth_knowing():
    """with the noise states drawn as an episode starts them (stationary: the factors of step index 0), the RMS error of the
    expected forecast against what the task then draws is sqrt(1 - rho^(2(i+1))) of the profile forecast's: below 1 at every
    stage and unit, and within 0.04 of that figure.  (Found: 0.596-0.601, 0.764-0.777, 0.853-0.864, 0.911-0.918 against
    0.600, 0.768, 0.859, 0.912; largest deviation 0.009.)"""
    M, n_stage, rho_s = 4000, 4, 0.8
    ser = anm6easy_series()
    n = ser.shape[0]
    amp, rho = np.ones_like(ser), np.full(n, rho_s)
    lo, hi = np.full(n, -1e6), np.full(n, 1e6)
    z = rng.exo_factors_v(1234, np.arange(M, dtype=np.uint64), np.uint64(2), np.uint64(0), n)
    aux = np.full(M, 10)
    chain = rng.exo_forecast_corr_v(1234, 0, np.full(M, 3), np.zeros(M, dtype=np.int64), n_stage, aux, z, ser, amp, rho,
                                    rng.exo_innovation(rho), lo, hi)
    expected = rng.exo_forecast_expected_v(M, n_stage, lo, hi, aux=aux, z=z, series=ser, noise=amp, rho=rho)
    profile = rng.exo_forecast_expected_v(M, n_stage, lo, hi, aux=aux, series=ser, noise=amp)
    rms = lambda d: np.sqrt((d * d).mean(axis=0))   # noqa: E731
    ratio = rms(expected - chain) / rms(profile - chain)       # [unit, stage]
    want = np.sqrt(1.0 - rho_s ** (2 * (np.arange(n_stage) + 1)))
    print("ratios per stage:", [(round(float(ratio[:, i].min()), 3), round(float(ratio[:, i].max()), 3)) for i in range(n_stage)],
          "against", np.round(want, 3), "largest deviation %.3f" % np.abs(ratio - want[None, :]).max())
    assert (ratio < 1.0).all(), ratio
    assert (np.abs(ratio - want[None, :]) < 0.04).all(), ratio


# ---- the kernel's own value function, compiled for the host --------------------------------------------------------------
def build_program(kind, sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    if kind == "anm6":
        topo = NetworkModel(networks.anm6_network(), 0.25, 100).topology()
        text = codegen.emit_header(topo, codegen.topology_name(topo))
    else:
        text = codegen.mpc_class_header(kind)
    hdr = os.path.join(OUT, "mpc_expect_check_%s.h" % kind)
    if not os.path.exists(hdr) or open(hdr).read() != text:
        open(hdr, "w").write(text)
    exe = os.path.join(OUT, "mpc_expect_check_%s%s" % (kind, "_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "mpc_expect_check.cpp")
    deps = [src, hdr, os.path.join(ROOT, "include", "anm_mi355x.h")] + [
        os.path.join(codegen.CSRC, f) for f in os.listdir(codegen.CSRC) if f.endswith(".hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-ftemplate-depth=4096", "-ffp-contract=off", "-pthread"] + flags +
                             ['-DANM_TOPO_HEADER="%s"' % hdr, "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def run_program(exe, task, aux, n_stage, nl, ng, base, lo, hi, rho, z, ser, amp):
    words = [task, len(aux), n_stage, nl, ng, ser.shape[1], int(bits([base])[0])] + [int(a) for a in aux]
    for arr in (lo, hi, rho, z, ser, amp):
        words += [int(w) for w in bits(arr).reshape(-1)]
    res = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
    out = np.array([int(x, 16) for x in res.stdout.split()], dtype=np.uint64)
    return out.reshape(len(aux), n_stage, nl + ng).transpose(0, 2, 1)     # [E, unit, stage]


# horizon -> environments: N = 1 one thread per environment (a whole wavefront and a partial one); 3: an idle fourth lane per
# group; 4: full groups side by side in a row; 16: a row; 17, 33: groups across two and three rows (with idle lanes behind);
# 64: the whole wavefront
HORIZONS = {1: 67, 3: 19, 4: 19, 16: 5, 17: 3, 33: 3, 64: 2}


def check_program(exe, horizons=HORIZONS):
    model, ser, amp, lo, hi = anm6_task()
    nl, ng, base = model.N_load, model.N_non_slack_gen, float(model.baseMVA)
    n, period = nl + ng, ser.shape[1]
    clipped = 0
    for n_stage, n_env in horizons.items():
        aux = (np.array((period - 1, 0, period - 2, 50, 17, 93, 1, 60))[np.arange(n_env) % 8] + np.arange(n_env) // 8) % period
        z = start_states(n_env, n, n_stage)
        for task in (2, 1, 0):       # correlated, uncorrelated, uniform
            got = run_program(exe, task, aux, n_stage, nl, ng, base, lo, hi, RHO, z, ser, amp)
            kw = {2: dict(aux=aux, z=z, series=ser, noise=amp, rho=RHO), 1: dict(aux=aux, series=ser, noise=amp), 0: dict()}[task]
            want = rng.exo_forecast_expected_v(n_env, n_stage, lo, hi, **kw) / base
            assert (got == bits(want)).all(), (n_stage, task)
            if task == 2:
                raw = got.view(np.float64) * base
                clipped += int((raw[:, 3, :] == hi[3]).sum())
                assert (raw[:, 3, :] < hi[3]).any()
    assert clipped > 0                                       # (the clip bites somewhere, and not everywhere)


@pytest.mark.parametrize("kind", ["anm6", "s1"])
def test_the_kernels_value_function_is_the_specification(kind):
    """mpc::act_expect_value over a wavefront of host threads, for a generated topology (ANM6) and for a padded size class
    that serves it (s1: 8 loads, 2 generators -- the generators' units and the rows of exo_z follow the NETWORK's counts)"""
    check_program(build_program(kind))


def test_the_value_function_under_the_address_and_undefined_behaviour_sanitizers():
    """the same stand-alone program (nothing here is loaded into Python) built with -fsanitize=address,undefined"""
    probe = os.path.join(OUT, "san_probe_expect")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    check_program(build_program("s1", sanitize=True), {1: 67, 3: 19, 17: 3, 64: 2})


# ---- the agent's refusals that need no device ------------------------------------------------------------------------------
def test_the_agent_refuses_a_task_that_is_not_drawn():
    from gym_anm_amd.agents import MPCAgentExpected

    for mode in ("host", "series", None):
        with pytest.raises(errors.ArgsError, match="MPCAgentPerfect.*MPCAgentConstant"):
            MPCAgentExpected(types.SimpleNamespace(exogenous=mode, exo_corr=None), None, 0.995)
    agent = object.__new__(MPCAgentExpected)
    for call in (agent.act, agent.forecast):
        for mode in ("host", None):
            with pytest.raises(errors.ArgsError, match="MPCAgentPerfect.*MPCAgentConstant"):
                call(types.SimpleNamespace(exogenous=mode, exo_corr=None))
    # a drawn mode passes the check (and fails later, on what a SimpleNamespace lacks: not an ArgsError)
    for mode, corr in (("uniform", None), ("series_noise", None), ("series_noise", np.full(5, 0.8))):
        MPCAgentExpected._check_task(mode, "x")
        with pytest.raises(AttributeError):
            MPCAgentExpected(types.SimpleNamespace(exogenous=mode, exo_corr=corr), None, 0.995)


# ---- exports and the C ABI ---------------------------------------------------------------------------------------------------
def test_exports_and_abi():
    import gym_anm_amd
    from gym_anm_amd import agents
    from gym_anm_amd.agents import mpc

    assert gym_anm_amd.MPCAgentExpected is agents.MPCAgentExpected is mpc.MPCAgentExpected
    assert "MPCAgentExpected" in dir(gym_anm_amd) and mpc.MPCAgentExpected.FUSED_FORECAST == 5 == _lib.MPC_FORECAST_EXPECT
    assert issubclass(mpc.MPCAgentExpected, mpc.MPCAgent)
    # anm_mpc_expect: an int32 and five pointers
    assert [name for name, _ in _lib.MpcExpect._fields_] == ["exo_mode", "exo_low", "exo_high", "exo_noise", "exo_rho", "exo_z"]
    assert [getattr(_lib.MpcExpect, k).offset for k, _ in _lib.MpcExpect._fields_] == [0, 8, 16, 24, 32, 40]
    assert C.sizeof(_lib.MpcExpect) == 48 and _lib.MpcExpect.exo_mode.size == 4
    assert "anm_mpc_act_expect_f64" in _lib.ABI and "anm_mpc_act_expect_f64" in _lib.GPU_ONLY and "anm_mpc_act_expect_f64" in _lib.MPC_ABI
    assert _lib.ABI["anm_mpc_act_expect_f64"][1][:-2] == _lib.ABI["anm_mpc_act_chain_f64"][1][:-2]
    assert _lib.ABI["anm_mpc_act_expect_f64"][1][-2]._type_ is _lib.MpcExpect
    text = open(os.path.join(ROOT, "include", "anm_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct anm_mpc_expect \{(.*?)\} anm_mpc_expect;", code, flags=re.S)
    assert m and [s.strip() for s in m.group(1).split(";") if s.strip()] == [
        "int32_t exo_mode", "const double* exo_low", "const double* exo_high", "const double* exo_noise", "const double* exo_rho",
        "const double* exo_z"]
    assert re.search(r"^#define ANM_MPC_FORECAST_EXPECT 5$", code, flags=re.M)
    assert re.search(r"const anm_mpc_opts\* opts,\s*const anm_mpc_expect\* exo, void\* stream\);", code)
