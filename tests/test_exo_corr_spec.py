"""CPU tier: the specification of the correlated noise of the series-noise mode (gym_anm_amd/rng.py: exo_series_corr,
series_corr_init_z and their vectorised forms), the host layers around it, and the device formula itself
(csrc/anm_device.hpp: ExoNoise::advance / map_state) compiled for the host into a stand-alone program, bit for bit.  The GPU
tier (tests/test_gpu_exo_corr.py) holds the kernels to this specification."""
import ctypes as C
import math
import os
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

from gym_anm_amd import _lib, codegen, errors, networks, rng
from gym_anm_amd.envs.anm6 import ANM6EasyVec, ANM6Vec, anm6easy_series
from gym_anm_amd.model import NetworkModel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "hostsim", "_build")
INF = float("inf")

SEED = 0x0123456789ABCDE
# (env, epoch, table index at the reset): environment 1 << 32 sets bit 32 of the global index; epochs 0 and large
KEYS = [(0, 0, 0), (1, 0, 95), (2, 3, 50), (1 << 32, 1, 7), ((1 << 32) + 5, 0, 94), (63, 2**31 - 2, 1), (64, 9, 17), (12345, 1, 60)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def anm6_task():
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo, hi = rng.default_exo_bounds(model)
    ser = anm6easy_series()
    return model, ser, 0.25 * np.abs(ser) + 0.5, lo, hi


def test_hand_worked_values():
    """Seed 1, environment 2, epoch 0 (episode key 0x711bfe117cc7f52e, pinned by tests/test_mpc_stream_spec.py); block 0 of
    steps 0 ... 3 under it gives the 53-bit integers k below, u = k 2^-53 and w = (k - 2^52) 2^-52 exactly.  Unit 0 has
    rho = 1/2 (c = sqrt(3/4) as math.sqrt rounds it), unit 1 has rho = 0.  Three steps from table index 2 of a table of
    period 3 (the index wraps at the first step); the amplitudes are powers of two, so x = amp z + mean rounds once.  The
    high end of unit 0, 11.5, bites at step 1 alone -- and the clip does not feed back into z."""
    assert rng.episode_key(1, 2, 0) == 0x711BFE117CC7F52E
    k = {0: (7687390246004841, 4926066967473602), 1: (4954031897238685, 8963569726976825),
         2: (1358509835184373, 5848541411001757), 3: (4492780548774475, 282703876600806)}   # step -> (unit 0, unit 1)
    assert k[0][0] == 0xDA7D2026E7434E1F >> 11 and k[3][1] == 0x0808F101219F3077 >> 11
    w = {t: [Fraction(kk - 2**52, 2**52) for kk in k[t]] for t in k}
    for t in k:
        assert [Fraction(x) for x in rng.exo_factors(1, 2, 0, t, 2)] == w[t]
    rho = np.array([0.5, 0.0])
    c = rng.exo_innovation(rho)
    assert c[0] == math.sqrt(0.75) and c[1] == 1.0
    ser = np.array([[10.0, 11.0, 12.0], [-3.0, -2.0, -1.0]])
    amp = np.array([[4.0, 4.0, 4.0], [2.0, 2.0, 2.0]])
    lo, hi = np.array([-100.0, -100.0]), np.array([11.5, 100.0])
    z = rng.series_corr_init_z(1, 2, 0, 2)
    assert [Fraction(x) for x in z] == w[0]
    zf = list(w[0])                                    # the chain in exact arithmetic, rounded where the text rounds
    aux, seen = 2, []
    for t in (1, 2, 3):
        aux = (aux + 1) % 3
        P, z = rng.exo_series_corr(1, 2, 0, t, aux, z, ser, amp, rho, c, lo, hi)
        tt = Fraction(float(Fraction(float(c[0])) * w[t][0]))                  # t = c w: a rounded product
        zf[0] = Fraction(float(Fraction(1, 2) * zf[0] + tt))                    # z' = fma(rho, z, t): one rounding
        zf[1] = w[t][1]                                                         # rho = 0: z' = w
        assert [Fraction(x) for x in z] == zf
        x = [float(4 * zf[0] + int(ser[0, aux])), float(2 * zf[1] + int(ser[1, aux]))]
        assert P[0] == min(x[0], 11.5) and P[1] == x[1]
        assert bits(P[1]) == bits(rng.exo_series_noise(1, 2, 0, t, aux, ser, amp, lo, hi)[1])
        seen.append((float(z[0]), float(P[0]), x[0]))
    assert aux == 2
    # z of unit 0: 0.70694353 -> 0.44008821 -> -0.38474493 -> -0.19445293;  x: 11.76035 (clipped to 11.5), 9.46102, 11.22219
    want = [(0.44008821, 11.5, 11.76035284), (-0.38474493, 9.46102029, 9.46102029), (-0.19445293, 11.22218827, 11.22218827)]
    assert np.allclose(seen, want, rtol=0, atol=1e-8) and abs(float(w[0][0]) - 0.70694353) < 1e-8
    assert [s[1] == 11.5 for s in seen] == [True, False, False]


def test_zero_correlation_is_the_uncorrelated_mode_bit_for_bit():
    model, ser, amp, lo, hi = anm6_task()
    n, period = ser.shape
    rho = np.zeros(n)
    c = rng.exo_innovation(rho)
    assert (c == 1.0).all() and any(env >> 32 == 1 for env, _, _ in KEYS) and len(KEYS) == 8
    for env, epoch, aux in KEYS:
        z = rng.series_corr_init_z(SEED, env, epoch, n)
        for t in range(1, 51):
            aux = (aux + 1) % period
            P, z = rng.exo_series_corr(SEED, env, epoch, t, aux, z, ser, amp, rho, c, lo, hi)
            want = rng.exo_series_noise(SEED, env, epoch, t, aux, ser, amp, lo, hi)
            assert (bits(P) == bits(want)).all(), (env, t)
            assert (bits(z) == bits(rng.exo_factors(SEED, env, epoch, t, n))).all()
    # (the clip bites somewhere on this task, and not everywhere: the comparison above covers both arms)
    P = np.array([rng.exo_series_noise(SEED, 0, 0, t, t % period, ser, amp, lo, hi) for t in range(96)])
    assert (P == hi).any() and (P < hi).all(axis=1).any()


def test_the_vectorised_form_is_the_scalar_form_exactly():
    model, ser, amp, lo, hi = anm6_task()
    n, period = ser.shape
    rho = np.array([0.9, 0.5, 0.0, 0.99, 0.25, 0.7, 1e-3])[:n]
    c = rng.exo_innovation(rho)
    env, epoch, aux = (np.array(x, dtype=np.uint64) for x in zip(*KEYS))
    aux = aux.astype(np.int64)
    zv = rng.series_corr_init_z_v(SEED, env, epoch, n)
    zs = [rng.series_corr_init_z(SEED, e, ep, n) for e, ep, _ in KEYS]
    assert (bits(zv) == bits(np.array(zs))).all()
    for t in range(1, 13):
        aux = (aux + 1) % period
        Pv, zv = rng.exo_series_corr_v(SEED, env, epoch, np.uint64(t), aux, zv, ser, amp, rho, c, lo, hi)
        for j, (e, ep, _) in enumerate(KEYS):
            P, zs[j] = rng.exo_series_corr(SEED, e, ep, t, int(aux[j]), zs[j], ser, amp, rho, c, lo, hi)
            assert (bits(Pv[j]) == bits(P)).all() and (bits(zv[j]) == bits(zs[j])).all(), (t, j)


def test_the_initial_z_is_the_factor_behind_the_initial_row():
    """the drawn initial row is that of the uncorrelated mode, series_noise_init_state, for every rho: its loads and
    generator potentials are the map of z = w(step 0) at the drawn table index"""
    model, ser, amp, lo, hi = anm6_task()
    n = ser.shape[0]
    lo2, hi2 = np.full(n, -INF), np.full(n, INF)                 # ends that do not bite: the row shows the factor itself
    for env, epoch, _ in KEYS[:4]:
        z0 = rng.series_corr_init_z(SEED, env, epoch, n)
        assert (bits(z0) == bits(rng.exo_factors(SEED, env, epoch, 0, n))).all() and (np.abs(z0) <= 1).all()
        s0 = rng.series_noise_init_state(model, ser, amp, lo2, hi2, SEED, env, epoch)
        at = int(s0[-1])
        x = [rng.fma(float(amp[i, at]), float(z0[i]), float(ser[i, at])) for i in range(n)]
        got = [s0[k] for k in model.load_idx] + [s0[k] for k in model.gen_idx]
        assert (bits(got) == bits(x)).all()


def test_the_chain_is_stationary_with_the_correlation_asked_for():
    """One chain of N steps at rho = 0.8 -- the specification's own z (ends play no part in z).  Var z = 1/3 and the lag-1
    autocorrelation is rho.  Standard errors, from N and rho alone: se(r1) ~ sqrt((1 - rho^2) / N) (Bartlett, AR(1)); the
    sample variance of N correlated draws is as uncertain as that of N_eff = N (1 - rho^2) / (1 + rho^2) independent ones,
    se(s^2) ~ sigma^2 sqrt(2 / N_eff) -- the Gaussian form, which overstates it for this lighter-tailed chain (uniform
    innovations: excess kurtosis < 0) and so only loosens the 5-sigma band a little.  N = 40 000: about a second."""
    N, rho = 40000, 0.8
    c = float(rng.exo_innovation(rho)[0])
    w = rng.exo_factors_v(SEED, np.uint64(3), np.uint64(0), np.arange(N + 1, dtype=np.uint64), 1)[:, 0]
    z = np.empty(N + 1)
    z[0] = w[0]
    assert bits(z[:1]) == bits(rng.series_corr_init_z(SEED, 3, 0, 1))
    for t in range(1, N + 1):
        z[t] = rng.fma(rho, float(z[t - 1]), c * float(w[t]))
    P, z1 = rng.exo_series_corr(SEED, 3, 0, 1, 0, z[:1], np.zeros((1, 1)), np.ones((1, 1)), [rho], [c], [-INF], [INF])
    assert bits(z1) == bits(z[1:2]) and bits(P) == bits(z[1:2])      # (the loop above is the specification's recurrence)
    z = z[1:]
    bound = c / (1 - rho) + 1
    assert np.abs(z).max() <= bound and np.abs(z).max() > 1.0         # |z| leaves [-1, 1]: bounded by c / (1 - rho) + 1
    var = float(np.mean(z * z))                                       # (the mean is 0 by construction)
    r1 = float(np.mean(z[1:] * z[:-1]) / var)
    n_eff = N * (1 - rho * rho) / (1 + rho * rho)
    se_var, se_r1 = (1 / 3) * math.sqrt(2 / n_eff), math.sqrt((1 - rho * rho) / N)
    print("var %.5f (1/3 +- %.5f)   r1 %.5f (0.8 +- %.5f)   mean %.5f" % (var, se_var, r1, se_r1, z.mean()))
    assert abs(var - 1 / 3) < 5 * se_var
    assert abs(r1 - rho) < 5 * se_r1
    assert 5 * se_var < 0.03 and 5 * se_r1 < 0.02                      # (bands tight enough to tell 0.8 from 0.75 or 0.85)


def test_env_config_corr_extends_the_noise_struct_at_its_tail():
    nz, cr = _lib.EnvConfigNoise, _lib.EnvConfigCorr
    assert issubclass(cr, nz)
    names = lambda cls: [f[0] for c in reversed(cls.__mro__) for f in c.__dict__.get("_fields_", [])]  # noqa: E731
    assert names(cr)[:-3] == names(nz) and names(cr)[-3:] == ["exo_rho", "exo_innov", "exo_z"]
    for n in names(nz):
        assert getattr(cr, n).offset == getattr(nz, n).offset and getattr(cr, n).size == getattr(nz, n).size
    assert cr.exo_rho.offset == C.sizeof(nz) and cr.exo_innov.offset == C.sizeof(nz) + 8 and cr.exo_z.offset == C.sizeof(nz) + 16
    assert C.sizeof(cr) == C.sizeof(nz) + 24
    # the older classes have not moved
    assert C.sizeof(_lib.EnvConfig) == _lib.EnvConfig.exo_high.offset + 8 == 80
    assert C.sizeof(nz) == C.sizeof(_lib.EnvConfigEpisode) + 8 == nz.exo_noise.offset + 8

    def tail(cfg):
        return C.c_int32.from_address(C.addressof(cfg) + _lib.EnvConfig.K.offset + 4).value

    assert tail(cr(K=1)) == _lib.ENV_TAIL_CORR == 3
    assert tail(nz(K=1)) == _lib.ENV_TAIL_NOISE == 2 and tail(_lib.EnvConfigEpisode(K=1)) == 1 and tail(_lib.EnvConfig(K=1)) == 0
    assert not cr(K=1).exo_rho and not cr(K=1).exo_z
    header = open(os.path.join(ROOT, "include", "anm_mi355x.h")).read()
    assert "#define ANM_ENV_TAIL_CORR 3" in header
    body = header.split("typedef struct anm_env_config_corr {")[1].split("}")[0]
    assert [ln.strip() for ln in body.strip().split("\n")] == [
        "anm_env_config_noise cfg;", "const double* exo_rho;", "const double* exo_innov;", "double* exo_z;"]


def _hostsim():
    sys.path.insert(0, HERE)
    from hostsim_backend import hostsim_backend

    return hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())


def _easy(**kw):
    return ANM6EasyVec(num_envs=4, device="cpu", seed=1, _backend=_hostsim(), **kw)


def test_what_the_constructor_refuses_on_the_host_test_double():
    noisy = dict(exogenous="series_noise", exo_noise=0.5)
    with pytest.raises(errors.ArgsError, match="exo_corr needs exogenous='series_noise'"):
        _easy(exo_corr=0.5)
    with pytest.raises(errors.ArgsError, match="exo_corr needs"):
        ANM6Vec("state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 1000]]), costs_clipping=(1, 100), seed=1, num_envs=4,
                device="cpu", _backend=_hostsim(), exogenous="uniform", exo_corr=0.0)
    for bad in (np.zeros(4), np.zeros((5, 2)), np.zeros((1, 5))):
        with pytest.raises(errors.ArgsError, match="exo_corr must be a scalar or have 5 entries"):
            _easy(exo_corr=bad, **noisy)
    for bad in (1.0, -0.1, float("nan"), INF, [0.5, 0.5, 0.5, 0.5, 1.5], [0.0, 0.0, -1e-300, 0.0, 0.0]):
        with pytest.raises(errors.ArgsError, match=r"finite and in \[0, 1\)"):
            _easy(exo_corr=bad, **noisy)
    # a valid correlation: the test double ignores the mode, so the task itself is refused there
    for ok in (0.0, 0.8, [0.9, 0.5, 0.0, 0.0, 0.99]):
        with pytest.raises(errors.EnvInitializationError, match="GPU library"):
            _easy(exo_corr=ok, **noisy)
    env = _easy()
    assert env.exo_corr is None and env.exo_z is None and env.simulator.exo_corr is None


def test_the_mixed_batch_refuses_the_keyword():
    from gym_anm_amd.envs.mixed import MixedBatchedANMEnv

    task = dict(network=networks.anm6_network(), series=anm6easy_series(), exo_corr=0.5)
    with pytest.raises(errors.EnvInitializationError, match="drawn in"):
        MixedBatchedANMEnv([task], np.zeros(4, dtype=np.int64), device="cpu")


def test_the_stream_agent_refuses_a_correlated_task():
    from gym_anm_amd.agents.mpc import MPCAgentPerfectStream

    sim = types.SimpleNamespace(exogenous="series_noise", exo_corr=np.full(5, 0.8))
    with pytest.raises(errors.ArgsError, match="correlated noise"):
        MPCAgentPerfectStream(sim, None, 0.995)
    agent = object.__new__(MPCAgentPerfectStream)
    env = types.SimpleNamespace(_drawn=True, _noisy=True, exo_corr=np.zeros(5))      # (an explicit 0.0 is the new path too)
    with pytest.raises(errors.ArgsError, match="correlated noise"):
        agent.act(env)
    with pytest.raises(errors.ArgsError, match="correlated noise"):
        agent.forecast(env)


# ---- the device formula, compiled for the host ----------------------------------------------------------------------------
def build_program(sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "exo_corr_check" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "exo_corr_check.cpp")
    deps = [src, os.path.join(codegen.CSRC, "anm_device.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def check_program(exe):
    model, ser, amp, lo, hi = anm6_task()
    n, period = ser.shape
    steps = 12
    rho = np.array([0.9, 0.5, 0.0, 0.99, 0.25])
    c = rng.exo_innovation(rho)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1], hi2[1], hi2[4] = -INF, INF, INF                     # infinite ends: no clip on that side
    for low, high in ((lo, hi), (lo2, hi2)):
        words = [SEED, n, period, steps, len(KEYS)]
        for row in KEYS:
            words += list(row)
        for arr in (rho, c, low, high, ser, amp):
            words += [int(x) for x in bits(arr).reshape(-1)]
        res = subprocess.run([exe], input=" ".join(str(x) for x in words) + "\n", capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
        out = [int(x, 16) for x in res.stdout.split()]
        per = n + 2 * n * steps
        assert len(out) == per * len(KEYS)
        clipped = free = 0
        for j, (env, epoch, aux) in enumerate(KEYS):
            got = out[j * per:(j + 1) * per]
            z = rng.series_corr_init_z(SEED, env, epoch, n)
            assert got[:n] == list(bits(z)), j
            zp = np.array(got[n:], dtype=np.uint64).reshape(steps, n, 2)
            for t in range(1, steps + 1):
                aux = (aux + 1) % period
                P, z = rng.exo_series_corr(SEED, env, epoch, t, aux, z, ser, amp, rho, c, low, high)
                assert (zp[t - 1, :, 0] == bits(z)).all() and (zp[t - 1, :, 1] == bits(P)).all(), (j, t)
                clipped += int(((P == low) | (P == high)).sum())
                free += int(((P > low) & (P < high)).sum())
        assert clipped > 0 and free > 0


def test_the_device_formula_is_the_specification():
    """ExoNoise::advance and ExoNoise::map_state as the kernels have them, over 8 episodes of 12 steps"""
    check_program(build_program())


def test_the_device_formula_under_the_address_and_undefined_behaviour_sanitizers():
    """the same stand-alone program (nothing here is loaded into Python) built with -fsanitize=address,undefined"""
    probe = os.path.join(OUT, "san_probe")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    check_program(build_program(sanitize=True))
