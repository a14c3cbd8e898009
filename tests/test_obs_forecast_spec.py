"""CPU tier: the expected forecast the step and reset kernels write beside the state row
(``BatchedANMEnv(exogenous="series_noise", forecast_horizon=H)``, ``env.exo_forecast``).  The specification is
gym_anm_amd/rng.py (exo_forecast_expected); here: its prefix property and the wrap of the table, the layout of
anm_env_config_forecast, what the constructors refuse, and the device function itself (csrc/anm_device.hpp:
ExoNoise::forecast_row) compiled for the host into a stand-alone program, bit for bit.  The GPU tier
(tests/test_gpu_obs_forecast.py) holds the kernels to the same specification."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gym_anm_amd import _lib, codegen, errors, networks, rng
from gym_anm_amd.envs.anm6 import ANM6EasyVec, ANM6Vec, anm6easy_series
from gym_anm_amd.model import NetworkModel

from test_gpu_exo_noise import task_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "hostsim", "_build")
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def noise_states(n, rows, seed):
    """rows of noise states inside the chain's bound for rho = 0.9 (|z| <= c / (1 - rho) + 1 ~ 5.4), signed zeros among them"""
    z = np.random.default_rng(seed).uniform(-5.0, 5.0, size=(rows, n))
    z[0, 0], z[-1, -1] = 0.0, -0.0
    return z


def rho_for(n):
    rho = np.zeros(n)
    rho[:4] = 0.9, 0.5, 0.0, 0.99
    return rho


# ---- the specification: prefix property, the wrap, the batched form ----------------------------------------------------------
@pytest.mark.parametrize("corr", [True, False])
def test_prefix_property_and_the_wrap_of_a_short_table(corr):
    ser, amp, low, high = task_of("case30")                  # the feeder's table: period 5
    n, period = ser.shape
    assert period == 5
    rho = rho_for(n) if corr else None
    z_rows = noise_states(n, 3, 5)
    for aux, z in zip((0, 3, 4), z_rows):
        kw = dict(aux=aux, z=z if corr else None, series=ser, noise=amp, rho=rho)
        f7, f12 = (rng.exo_forecast_expected(H, low, high, **kw) for H in (7, 12))
        assert f7.shape == (n, 7) and f12.shape == (n, 12)
        assert bits(f12[:, :7]).tobytes() == bits(f7).tobytes()                 # stages 0 .. 6 of 12 are the 7-stage forecast
        for N in (1, 2, 5, 6):
            assert bits(rng.exo_forecast_expected(N, low, high, **kw)).tobytes() == bits(f12[:, :N]).tobytes()
        # every stage by the formula, the table index wrapping at 5: H = 7 wraps once, H = 12 twice
        for u in range(n):
            zb = float(z[u]) if corr else 0.0
            for i in range(12):
                if corr:
                    zb = rng.fma(float(rho[u]), zb, 0.0)
                at = (aux + 1 + i) % 5
                want = rng.noise_clip(rng.fma(float(amp[u, at]), zb, float(ser[u, at])), float(low[u]), float(high[u]))
                assert bits(f12[u, i:i + 1]) == bits([want]), (aux, u, i)
        if not corr:   # no noise state: the forecast is the clipped table, periodic with the table
            assert bits(f12[:, 5:10]).tobytes() == bits(f12[:, :5]).tobytes() and bits(f12[:, 10:]).tobytes() == bits(f12[:, :2]).tobytes()
            clipped = np.clip(ser, low[:, None], high[:, None])
            assert np.array_equal(f12[:, 0], clipped[:, (aux + 1) % 5])
        else:
            assert (f12[:2, 5:10] != f12[:2, :5]).any()      # the noise state decays: not periodic
    # the batched form is the scalar one, row by row
    auxs = np.array([0, 3, 4])
    for H in (7, 12):
        fv = rng.exo_forecast_expected_v(3, H, low, high, aux=auxs, z=z_rows if corr else None, series=ser, noise=amp, rho=rho)
        for e in range(3):
            one = rng.exo_forecast_expected(H, low, high, aux=int(auxs[e]), z=z_rows[e] if corr else None, series=ser, noise=amp, rho=rho)
            assert bits(fv[e]).tobytes() == bits(one).tobytes()


# ---- the C ABI struct ----------------------------------------------------------------------------------------------------------
def test_env_config_forecast_extends_the_corr_struct_at_its_tail():
    cr, fc = _lib.EnvConfigCorr, _lib.EnvConfigForecast
    assert issubclass(fc, cr)
    names = lambda cls: [f[0] for c in reversed(cls.__mro__) for f in c.__dict__.get("_fields_", [])]  # noqa: E731
    assert names(fc)[:-2] == names(cr) and names(fc)[-2:] == ["forecast_horizon", "exo_forecast"]
    for n in names(cr):       # the corr struct is its prefix
        assert getattr(fc, n).offset == getattr(cr, n).offset and getattr(fc, n).size == getattr(cr, n).size
    assert fc.forecast_horizon.offset == C.sizeof(cr) and fc.forecast_horizon.size == 4
    assert fc.exo_forecast.offset == C.sizeof(cr) + 8 and C.sizeof(fc) == C.sizeof(cr) + 16
    # the older classes have not moved
    assert C.sizeof(_lib.EnvConfig) == 80 and C.sizeof(cr) == C.sizeof(_lib.EnvConfigNoise) + 24

    def tail(cfg):
        return C.c_int32.from_address(C.addressof(cfg) + _lib.EnvConfig.K.offset + 4).value

    assert tail(fc(K=1)) == _lib.ENV_TAIL_FORECAST == 5 and tail(cr(K=1)) == _lib.ENV_TAIL_CORR == 3
    c = fc(K=1)
    assert not c.exo_rho and not c.exo_innov and not c.exo_z and not c.exo_forecast and c.forecast_horizon == 0
    header = open(os.path.join(ROOT, "include", "anm_mi355x.h")).read()
    assert "#define ANM_ENV_TAIL_FORECAST 5" in header and "#define ANM_ENV_TAIL_CORR 3" in header
    body = header.split("typedef struct anm_env_config_forecast {")[1].split("}")[0]
    assert [ln.strip() for ln in body.strip().split("\n")] == ["anm_env_config_corr cfg;", "int32_t forecast_horizon;", "void* exo_forecast;"]


# ---- the constructors ---------------------------------------------------------------------------------------------------------
def _hostsim():
    sys.path.insert(0, HERE)
    from hostsim_backend import hostsim_backend

    return hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())


def _easy(**kw):
    return ANM6EasyVec(num_envs=4, device="cpu", seed=1, _backend=_hostsim(), **kw)


def test_what_the_constructor_refuses_on_the_host_test_double():
    noisy = dict(exogenous="series_noise", exo_noise=0.5)
    # any mode other than series_noise
    with pytest.raises(errors.ArgsError, match="forecast_horizon needs exogenous='series_noise'"):
        _easy(forecast_horizon=4)
    with pytest.raises(errors.ArgsError, match="forecast_horizon needs exogenous='series_noise'"):
        _easy(forecast_horizon=4, exogenous="host")
    # H out of range or not an int (checked before the backend is: the test double never sees the task)
    for bad in (0, 65, -1, 1 << 40):
        with pytest.raises(errors.ArgsError, match=r"should be in \[1, 64\]"):
            _easy(forecast_horizon=bad, **noisy)
    for bad in (3.0, "8", True, [4], np.float64(2)):
        with pytest.raises(errors.ArgsError, match="should be an int"):
            _easy(forecast_horizon=bad, **noisy)
    # a backend other than the GPU library: the test double draws nothing, so the task itself is refused there
    for ok in (1, 64, np.int64(7)):
        for corr in (None, 0.8):
            with pytest.raises(errors.EnvInitializationError, match="GPU library"):
                _easy(forecast_horizon=ok, exo_corr=corr, **noisy)
    env = _easy()
    assert env.forecast_horizon is None and env.exo_forecast is None and env.forecast_space is None


def test_the_uniform_mode_refuses_the_keyword():
    with pytest.raises(errors.ArgsError, match="forecast_horizon needs exogenous='series_noise'"):
        ANM6Vec("state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 1000]]), costs_clipping=(1, 100), seed=1, num_envs=4,
                device="cpu", _backend=_hostsim(), exogenous="uniform", forecast_horizon=4)


def test_the_mixed_batch_refuses_the_keyword():
    from gym_anm_amd.envs.mixed import MixedBatchedANMEnv

    task = dict(network=networks.anm6_network(), series=anm6easy_series(), forecast_horizon=8)
    with pytest.raises(errors.EnvInitializationError, match="forecast"):
        MixedBatchedANMEnv([task], np.zeros(4, dtype=np.int64), device="cpu")


# ---- the device function, compiled for the host ------------------------------------------------------------------------------
def build_program(sanitize=False):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "obs_forecast_check" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "hostsim", "obs_forecast_check.cpp")
    deps = [src, os.path.join(codegen.CSRC, "anm_device.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(p) for p in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        res = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
    return exe


def program_tasks():
    """(series, noise, [(low, high), ...]): ANM6's table (period 96; the default ends bite on the solar farm) and the
    feeder's (period 5; ends that bite on every third unit, infinite on unit 1), each also with infinite ends."""
    out = []
    for net in ("anm6", "case30"):
        ser, amp, low, high = task_of(net)
        if net == "anm6":
            amp = amp + 0.5
        lo2, hi2 = low.copy(), high.copy()
        lo2[1], hi2[1], hi2[-1] = -INF, INF, INF
        out.append((ser, amp, [(low, high), (lo2, hi2), (np.full(len(low), -INF), np.full(len(low), INF))]))
    return out


def check_program(exe):
    n_runs = clipped = free = 0
    for ser, amp, ends in program_tasks():
        n, period = ser.shape
        auxs = [0, 1, period // 2, period - 2, period - 1]
        zs = noise_states(n, len(auxs), n)
        for low, high in ends:
            # correlated; rho = 0 with noise states (the states do not reach the forecast); no noise states at all
            for rho, states in ((rho_for(n), 1), (np.zeros(n), 1), (np.zeros(n), 0)):
                for H in (1, 3, 7, 64):
                    words = [n, period, H, len(auxs), states]
                    for aux, z in zip(auxs, zs):
                        words += [aux] + [int(x) for x in bits(z)]
                    for arr in (rho, low, high, ser, amp):
                        words += [int(x) for x in bits(arr).reshape(-1)]
                    res = subprocess.run([exe], input=" ".join(str(x) for x in words) + "\n", capture_output=True, text=True, timeout=120)
                    assert res.returncode == 0, (res.returncode, res.stderr[-4000:])
                    got = np.array([int(x, 16) for x in res.stdout.split()], dtype=np.uint64).reshape(len(auxs), n, H)
                    for r, (aux, z) in enumerate(zip(auxs, zs)):
                        want = rng.exo_forecast_expected(H, low, high, aux=aux, z=z if states else None, series=ser, noise=amp,
                                                         rho=rho if states else None)
                        assert got[r].tobytes() == bits(want).tobytes(), (n, H, states, aux)
                        clipped += int(((want == low[:, None]) | (want == high[:, None])).sum())
                        free += int(((want > low[:, None]) & (want < high[:, None])).sum())
                    n_runs += 1
    assert n_runs == 2 * 3 * 3 * 4 and clipped > 0 and free > 0


def test_the_device_function_is_the_specification():
    """ExoNoise::forecast_row as the kernels have it: H = 1, 3, 7, 64 on both tables, with and without noise states"""
    check_program(build_program())


def test_the_device_function_under_the_address_and_undefined_behaviour_sanitizers():
    """the same stand-alone program (nothing here is loaded into Python) built with -fsanitize=address,undefined"""
    probe = os.path.join(OUT, "san_probe")
    os.makedirs(OUT, exist_ok=True)
    res = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input="int main() { return 0; }\n",
                         capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([probe]).returncode != 0:
        pytest.skip("this g++ has no address / undefined-behaviour sanitizer runtime")
    check_program(build_program(sanitize=True))
