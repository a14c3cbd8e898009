"""CPU tier: the specification of the uniform exogenous mode (gym_anm_amd/rng.py: exo_uniform, uniform_init_state) and the
host layers around it.  The GPU tier (tests/test_gpu_exo_uniform.py) holds the kernels to this specification."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import numpy.testing as npt
import pytest

from gym_anm_amd import _lib, errors, networks, rng
from gym_anm_amd.envs.anm6 import ANM6Vec, anm6easy_series
from gym_anm_amd.model import NetworkModel

from test_sampler_cpu import KAT


def test_vectorised_philox_equals_the_scalar_one_and_the_known_answers():
    for ctr, key, out in KAT:
        got = rng.philox4x32_v(key[0] | (key[1] << 32), ctr[0] | (ctr[1] << 32), ctr[2], ctr[3])
        assert tuple(int(x) for x in got) == out
    r = np.random.default_rng(11)
    n = 500
    seeds = r.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)
    envs = r.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)
    epochs = r.integers(0, 2**32, n, dtype=np.uint64)
    draws = r.integers(0, 2**32, n, dtype=np.uint64)
    draws[:3] = [0, rng.EXO_KEY_DRAW, rng.EXO_TAG]
    got = rng.philox4x32_v(seeds, envs, epochs, draws)
    for k in range(n):
        assert tuple(int(x) for x in got[k]) == tuple(rng.philox4x32(int(seeds[k]), int(envs[k]), int(epochs[k]), int(draws[k]))), k
    hi, lo = r.integers(0, 2**32, n, dtype=np.uint64), r.integers(0, 2**32, n, dtype=np.uint64)
    npt.assert_array_equal(rng.u01_v(hi, lo), [rng.u01(int(a), int(b)) for a, b in zip(hi, lo)])


def test_vectorised_draws_follow_the_scalar_specification():
    low, high = np.array([-10.0, -3.5, 0.0, 1.25, 2.0]), np.array([0.0, -1.0, 30.0, 1.25, 50.0])
    envs = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 17], dtype=np.uint64)
    epochs = np.array([0, 5, 2**31 - 2, 1, 3], dtype=np.uint64)
    ts = np.array([0, 1, 2, 1000, 2**31 - 1], dtype=np.uint64)
    got = rng.exo_uniform_v(0xFEDCBA9876543210, envs, epochs, ts, low, high)
    for k in range(len(envs)):
        want = rng.exo_uniform(0xFEDCBA9876543210, int(envs[k]), int(epochs[k]), int(ts[k]), low, high)
        npt.assert_allclose(got[k], want, rtol=0, atol=8e-15)      # (one rounding of a value below 64 in magnitude)
        assert ((want >= low) & (want <= high)).all()
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo6, hi6 = rng.default_exo_bounds(model)
    rows = rng.uniform_init_state_v(model, 77, envs, epochs, lo6, hi6)
    for k in range(len(envs)):
        want = rng.uniform_init_state(model, 77, int(envs[k]), int(epochs[k]), lo6, hi6)
        npt.assert_allclose(rows[k], want, rtol=0, atol=8e-15)
        assert want[-1] == 0.0
        npt.assert_array_equal(want[[0, 7, 8, 10, 12, 13]], 0.0)      # slack, load Q, storage P / Q: not drawn


def test_default_ends_are_the_load_and_generator_ranges():
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo, hi = rng.default_exo_bounds(model)
    npt.assert_array_equal(hi[:3], 0.0)
    npt.assert_array_equal(lo[3:], 0.0)
    npt.assert_array_equal(lo[:3], [model.dev_p_min[k] * model.baseMVA for k in model.load_idx])
    npt.assert_array_equal(hi[3:], [model.dev_p_max[k] * model.baseMVA for k in model.gen_idx])
    assert (lo[:3] < 0).all() and (hi[3:] > 0).all()


def test_fraction_fma_agrees_with_plain_arithmetic_where_that_is_exact():
    r = np.random.default_rng(5)
    # small integers and dyadic fractions: products and sums are exact in double precision
    for _ in range(2000):
        a, b, c = (float(r.integers(-2**20, 2**20)) / 2.0 ** int(r.integers(0, 10)) for _ in range(3))
        assert rng.fma(a, b, c) == a * b + c
    assert rng.fma(0.0, 5.0, 0.0) == 0.0 and not np.signbit(rng.fma(0.0, 5.0, 0.0))
    assert np.signbit(rng.fma(-0.0, 5.0, -0.0)) and not np.signbit(rng.fma(3.0, 1.0, -3.0))
    # ... and rounds ONCE where it is not: (1 + e)^2 - 1 = 2 e + e^2 exactly representable, the unfused form loses e^2
    e = 2.0 ** -52
    assert rng.fma(1.0 + e, 1.0 + e, -1.0) == 2 * e + e * e
    assert (1.0 + e) * (1.0 + e) - 1.0 == 2 * e
    for _ in range(500):
        a, b, c = r.standard_normal(3)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        got = rng.fma(a, b, c)
        assert abs(Fraction(got) - exact) <= abs(Fraction(np.nextafter(got, np.inf)) - Fraction(got)) / 2


def test_the_step_stream_shares_no_key_counter_pair_with_the_init_sampler():
    n_gen, n_des, n_exo = 2, 1, 5
    seeds = [0, 1, 0x45584F31, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF]
    envs = [0, 1, 2, 0x45584F31, (1 << 32) - 1, 1 << 32, (0x45584F31 << 32) | 3]
    epochs = [0, 1, 2, 0x45584F31, 2**31 - 1]
    init, exo, n_exo_pairs = set(), set(), 0
    for seed, env, epoch in itertools.product(seeds, envs, epochs):
        init |= rng.init_pairs(seed, env, epoch, n_gen, n_des)
        for t in (0, 1, 2, 3, 0x45584F31, 2**31 - 1):
            p = rng.exo_pairs(seed, env, epoch, t, n_exo)
            assert len(p) == 1 + (n_exo + 1) // 2
            exo |= p
            n_exo_pairs += len(p) - 1
    assert len(init) == len(seeds) * len(envs) * len(epochs) * (2 + (n_gen + n_des + 1) // 2)
    assert not (init & exo)
    # the step blocks of different (episode, step, block) are all different pairs: no stream is used twice
    keyblocks = len(seeds) * len(envs) * len(epochs)
    assert len(exo) == keyblocks + n_exo_pairs
    # the pairs are the ones the draws really use
    seed, env, epoch, t = seeds[4], envs[5], 7, 9
    key = rng.episode_key(seed, env, epoch)
    assert (key, (t, 1, 0, rng.EXO_TAG)) in rng.exo_pairs(seed, env, epoch, t, n_exo)
    assert rng.exo_block(key, t, 1) == rng.philox4x32(key, t | (1 << 32), 0, rng.EXO_TAG)
    assert key == (lambda r: r[0] | (r[1] << 32))(rng.philox4x32(seed, env, epoch, 0xFFFFFFFF))


def test_neighbouring_steps_environments_and_epochs_are_uncorrelated():
    n = 10000
    low, high = np.array([-10.0, 0.0, 0.0]), np.array([0.0, 30.0, 50.0])
    k = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    for what, (env, epoch, t) in {"t": (zero + 5, zero + 3, k), "env": ((1 << 32) - 5000 + k, zero + 3, zero + 7),
                                  "epoch": (zero + 5, k, zero + 7)}.items():
        x = rng.exo_uniform_v(42, env, epoch, t, low, high)
        for i in range(3):
            assert low[i] <= x[:, i].min() and x[:, i].max() < high[i]
            assert abs(np.corrcoef(x[:-1, i], x[1:, i])[0, 1]) < 0.04, (what, i)
            assert abs(x[:, i].mean() - (low[i] + high[i]) / 2) < 0.02 * (high[i] - low[i]), (what, i)
        c = np.corrcoef(x.T)
        assert np.abs(c - np.eye(3)).max() < 0.04, (what, c)
    # the initial state's Q / SoC draws (init sampler) against the step stream at t = 0 of the same episode
    model = NetworkModel(networks.anm6_network(), 0.25, 100)
    lo6, hi6 = rng.default_exo_bounds(model)
    rows = rng.uniform_init_state_v(model, 42, k, zero, lo6, hi6)
    c = np.corrcoef(rows[:, [1, 2, 3, 4, 5, 9, 11, 14]].T)
    assert np.abs(c - np.eye(8)).max() < 0.04, c


def test_env_config_has_the_new_fields_at_the_tail():
    names = [f[0] for f in _lib.EnvConfig._fields_]
    assert names[-3:] == ["exo_mode", "exo_low", "exo_high"]
    assert names[:8] == ["K", "gamma", "clip_e_loss", "clip_penalty", "obs_low", "obs_high", "series", "period"]
    # (the C layout: exo_mode shares the 8-byte slot of period, the pointers follow)
    assert _lib.EnvConfig.exo_mode.offset == _lib.EnvConfig.period.offset + 4
    assert _lib.EnvConfig.exo_low.offset == _lib.EnvConfig.exo_mode.offset + 4
    assert _lib.EnvConfig.exo_high.offset == _lib.EnvConfig.exo_low.offset + 8
    assert C.sizeof(_lib.EnvConfig) == _lib.EnvConfig.exo_high.offset + 8
    cfg = _lib.EnvConfig(K=1, gamma=0.9)        # built by keyword: the tail is zero = today's behaviour
    assert cfg.exo_mode == _lib.EXO_HOST == 0 and not cfg.exo_low and not cfg.exo_high
    assert _lib.EXO_UNIFORM == 1


def _hostsim():
    from hostsim_backend import hostsim_backend

    return hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())


def _anm6(**kw):
    return ANM6Vec("state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 1000]]), costs_clipping=(1, 100), seed=1,
                   num_envs=4, device="cpu", _backend=_hostsim(), **kw)


def test_a_backend_that_is_not_the_gpu_library_refuses_the_mode():
    with pytest.raises(errors.EnvInitializationError, match="GPU library"):
        _anm6(exogenous="uniform")
    env = _anm6()                       # the default stays the host hook
    assert env.exogenous == "host" and env.exo_low is None


def test_the_mode_and_a_series_do_not_go_together():
    with pytest.raises(errors.EnvInitializationError, match="series"):
        _anm6(exogenous="uniform", series=anm6easy_series())


def test_argument_checks():
    with pytest.raises(errors.ArgsError):
        _anm6(exogenous="gaussian")
    with pytest.raises(errors.ArgsError):
        _anm6(exo_low=np.zeros(5))
