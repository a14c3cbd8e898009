"""CPU tier: the affine policy I/O mode (gym_anm_amd/io_affine.py) -- the two stock maps on the Boxes of ANM6 and of the 30-bus
feeder, the exact evaluations the GPU tests compare the kernels with, and what the host layer refuses without a GPU."""
import os
import sys

import numpy as np
import pytest

from gym_anm_amd import _lib, errors, io_affine, io_dtype, networks, rng
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_io_f32_spec import NETS, state_bounds_vectors  # noqa: E402

EPS = 2.0**-50


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("net", sorted(NETS))
def test_unit_action_map(net):
    lo, hi = (np.asarray(x, np.float64) for x in NetworkModel(NETS[net](), 0.25, 100).action_bounds())
    mid, half = io_affine.unit_action_map(lo, hi)
    assert np.array_equal(mid, 0.5 * lo + 0.5 * hi) and np.array_equal(half, 0.5 * hi - 0.5 * lo) and (half > 0).all()
    ends = io_affine.map_action(np.stack([-np.ones_like(lo), np.ones_like(lo)]), mid, half, lo, hi)
    assert (ends >= lo).all() and (ends <= hi).all() and (ends[0] <= ends[1]).all()          # u = +-1 land inside [lo, hi]
    assert (np.abs(ends[0] - lo) <= 4 * np.spacing(np.abs(lo) + np.abs(hi))).all()            # ... and at its ends
    assert (np.abs(ends[1] - hi) <= 4 * np.spacing(np.abs(lo) + np.abs(hi))).all()
    r = np.random.default_rng(1)
    u = 3 * r.random((200, lo.size)) - 1.5
    a = io_affine.map_action(u, mid, half, lo, hi)
    assert (a >= lo).all() and (a <= hi).all()
    x = np.array([[rng.fma(float(half[j]), float(u[i, j]), float(mid[j])) for j in range(lo.size)] for i in range(200)])
    assert np.array_equal(bits(a), bits(np.where(x < lo, lo, np.where(x > hi, hi, x))))      # the select form on the one-rounding fma
    assert np.array_equal(a[np.abs(u) <= 0.999], x[np.abs(u) <= 0.999])
    for bad_lo, bad_hi in ((np.array([-np.inf, 0.0]), np.array([1.0, 1.0])), (np.array([0.0, 0.0]), np.array([1.0, np.inf])),
                           (np.array([0.0, np.nan]), np.array([1.0, 1.0]))):
        with pytest.raises(errors.ArgsError, match="unit"):
            io_affine.unit_action_map(bad_lo, bad_hi)


def test_map_action_select_form_and_encode():
    mid, half, lo, hi = np.array([1.0, -2.0]), np.array([2.0, 0.5]), np.array([-1.0, -2.5]), np.array([3.0, -1.5])
    u = np.array([[np.nan, 0.0], [2.0, np.nan], [-5.0, 5.0], [-0.0, 0.25]])
    a = io_affine.map_action(u, mid, half, lo, hi)
    assert np.isnan(a[0, 0]) and np.isnan(a[1, 1])                                            # NaN in, NaN out
    assert a[0, 1] == -2.0 and a[1, 0] == 3.0 and a[2, 0] == -1.0 and a[2, 1] == -1.5 and a[3, 0] == 1.0 and a[3, 1] == -1.875
    a32 = io_affine.map_action(u.astype(np.float32), mid, half, lo, hi)                       # float32 u is widened first
    assert a32.dtype == np.float64 and np.array_equal(np.isnan(a32), np.isnan(a)) and np.array_equal(a32[2:], a[2:])
    # the identity tables the library fills in for a part that is not mapped: exact for every u, signed zeros included
    v = np.array([0.0, -0.0, 1e-310, -3.5, 1e300, np.inf, -np.inf])
    ident = io_affine.map_action(v, np.full(7, -0.0), np.ones(7), np.full(7, -np.inf), np.full(7, np.inf))
    assert np.array_equal(bits(ident), bits(v)) and np.array_equal(bits(io_affine.map_obs(v, np.ones(7), np.full(7, -0.0))), bits(v))
    # encode_action follows its definition (and is not the exact inverse)
    a_mw = np.array([[0.3, -1.7], [2.9, -2.4]])
    assert np.array_equal(io_affine.encode_action(a_mw, mid, half), (a_mw - mid) / half)
    back = io_affine.map_action(io_affine.encode_action(a_mw, mid, half), mid, half, lo, hi)
    assert np.allclose(back, a_mw, rtol=0, atol=1e-15)
    torch = pytest.importorskip("torch")
    t = io_affine.encode_action(torch.as_tensor(a_mw), mid, half)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), (a_mw - mid) / half)


@pytest.mark.parametrize("net", sorted(NETS))
def test_box_obs_map(net):
    lo, hi = state_bounds_vectors(NetworkModel(NETS[net](), 0.25, 100))
    lo, hi = np.concatenate([lo, [0.0, 3.0, -np.inf, 2.0]]), np.concatenate([hi, [95.0, 3.0, np.inf, np.inf]])   # aux; degenerate; infinite
    scale, bias = io_affine.box_obs_map(lo, hi)
    prop = np.isfinite(lo) & np.isfinite(hi) & (lo < hi)
    assert prop.sum() > 50 and (~prop).sum() >= 3
    assert (scale[~prop] == 1.0).all() and (bias[~prop] == 0.0).all()                        # infinite and degenerate columns: the identity
    assert (scale > 0).all() and np.isfinite(scale).all() and np.isfinite(bias).all()
    io_affine.check_obs_map(scale, bias, lo.size)
    ilo, ihi = io_affine.observation_image(lo, hi, scale, bias)
    assert (ilo <= ihi).all()                                                                  # mapped bounds are ordered
    assert (ilo[prop] >= -1 - EPS).all() and (ihi[prop] <= 1 + EPS).all()                      # ... and land on about [-1, 1]
    assert (np.abs(ilo[prop] + 1) <= EPS).all() and (np.abs(ihi[prop] - 1) <= EPS).all()
    assert np.array_equal(bits(ilo[~prop]), bits(lo[~prop])) and np.array_equal(bits(ihi[~prop]), bits(hi[~prop]))
    # monotone: a clipped row, mapped, lies inside the image Box -- in float64 and after the float32 rounding
    r = np.random.default_rng(0)
    flo, fhi = np.where(np.isfinite(lo), lo, -50.0), np.where(np.isfinite(hi), hi, 50.0)
    v = np.clip(flo + (fhi - flo) * (1.2 * r.random((64, lo.size)) - 0.1), lo, hi)
    v[:8] = np.where(r.random((8, lo.size)) < 0.5, flo, fhi)                                  # rows that sit on the bounds
    m = io_affine.map_obs(v, scale, bias)
    assert (m >= ilo).all() and (m <= ihi).all()
    lo32, hi32 = io_dtype.observation_bounds32(ilo, ihi)
    m32 = io_dtype.to_float32(m)
    assert m32.dtype == np.float32 and (m32 >= lo32).all() and (m32 <= hi32).all()
    # exact: every entry is the one-rounding fma
    for i, k in ((0, 0), (3, 5), (63, lo.size - 4)):
        assert m[i, k] == rng.fma(float(v[i, k]), float(scale[k]), float(bias[k]))
    # a zero row maps to the bias exactly
    assert np.array_equal(bits(io_affine.map_obs(np.zeros_like(lo), scale, bias)), bits(bias))
    assert np.array_equal(io_affine.map_reward(np.array([-0.0, 0.0, -2e4, -1e-2]), 1 / 64), np.array([-0.0, 0.0, -312.5, -1e-2 / 64]))


def test_arguments_refused_before_any_backend_is_touched():
    args = (networks.anm6_network(), "state", 1, 0.25, 0.995, 100)
    for kw, exc, word in ((dict(action_map="box"), errors.ArgsError, "action_map"), (dict(obs_map="unit"), errors.ArgsError, "obs_map"),
                          (dict(obs_map=np.ones(3)), errors.ArgsError, "obs_map"), (dict(action_map=(1, 2, 3)), errors.ArgsError, "action_map"),
                          (dict(reward_scale=0.0), errors.ArgsError, "reward_scale"), (dict(reward_scale=float("inf")), errors.ArgsError, "reward_scale"),
                          (dict(reward_scale="big"), errors.ArgsError, "reward_scale"),
                          (dict(action_map="unit", variants=[networks.anm6_network()]), errors.EnvInitializationError, "action_map.*variants"),
                          (dict(obs_map="box", track_full=True), errors.EnvInitializationError, "obs_map.*track_full"),
                          (dict(reward_scale=2.0, fuse_observation=False, observation=[("dev_p", "all", "MW")]), errors.EnvInitializationError,
                           "reward_scale.*fuse_observation=False"),
                          (dict(obs_map="box", observation=lambda s: s), errors.EnvInitializationError, "obs_map.*callable")):
        kw = dict(kw)
        a = list(args)
        if "observation" in kw:
            a[1] = kw.pop("observation")
        with pytest.raises(exc, match=word):        # (device="cpu": building the simulator would raise HipExtensionError instead)
            BatchedANMEnv(*a, device="cpu", **kw)
    for bad in (0, -1.0, np.nan, np.inf, None, "x"):
        with pytest.raises(errors.ArgsError, match="reward_scale"):
            io_affine.check_reward_scale(bad)
    with pytest.raises(errors.ArgsError, match="half"):
        io_affine.check_action_map(np.zeros(2), np.array([1.0, 0.0]), -np.ones(2), np.ones(2))
    with pytest.raises(errors.ArgsError, match="scale"):
        io_affine.check_obs_map(np.array([1.0, -1.0]), np.zeros(2), 2)


def test_the_host_backend_and_the_mixed_environment_refuse_the_mode():
    """the test double maps nothing (and has no anm_model_set_io_map): the mode is an error there, not ignored"""
    from hostsim_backend import hostsim_backend

    net = networks.anm6_network()
    be = hostsim_backend(NetworkModel(net, 0.25, 100).topology())
    assert be.device_type == "cpu" and not hasattr(be.lib, "anm_model_set_io_map") and "anm_model_set_io_map" in _lib.GPU_ONLY
    kw = dict(aux_bounds=np.array([[0, 95]]), costs_clipping=(1, 100), num_envs=4, device="cpu", series=anm6easy_series(), _backend=be)
    for maps in (dict(action_map="unit"), dict(obs_map="box"), dict(reward_scale=0.5)):
        with pytest.raises(errors.EnvInitializationError, match="GPU library"):
            BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **maps, **kw)
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **kw)    # the default is today's interface
    assert env.io_map is None and env.raw_action_space is env.action_space and env.reward_scale is None
    a = np.ones((4, 6))
    assert env.encode_action(a) is a
    from gym_anm_amd.envs import MixedBatchedANMEnv

    for maps in (dict(action_map="unit"), dict(obs_map="box"), dict(reward_scale=0.5)):
        with pytest.raises(errors.EnvInitializationError, match="batch views"):
            MixedBatchedANMEnv([dict(network=net, series=anm6easy_series())], [0, 0], **maps)
