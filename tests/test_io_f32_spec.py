"""CPU tier: the float32 policy-facing I/O mode (gym_anm_amd/io_dtype.py) -- the rounding rules of the spaces on the bounds of
ANM6 and of the 30-bus feeder, and what the host layer refuses without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, io_dtype, networks
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NETS = {"anm6": networks.anm6_network, "case30": lambda: networks.synthetic_radial_network(30, 0)}


def state_bounds_vectors(model):
    """every finite or infinite bound the "state" observation Box and the list forms draw from, as two flat float64 vectors"""
    lo, hi = [], []
    for key, per_id in model.state_bounds().items():
        for units in per_id.values():
            for pair in units.values():
                lo.append(pair[0])
                hi.append(pair[1])
    return np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)


@pytest.mark.parametrize("net", sorted(NETS))
def test_action_bounds_are_rounded_inward(net):
    lo, hi = NetworkModel(NETS[net](), 0.25, 100).action_bounds()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    lo32, hi32 = io_dtype.action_bounds32(lo, hi)
    assert lo32.dtype == np.float32 and hi32.dtype == np.float32 and lo32.shape == lo.shape
    # widened, every bound lies inside the float64 Box ...
    assert (lo32.astype(np.float64) >= lo).all() and (hi32.astype(np.float64) <= hi).all()
    assert (lo32 <= hi32).all()
    # ... and is at most one float32 step from the float64 bound: the next float32 outward is outside (or the bound itself)
    out_lo = np.nextafter(lo32, np.float32(-np.inf)).astype(np.float64)
    out_hi = np.nextafter(hi32, np.float32(np.inf)).astype(np.float64)
    assert (out_lo < lo).all() and (out_hi > hi).all()
    # bounds a float32 holds exactly stay where they are
    exact = lo.astype(np.float32).astype(np.float64) == lo
    assert (lo32[exact].astype(np.float64) == lo[exact]).all()


def test_inward_rounding_on_values_no_float32_holds():
    x = np.array([0.1, -0.1, 1.0, -2.5, 1e-50, -1e-50, 3.5e38, -3.5e38, np.inf, -np.inf, 0.0])
    lo32, hi32 = io_dtype.action_bounds32(x, x)
    assert (lo32.astype(np.float64) >= x).all() and (hi32.astype(np.float64) <= x).all()
    f32max = np.finfo(np.float32).max
    assert hi32[6] == f32max and lo32[6] == np.inf and lo32[7] == -f32max and hi32[7] == -np.inf
    assert hi32[8] == np.inf and lo32[9] == -np.inf
    tiny = np.float32(1e-45)                                      # the smallest subnormal
    assert lo32[4] == tiny and hi32[4] == 0.0 and hi32[5] == -tiny and lo32[5] == 0.0
    assert lo32[0] == np.float32(0.1) and hi32[0] == np.nextafter(np.float32(0.1), np.float32(-np.inf))   # float32(0.1) > 0.1
    assert hi32[1] == np.float32(-0.1) and lo32[1] == np.nextafter(np.float32(-0.1), np.float32(np.inf))
    for k in (2, 3, 10):
        assert lo32[k] == x[k] and hi32[k] == x[k]


@pytest.mark.parametrize("net", sorted(NETS))
def test_observation_bounds_are_rounded_to_nearest(net):
    lo, hi = state_bounds_vectors(NetworkModel(NETS[net](), 0.25, 100))
    assert lo.size > 50
    lo32, hi32 = io_dtype.observation_bounds32(lo, hi)
    for x, x32 in ((lo, lo32), (hi, hi32)):
        assert x32.dtype == np.float32
        fin = np.isfinite(x)
        assert (x32[~fin].astype(np.float64) == x[~fin]).all()
        # nearest: no float32 neighbour is closer
        err = np.abs(x32[fin].astype(np.float64) - x[fin])
        for nb in (np.nextafter(x32[fin], np.float32(np.inf)), np.nextafter(x32[fin], np.float32(-np.inf))):
            assert (err <= np.abs(nb.astype(np.float64) - x[fin])).all()
        # the same conversion as tensor.to(torch.float32), which is what the kernels' stores are tested against
        assert np.array_equal(x32.view(np.int32), torch.from_numpy(x).to(torch.float32).numpy().view(np.int32))
    # monotone: a clipped value, rounded, lies inside the rounded Box
    r = np.random.default_rng(0)
    both = np.isfinite(lo) & np.isfinite(hi)
    v = np.clip(lo[both] + (hi[both] - lo[both]) * r.random((64, both.sum())) * 1.2 - 0.1, lo[both], hi[both])
    v32 = io_dtype.to_float32(v)
    assert (v32 >= lo32[both]).all() and (v32 <= hi32[both]).all()


def test_to_float32_keeps_subnormals_and_overflows_to_inf():
    x = torch.tensor([1e-40, -1e-45, 1e39, -1e39, 0.0, -0.0, 1.0 + 2.0**-24, 1.0 + 3 * 2.0**-24], dtype=torch.float64)
    y = io_dtype.to_float32(x)
    assert y.dtype == torch.float32 and y[0] != 0 and y[1] != 0 and y[2] == float("inf") and y[3] == -float("inf")
    assert y.view(torch.int32)[5] == -(2**31) and y.view(torch.int32)[4] == 0
    assert y[6] == 1.0 and y[7] == 1.0 + 2.0**-22               # ties go to even


def test_io_dtype_argument():
    assert io_dtype.check_io_dtype(None) == torch.float64 and io_dtype.check_io_dtype(torch.float64) == torch.float64
    assert io_dtype.check_io_dtype(torch.float32) == torch.float32 and io_dtype.check_io_dtype(np.float32) == torch.float32
    for bad in (torch.float16, torch.bfloat16, torch.int32, np.float16, "float32", 32):
        with pytest.raises(errors.ArgsError, match="io_dtype"):
            io_dtype.check_io_dtype(bad)
    with pytest.raises(errors.ArgsError, match="io_dtype"):       # ... and the constructor raises before it builds anything
        BatchedANMEnv(networks.anm6_network(), "state", 1, 0.25, 0.995, 100, io_dtype=torch.float16, device="cpu")


def test_the_host_backend_refuses_the_mode():
    """the test double computes in float64 arrays alone (and has no anm_model_set_io): the mode is an error there, not ignored"""
    from hostsim_backend import hostsim_backend

    net = networks.anm6_network()
    be = hostsim_backend(NetworkModel(net, 0.25, 100).topology())
    assert be.device_type == "cpu" and not hasattr(be.lib, "anm_model_set_io") and "anm_model_set_io" in _lib.GPU_ONLY
    kw = dict(aux_bounds=np.array([[0, 95]]), costs_clipping=(1, 100), num_envs=4, device="cpu", series=anm6easy_series(), _backend=be)
    with pytest.raises(errors.EnvInitializationError, match="GPU library"):
        BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, io_dtype=torch.float32, **kw)
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **kw)    # the default is today's interface
    assert env.io_dtype == torch.float64 and env.action_space.dtype == np.float64 and env.observation_space.dtype == np.float64
    assert env.reward.dtype == torch.float64 and env._state_obs.dtype == torch.float64
    from gym_anm_amd.envs import MixedBatchedANMEnv

    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv([dict(network=net, series=anm6easy_series())], [0, 0], io_dtype=torch.float32)
