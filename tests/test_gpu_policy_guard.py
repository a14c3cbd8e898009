"""GPU tier: the Gaussian MLP policy under guard bands (tests/guard_common.py).  Every tensor ``act`` and ``value`` write --
``actions``, ``values``, ``logp``, ``pi.noise``, ``pi.std`` -- and the environment's own buffers are allocated under the guarded
allocator: after each call no guard byte has changed (k_policy writes only its rows; the idle rows of a last wavefront and the
idle wavefronts of a last workgroup write nothing), the outputs equal those of a plain twin bit for bit (0xFF guards read as
NaN: a read past the rows that mattered would show), and the inputs -- ``pi.flat`` above all -- are bit-identical afterwards."""
import pytest
import torch

from gym_anm_amd.policy import GaussianMLPPolicy

from guard_common import GuardRegistry
from test_gpu_guard_bands import assert_guarded, bits, env_tensors
from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("io,vdt", [(F64, F64), (F32, F32), (F32, F64)], ids=["f64-v64", "f32-v32", "f32-v64"])
@pytest.mark.parametrize("E_", [1, 33])
def test_policy_kernel_writes_only_its_rows(E_, io, vdt):
    reg = GuardRegistry()

    def build():
        env = make_env("anm6", "thread", "uniform", E_, 161, io_dtype=io)
        pi = GaussianMLPPolicy(env, hidden=(64, 64), log_std_init=-0.25, seed=2, init_seed=6)
        out = (torch.zeros((E_, 6), dtype=io, device=DEV), torch.zeros(E_, dtype=vdt, device=DEV), torch.zeros(E_, dtype=vdt, device=DEV))
        return env, pi, out

    with reg.guarding():
        ea, pa, outa = build()
    eb, pb, outb = build()
    assert_guarded(reg, *env_tensors(ea), pa.noise, pa.std, *outa)
    reg.assert_intact("construction")
    oa, _ = device_reset(ea)
    ob, _ = device_reset(eb)
    flat0, obs0 = pa.flat.detach().clone(), oa.clone()
    counters0 = (ea.timestep.clone(), ea._reset_count.clone())

    def compare(where):
        reg.assert_intact(where)
        for x, y in zip(outa + (pa.noise, pa.std), outb + (pb.noise, pb.std)):
            assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), where
        assert torch.equal(bits(pa.flat.detach()), bits(flat0)) and torch.equal(bits(oa), bits(obs0)), where + ": an input changed"
        assert torch.equal(ea.timestep, counters0[0]) and torch.equal(ea._reset_count, counters0[1]), where + ": a counter changed"

    for det in (False, True):
        pa.act(oa, *outa, deterministic=det)
        pb.act(ob, *outb, deterministic=det)
        compare("act, deterministic=%s" % det)
    assert bool(torch.isfinite(outa[0]).all()) and bool(torch.isfinite(outa[2]).all())
    for out in (outa, outb):
        out[1].fill_(3.0)
    pa.value(oa, outa[1])
    pb.value(ob, outb[1])
    compare("value")
    assert not bool((outa[1] == 3.0).any())
