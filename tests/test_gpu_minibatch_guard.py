"""GPU tier: the minibatch sampler under guard bands (tests/guard_common.py).  A -- environment, buffer and sampler -- is built
under the guarded allocator, B plain, from one seed; both run the same rollout.  After ``prepare`` and after every ``gather`` no
guard byte of A has changed (k_mb_count, k_mb_scan, k_mb_scatter and k_mb_gather write only their slots and rows, and the idle
lanes of a last chunk, range or tile nothing), and every tensor of A's sampler equals B's bit for bit (0xFF guards read as
NaN / -1 / 255: a flags byte, an index or a source row read past the end would show).  Sizes: one row, a partial wavefront, one
row past a wavefront, one slot past three ranges of 1024; the batch size does not divide the number of valid slots."""
import pytest
import torch

from gym_anm_amd.minibatch import FIELDS
from gym_anm_amd.rollout import RolloutBuffer

from guard_common import GuardRegistry
from test_gpu_guard_bands import assert_guarded, bits, env_tensors
from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import box_actions, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SCRATCH = ("index", "_counts", "_offsets", "_state")


def tensors(s):
    return dict({k: getattr(s.mb, k) for k in FIELDS}, **{k: getattr(s, k) for k in SCRATCH})


def same(a, b, where):
    xa, xb = tensors(a), tensors(b)
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape and torch.equal(bits(xa[k]), bits(xb[k])), \
            "%s: %s of the guarded sampler differs from the plain one's" % (where, k)


@pytest.mark.parametrize("dtype,vdt", [(F64, None), (F32, None), (F32, F64)], ids=["f64", "f32", "f32-v64"])
@pytest.mark.parametrize("E_", [1, 63, 65, 1025])
def test_sampler_kernels_write_only_their_rows(E_, dtype, vdt):
    T = 3
    reg = GuardRegistry()

    def build():
        env = make_env("anm6", "thread", "uniform", E_, 2718, io_dtype=dtype, autoreset=True, max_episode_steps=2)
        return env, RolloutBuffer(env, T, gae_lambda=0.95, value_dtype=vdt)

    with reg.guarding():
        ea, a = build()
    eb, b = build()
    oa, _ = device_reset(ea)
    ob, _ = device_reset(eb)
    gen = torch.Generator(device=DEV).manual_seed(7)
    a.begin(oa)
    b.begin(ob)
    for k in range(T):
        u = box_actions(ea, gen)
        lp = torch.randn(E_, generator=gen, device=DEV, dtype=F64)
        for env, buf in ((ea, a), (eb, b)):
            buf.actions[k].copy_(u)
            buf.logp[k].copy_(lp)
            buf.values[k].copy_(buf.obs[k][:, 0] - 0.5 * buf.obs[k][:, 1])
            buf.add(*env.step(buf.actions[k])[:4])
    for buf in (a, b):
        buf.values[T].copy_(buf.obs[T][:, 0] - 0.5 * buf.obs[T][:, 1])
        buf.finish(normalize=True)
    n = int(a.valid.sum())
    B = next(x for x in range({1: 3, 63: 50, 65: 50, 1025: 700}[E_], 4096) if n % x != 0)          # does not divide n
    with reg.guarding():
        sa = a.sampler(B, seed=3)
    sb = b.sampler(B, seed=3)
    assert_guarded(reg, *env_tensors(ea), *tensors(sa).values())
    reg.assert_intact("construction")
    for rnd in range(2):
        sa.prepare()
        sb.prepare()
        reg.assert_intact("prepare %d" % rnd)
        same(sa, sb, "prepare %d" % rnd)
        for ep in range(2):
            for m in range(sa.n_minibatches):
                sa.gather(m, ep)
                sb.gather(m, ep)
                reg.assert_intact("gather %d of epoch %d" % (m, ep))
                same(sa, sb, "gather %d of epoch %d" % (m, ep))
    assert sa.state() == dict(rollout_count=2) and sa.count_minibatches() == -(-n // B)
    assert (0 < n < T * E_ or E_ == 1 and n <= T) and n % B != 0
    assert (sa.n_minibatches >= 2 or E_ == 1) and bool((sa.mb.slot == -1).any())          # the last minibatch carries padding rows
