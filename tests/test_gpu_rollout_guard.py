"""GPU tier: the rollout buffer under guard bands (tests/guard_common.py).  A -- environment and buffer -- is built under the
guarded allocator, B plain, from one seed; both run the same rollout.  After ``begin``, every ``add`` and ``finish`` no guard
byte of A has changed (k_rollout_store, k_rollout_gae, k_adv_partial, k_adv_finish and k_adv_apply write only their slots, and
the idle lanes of a last block nothing), and every buffer of A equals B's bit for bit (0xFF guards read as NaN / -1 / 255: a
read past the rows that mattered would show).  Sizes: one row, a partial wavefront, one row past a wavefront, one slot past
three slabs of 1024."""
import pytest
import torch

from gym_anm_amd.rollout import RolloutBuffer

from guard_common import GuardRegistry
from test_gpu_guard_bands import assert_guarded, bits, env_tensors
from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import box_actions, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAMES = ("obs", "actions", "rewards", "values", "logp", "flags", "advantages", "returns", "adv_norm", "t_seen", "_stats", "_slabs")


def same(a, b, where):
    for n in NAMES:
        x, y = getattr(a, n), getattr(b, n)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x), bits(y)), \
            "%s: %s of the guarded buffer differs from the plain one's" % (where, n)


@pytest.mark.parametrize("dtype,vdt", [(F64, None), (F32, None), (F32, F64)], ids=["f64", "f32", "f32-v64"])
@pytest.mark.parametrize("E_", [1, 63, 65, 1025])
def test_rollout_kernels_write_only_their_slots(E_, dtype, vdt):
    T = 3
    reg = GuardRegistry()

    def build():
        env = make_env("anm6", "thread", "uniform", E_, 2718, io_dtype=dtype, autoreset=True, max_episode_steps=2)
        return env, RolloutBuffer(env, T, gae_lambda=0.95, value_dtype=vdt)

    with reg.guarding():
        ea, a = build()
    eb, b = build()
    assert_guarded(reg, *env_tensors(ea), *(getattr(a, n) for n in NAMES))
    reg.assert_intact("construction")
    oa, _ = device_reset(ea)
    ob, _ = device_reset(eb)
    gen = torch.Generator(device=DEV).manual_seed(7)
    for rnd in range(2):                 # the second rollout begins from obs[T]
        a.begin(oa if rnd == 0 else None)
        b.begin(ob if rnd == 0 else None)
        reg.assert_intact("begin %d" % rnd)
        same(a, b, "begin %d" % rnd)
        for k in range(T):
            u = box_actions(ea, gen)
            for env, buf in ((ea, a), (eb, b)):
                buf.actions[k].copy_(u)
                buf.values[k].copy_(buf.obs[k][:, 0] - 0.5 * buf.obs[k][:, 1])
                buf.add(*env.step(buf.actions[k])[:4])
            reg.assert_intact("add %d of rollout %d" % (k, rnd))
            same(a, b, "add %d of rollout %d" % (k, rnd))
        for buf in (a, b):
            buf.values[T].copy_(buf.obs[T][:, 0] - 0.5 * buf.obs[T][:, 1])
            buf.finish(normalize=True)
        reg.assert_intact("finish %d" % rnd)
        same(a, b, "finish %d" % rnd)
        for buf in (a, b):
            buf.finish(normalize=False)
        reg.assert_intact("finish without the normalisation")
        same(a, b, "finish without the normalisation")
    st = a.stats()
    assert 0 < st["n_valid"] < T * E_ or E_ == 1 and st["n_valid"] <= T
    assert bool((a.flags & 4).any())     # the limit of 2: truncations, and reset slots behind them
