"""GPU tier: the running normalisation under guard bands (tests/guard_common.py).  A is built under the guarded allocator, B
plain, from one seed; both run the same loop -- a device reset, steps with the update pair behind them, a masked reset, a
step after it.  After every call no guard byte of A has changed (k_norm_partial, k_norm_finish and k_norm_tables write only
their rows of the statistics, the counters, the slabs, G and t_seen, and nothing beside the arrays they read), and every
output and every normalisation buffer of A equals B's bit for bit (0xFF guards read as NaN / -1: a read past the rows that
mattered would show).  Sizes: one row, a partial wavefront, one row past a wavefront, one row past a slab of 1024."""
import pytest
import torch

from guard_common import GuardRegistry
from test_gpu_guard_bands import assert_guarded, bits, env_tensors, outputs
from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import BOTH, ROLL, box_actions, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def norm_tensors(env):
    return dict(norm_stats=env._norm_stats, norm_counters=env._norm_counters, norm_slabs=env._norm_slabs, norm_G=env._norm_G,
                norm_t_seen=env._norm_t_seen)


def same(a, b, oa, ob, where):
    xa, xb = dict(outputs(a, oa), **norm_tensors(a)), dict(outputs(b, ob), **norm_tensors(b))
    assert list(xa) == list(xb)
    for k in xa:
        assert xa[k].dtype == xb[k].dtype and xa[k].shape == xb[k].shape and torch.equal(bits(xa[k]), bits(xb[k])), \
            "%s: %s of the guarded environment differs from the plain one's" % (where, k)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("E_", [1, 63, 65, 1025])
def test_update_pair_writes_only_its_rows(E_, dtype):
    reg = GuardRegistry()
    build = lambda: make_env("anm6", "thread", "uniform", E_, 2718, io_dtype=dtype, **BOTH, **ROLL)  # noqa: E731
    with reg.guarding():
        a = build()
    b = build()
    assert_guarded(reg, *env_tensors(a), *norm_tensors(a).values())
    reg.assert_intact("construction (anm_model_io_norm_tables)")
    oa, _ = device_reset(a)
    ob, _ = device_reset(b)
    reg.assert_intact("reset")
    same(a, b, oa, ob, "reset")
    gen = torch.Generator(device=DEV).manual_seed(7)
    for t in range(5):
        u = box_actions(a, gen)
        oa, _, _, _, _ = a.step(reg.like(u))
        ob, _, _, _, _ = b.step(u)
        reg.assert_intact("step %d" % t)
        same(a, b, oa, ob, "step %d" % t)
    m = torch.arange(E_, device=DEV) % 3 == 0
    with reg.guarding():
        oa, _ = device_reset(a, reg.like(m))
    ob, _ = device_reset(b, m)
    reg.assert_intact("masked reset")
    same(a, b, oa, ob, "masked reset")
    u = box_actions(a, gen)
    oa, _, _, _, _ = a.step(reg.like(u))
    ob, _, _, _, _ = b.step(u)
    reg.assert_intact("step after the masked reset")
    same(a, b, oa, ob, "step after the masked reset")
    ck = a.norm_state()
    a.load_norm_state(ck)
    b.load_norm_state(ck)
    reg.assert_intact("load_norm_state")
    same(a, b, oa, ob, "load_norm_state")
    assert ck["n_updates"] == 6 and ck["cnt"] > 1e-4
