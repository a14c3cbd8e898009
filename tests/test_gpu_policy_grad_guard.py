"""GPU tier: the PPO gradient under guard bands (tests/guard_common.py).  Every tensor ``g(mb)`` writes -- ``pi.flat.grad``, the
partials, ``ratio``, ``logp``, ``values``, ``inv_std``, ``stats`` -- and the buffer's, the sampler's and the environment's own are
allocated under the guarded allocator: after each call no guard byte has changed (the kernels write only their rows and their
``P`` gradient words; the idle rows of a last wavefront write nothing), the outputs equal those of a plain twin bit for bit
(0xFF guards read as NaN: a read past the rows that mattered would show), and ``pi.flat``, the minibatch and the buffer's tensors
are bit-identical afterwards."""
import pytest
import torch

from gym_anm_amd.minibatch import FIELDS

from guard_common import GuardRegistry
from test_gpu_guard_bands import assert_guarded, bits, env_tensors
from test_gpu_policy import T, make_loop, rollout_once

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BUF = ("obs", "actions", "rewards", "values", "logp", "flags", "advantages", "returns", "adv_norm")


@pytest.mark.parametrize("vdt", [F32, F64], ids=["v32", "v64"])
@pytest.mark.parametrize("B", [1, 33, 100])
def test_gradient_kernels_write_only_their_words(B, vdt):
    reg = GuardRegistry()

    def build():
        env, buf, pi = make_loop(33, 161, vdt)
        sampler = buf.sampler(B, seed=6)
        g = pi.ppo_gradient(B, ent_coef=0.01, vf_clip=0.2)
        return env, buf, pi, sampler, g

    with reg.guarding():
        ea, ba, pa, sa, ga = build()
    eb, bb, pb, sb, gb = build()
    outs = lambda p, g: (p.flat.grad, g.partials, g.ratio, g.logp, g.values, g.inv_std, g.stats)  # noqa: E731
    assert_guarded(reg, *env_tensors(ea), *outs(pa, ga), *(getattr(sa.mb, k) for k in FIELDS), *(getattr(ba, k) for k in BUF))
    reg.assert_intact("construction")
    for env, buf, pi, s in ((ea, ba, pa, sa), (eb, bb, pb, sb)):
        rollout_once(env, buf, pi)
        s.prepare()
    reg.assert_intact("rollout")
    flat0 = pa.flat.detach().clone()
    buf0 = [getattr(ba, k).clone() for k in BUF]
    last = sa.n_minibatches - 1                                 # 0: a full minibatch; the last: padding rows behind the valid ones
    for m in sorted({0, last}, reverse=True):
        mba, mbb = sa.gather(m, 0), sb.gather(m, 0)
        mb0 = [getattr(mba, k).clone() for k in FIELDS]
        ga(mba)
        gb(mbb)
        where = "minibatch %d" % m
        reg.assert_intact(where)
        for x, y in zip(outs(pa, ga), outs(pb, gb)):
            assert x.dtype == y.dtype and torch.equal(bits(x), bits(y)), where
        assert torch.equal(bits(pa.flat.detach()), bits(flat0)), where + ": the parameters changed"
        for k, x in zip(FIELDS, mb0):
            assert torch.equal(bits(getattr(mba, k)), bits(x)), where + ": the minibatch's %s changed" % k
        for k, x in zip(BUF, buf0):
            assert torch.equal(bits(getattr(ba, k)), bits(x)), where + ": the buffer's %s changed" % k
    assert bool(torch.isfinite(pa.flat.grad).all()) and bool(pa.flat.grad.any()) and T == 5
