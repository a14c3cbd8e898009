"""GPU tier: the device rollout buffer (``gym_anm_amd.rollout.RolloutBuffer``, ``anm_rollout_begin`` / ``_add`` / ``_gae`` /
``_adv_norm``; the specification is gym_anm_amd/rollout.py).  Every comparison with the specification is on bit patterns:
float64 through ``int64`` views, float32 through ``int32`` views; no tolerance anywhere.
  1. GAE alone, through the C ABI, on synthetic tensors;  2. the moments on synthetic tensors, over the grids of the slab plan;
  3. the store behind real steps;  4. end to end against the specification run on the buffer's own contents;  5. HIP graph,
  nothing allocated;  6. refusals of the C ABI."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, rollout
from gym_anm_amd.rollout import RolloutBuffer

from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import box_actions, make_env, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
GAMMA, LAM = 0.995, 0.95
V, T_, U = rollout.VALID, rollout.TERMINATED, rollout.TRUNCATED
CODE = {F64: _lib.IO_F64, F32: _lib.IO_F32}
LIMIT = dict(autoreset=True, max_episode_steps=7)


def lib():
    return _lib.load_for_topology(codegen.stock_topologies()["anm6"]).lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tsame(x, y):
    """a device tensor against an array (or another device tensor), bit for bit"""
    return same(x.cpu().numpy(), y.cpu().numpy() if isinstance(y, torch.Tensor) else y)


class Raw:
    """the buffers of the C ABI without an environment: what the kernels of rules 3 and 4 take"""

    def __init__(self, T, E_, rdt, vdt, D=1, slab_doubles=None):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731
        self.T, self.E = T, E_
        self.obs, self.rewards, self.values = z((T + 1, E_, D), rdt), z((T, E_), rdt), z((T + 1, E_), vdt)
        self.flags, self.t_seen = z((T, E_), torch.uint8), z(E_, torch.int32)
        self.advantages, self.returns, self.adv_norm = z((T, E_), vdt), z((T, E_), vdt), z((T, E_), vdt)
        self.stats = z(rollout.STATS_SIZE, F64)
        self.slabs = z(rollout.slab_doubles(T * E_) if slab_doubles is None else slab_doubles, F64)
        self.struct = _lib.Rollout(
            obs=self.obs.data_ptr(), rewards=self.rewards.data_ptr(), values=self.values.data_ptr(), flags=self.flags.data_ptr(),
            advantages=self.advantages.data_ptr(), returns=self.returns.data_ptr(), adv_norm=self.adv_norm.data_ptr(),
            t_seen=self.t_seen.data_ptr(), stats=self.stats.data_ptr(), slabs=self.slabs.data_ptr(), n_slab_doubles=self.slabs.numel(),
            T=T, E=E_, D=D, io_dtype=CODE[rdt], value_dtype=CODE[vdt], gamma=GAMMA, gae_lambda=LAM, eps=1e-8)

    def stats_dict(self):
        s = self.stats.cpu().numpy()
        c = s.view(np.int64)
        return dict(n=float(s[0]), mean=float(s[1]), var=float(s[2]), std=float(s[3]), n_valid=int(c[6]), n_norm_skipped=int(c[7]))


def same_stats(a, b):
    return all(same(np.float64(a[k]), np.float64(b[k])) for k in ("n", "mean", "var", "std")) and \
        a["n_valid"] == b["n_valid"] and a["n_norm_skipped"] == b["n_norm_skipped"]


# ---- 1. GAE alone -----------------------------------------------------------------------------------------------------------------------
def random_flags(shape, gen):
    f = (torch.rand(shape, generator=gen) < 0.8).to(torch.uint8) * V
    f |= (torch.rand(shape, generator=gen) < 0.15).to(torch.uint8) * T_
    f |= (torch.rand(shape, generator=gen) < 0.15).to(torch.uint8) * U
    return f


def sprinkle(x, gen, p):
    """NaN, +inf and -inf over about 3 p of the entries"""
    u = torch.rand(x.shape, generator=gen)
    x[u < p] = float("nan")
    x[(u >= p) & (u < 2 * p)] = float("inf")
    x[(u >= 2 * p) & (u < 3 * p)] = float("-inf")
    return x


# (T = 33: two load blocks of the kernel and one slot; T = 17: one slot past ITS block of 16 slots)
GAE_SHAPES = [(1, 1), (2, 63), (7, 65), (33, 257), (17, 130)]


@pytest.mark.parametrize("vdt", [F64, F32], ids=["v64", "v32"])
@pytest.mark.parametrize("rdt", [F64, F32], ids=["r64", "r32"])
@pytest.mark.parametrize("T,E_", GAE_SHAPES)
def test_gae_alone_against_the_specification(T, E_, rdt, vdt):
    raw = Raw(T, E_, rdt, vdt)
    gen = torch.Generator().manual_seed(100 * T + E_)
    patterns = [torch.full((T, E_), b, dtype=torch.uint8) for b in range(8)] if T * E_ == 1 else []
    for rep, flags in enumerate(patterns + [random_flags((T, E_), gen) for _ in range(3)]):
        r = torch.randn((T, E_), generator=gen, dtype=F64) * 3 - 1
        v = torch.randn((T + 1, E_), generator=gen, dtype=F64) * 5
        if rep % 3 == 2:
            sprinkle(r, gen, 0.01)
            sprinkle(v, gen, 0.01)
        if T >= 2:      # column 0: a termination, then a slot that is no transition; the value between them is never used
            flags[T - 2, 0], flags[T - 1, 0] = V | T_, 0
            r[T - 2:, 0], v[T - 2, 0], v[T - 1:, 0] = 2.0, 0.5, float("nan")
        raw.rewards.copy_(r.to(rdt))
        raw.values.copy_(v.to(vdt))
        raw.flags.copy_(flags)
        raw.advantages.fill_(7.0)
        raw.returns.fill_(7.0)
        assert lib().anm_rollout_gae(C.byref(raw.struct), stream()) == 0, lib().anm_last_error()
        adv, ret = rollout.gae(raw.rewards.cpu().numpy(), raw.values.cpu().numpy(), flags.numpy(), GAMMA, LAM)
        where = "T=%d E=%d rep %d" % (T, E_, rep)
        assert tsame(raw.advantages, adv), where + ": advantages"
        assert tsame(raw.returns, ret), where + ": returns"
        if T >= 2:
            assert adv[T - 2, 0] == 1.5 and ret[T - 2, 0] == 2.0 and adv[T - 1, 0] == 0.0
        if rep % 3 != 2:
            assert np.isfinite(adv).all() or T >= 2 and np.isfinite(np.delete(adv, 0, axis=1)).all()
        else:
            assert T * E_ < 100 or (np.isnan(adv).any() and np.isinf(adv).any())          # used ones do come through


# ---- 2. the moments ----------------------------------------------------------------------------------------------------------------------
# T E: one slot; a partial range; one slot past a quarter range (a wavefront's share); one slot past a slab; three slabs, ragged;
# one slot past the point where the slab doubles to 2048 slots
MOMENT_SHAPES = [(1, 1, F64), (1, 255, F32), (1, 257, F64), (5, 205, F32), (3, 1000, F64), (1, 4096 * 1024 + 1, F32)]


@pytest.mark.parametrize("T,E_,vdt", MOMENT_SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_moments_do_not_depend_on_the_grid(T, E_, vdt):
    raw = Raw(T, E_, F32, vdt)
    assert raw.slabs.numel() == 3 * -(-T * E_ // (2048 if T * E_ > 4096 * 1024 else 1024))
    gen = torch.Generator().manual_seed(T * E_)
    a = (torch.randn((T, E_), generator=gen, dtype=F64) * 2 + 0.75).to(vdt)
    flags = random_flags((T, E_), gen)
    if T * E_ > 1:
        flags.view(-1)[-1] = V          # the last slot counts: a range that dropped it would show
        flags.view(-1)[0] = V
    a[(flags & V) == 0] = float("nan")  # what an invalid slot holds is never read into a sum
    raw.advantages.copy_(a)
    raw.flags.copy_(flags)
    assert lib().anm_rollout_adv_norm(C.byref(raw.struct), stream()) == 0, lib().anm_last_error()
    want, st = rollout.normalise(a.numpy(), flags.numpy())
    got = raw.stats_dict()
    assert same_stats(got, st), (got, st)
    assert tsame(raw.adv_norm, want)
    assert st["n_norm_skipped"] == (1 if T * E_ == 1 else 0)


def test_skipped_normalisations_are_counted_and_copy_the_advantages():
    raw = Raw(3, 70, F32, F32)
    gen = torch.Generator().manual_seed(3)
    a = torch.randn((3, 70), generator=gen, dtype=F32)
    a[1, 5] = float("nan")              # (an invalid slot in every case below)
    skipped = 0
    cases = {"no valid slot": (a, torch.zeros((3, 70), dtype=torch.uint8)), "one valid slot": (a, torch.zeros((3, 70), dtype=torch.uint8))}
    cases["one valid slot"][1][2, 69] = V
    inf = a.clone()
    inf[0, 3] = float("inf")
    most = torch.full((3, 70), V, dtype=torch.uint8)
    most[1, 5] = 0
    cases["an infinite advantage"] = (inf, most)
    cases["a constant column"] = (torch.full((3, 70), 2.5, dtype=F32), most)
    cases["a plain batch"] = (a, most)
    for name, (x, flags) in cases.items():
        raw.advantages.copy_(x)
        raw.flags.copy_(flags)
        raw.adv_norm.fill_(9.0)
        assert lib().anm_rollout_adv_norm(C.byref(raw.struct), stream()) == 0
        want, st = rollout.normalise(x.numpy(), flags.numpy(), n_norm_skipped=skipped)
        assert same_stats(raw.stats_dict(), st), (name, raw.stats_dict(), st)
        assert tsame(raw.adv_norm, want), name
        if name in ("no valid slot", "one valid slot", "an infinite advantage"):
            assert st["n_norm_skipped"] == skipped + 1 and tsame(raw.adv_norm, x.numpy()), name
        else:
            assert st["n_norm_skipped"] == skipped and np.isfinite(want).all() and want[1, 5] == 0.0, name
        skipped = st["n_norm_skipped"]
    assert skipped == 3


# ---- 3. the store -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("net,impl", [("anm6", "thread"), ("case30", "radial")])
def test_store_behind_real_steps(net, impl, dtype, capsys):
    E_, T = 200, 20
    env = make_env(net, impl, "uniform", E_, 31, io_dtype=dtype, **LIMIT)
    obs, _ = device_reset(env)
    buf = RolloutBuffer(env, T, gae_lambda=LAM)
    assert buf.obs.dtype == dtype and buf.values.dtype == dtype and buf.obs.shape == (T + 1, E_, env.observation_N)
    assert buf.actions.shape == (T, E_, env.simulator.dims.action_dim) and buf.flags.dtype == torch.uint8
    buf.begin(obs)
    assert tsame(buf.obs[0], obs) and torch.equal(buf.t_seen, env.timestep)
    gen = torch.Generator(device=DEV).manual_seed(4)
    ts, term, trunc = [env.timestep.cpu().numpy().copy()], [], []
    for k in range(T):
        buf.actions[k].copy_(box_actions(env, gen))
        out = env.step(buf.actions[k])
        o, r, te, tr = (x.clone() for x in out[:4])
        buf.add(*out[:4])
        assert tsame(buf.obs[k + 1], o) and tsame(buf.rewards[k], r), "slot %d" % k
        assert torch.equal(buf.t_seen, env.timestep)
        ts.append(env.timestep.cpu().numpy().copy())
        term.append(te.cpu().numpy())
        trunc.append(tr.cpu().numpy())
    with pytest.raises(Exception, match="full"):
        buf.add(*out[:4])
    seen, want = ts[0], []
    for k in range(T):                   # a host replay of rule 2 from the recorded timesteps
        f, seen = rollout.classify(ts[k + 1], seen, term[k], trunc[k])
        want.append(f)
    want = np.stack(want)
    assert tsame(buf.flags, want)
    assert torch.equal(buf.valid, torch.as_tensor((want & V) != 0, device=DEV))
    resets = (np.stack(ts[1:]) == 0) & ((want & V) == 0)
    assert ((want & V) != 0).any() and ((want & U) != 0).any() and resets.any()          # the limit of 7: truncations and reset slots
    assert (want[resets.nonzero()[0] - 1, resets.nonzero()[1]] & (T_ | U)).all() or (resets.nonzero()[0] == 0).any()
    with capsys.disabled():
        print("\n  %s %s %s: %d valid slots, %d truncations, %d reset slots, %d terminations" % (
            net, impl, str(dtype).replace("torch.", ""), int(((want & V) != 0).sum()), int(((want & V != 0) & (want & U != 0)).sum()),
            int(resets.sum()), int(((want & V != 0) & (want & T_ != 0)).sum())))


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
def value_weights(D, dtype, seed=12):
    return (torch.randn(D, generator=torch.Generator().manual_seed(seed), dtype=F64) * 0.3).to(dtype).to(DEV)


def fill_rollout(env, buf, gen, w):
    """one rollout with random actions and values that are a fixed linear function of obs"""
    T = buf.n_steps
    for k in range(T):
        buf.actions[k].copy_(box_actions(env, gen))
        buf.values[k].copy_((buf.obs[k].to(w.dtype) * w).sum(dim=1))
        buf.add(*env.step(buf.actions[k])[:4])
    buf.values[T].copy_((buf.obs[T].to(w.dtype) * w).sum(dim=1))


@pytest.mark.parametrize("io,vdt", [(F32, None), (F32, F64), (F64, None), (F64, F32)], ids=["f32", "f32-v64", "f64", "f64-v32"])
def test_end_to_end_against_the_specification(io, vdt):
    E_, T = 200, 20
    env = make_env("anm6", "thread", "uniform", E_, 77, io_dtype=io, **LIMIT)
    obs, _ = device_reset(env)
    buf = RolloutBuffer(env, T, gae_lambda=LAM, value_dtype=vdt)
    assert buf.gamma == env.gamma and buf.value_dtype == (io if vdt is None else vdt)
    gen = torch.Generator(device=DEV).manual_seed(8)
    w = value_weights(env.observation_N, buf.value_dtype)
    skipped = 0
    for rnd in range(2):                 # the second rollout continues from obs[T] of the first
        last = buf.obs[T].clone()
        buf.begin(obs if rnd == 0 else None)
        assert rnd == 0 or tsame(buf.obs[0], last)
        fill_rollout(env, buf, gen, w)
        buf.finish(normalize=True)
        r, v, f = buf.rewards.cpu().numpy(), buf.values.cpu().numpy(), buf.flags.cpu().numpy()
        adv, ret = rollout.gae(r, v, f, env.gamma, LAM)
        assert tsame(buf.advantages, adv) and tsame(buf.returns, ret), "rollout %d" % rnd
        norm, st = rollout.normalise(adv, f, buf.adv_eps, skipped)
        assert tsame(buf.adv_norm, norm) and same_stats(buf.stats(), st), (buf.stats(), st)
        assert st["n_norm_skipped"] == 0 and 0 < st["n_valid"] < T * E_ and st["n_valid"] == int(buf.valid.sum())
        assert (f & U).any() and np.isfinite(adv).all()
        m = buf.adv_norm[buf.valid].double()
        assert abs(float(m.mean())) < 1e-5 and abs(float(m.std()) - 1) < 1e-5
    before = buf.adv_norm.clone()
    buf.adv_norm.fill_(3.0)
    buf.finish(normalize=False)          # GAE alone leaves adv_norm and the statistics alone
    assert tsame(buf.advantages, adv) and bool((buf.adv_norm == 3.0).all()) and same_stats(buf.stats(), st)
    buf.finish()
    assert tsame(buf.adv_norm, before)


# ---- 5. HIP graph: a whole rollout, nothing allocated ---------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_allocates_nothing():
    T, E_ = 4, 1025
    kw = dict(io_dtype=F32, **LIMIT)
    envs = [make_env("anm6", "thread", "uniform", E_, 8, **kw) for _ in range(2)]
    bufs, acts = [], []
    for env in envs:
        obs, _ = device_reset(env)
        buf = RolloutBuffer(env, T, gae_lambda=LAM)
        buf.obs[T].copy_(obs)            # begin() continues from obs[T]: the first rollout from the reset
        bufs.append(buf)
        acts.append(torch.zeros_like(buf.actions))

    def one_rollout(env, buf, act):
        buf.begin()
        for k in range(T):
            buf.actions[k].copy_(act[k])                               # the policy's writes, in place
            torch.mul(buf.obs[k][:, 0], 0.5, out=buf.values[k])
            buf.values[k].add_(buf.obs[k][:, 3])
            buf.add(*env.step(buf.actions[k])[:4])
        torch.mul(buf.obs[T][:, 0], 0.5, out=buf.values[T])
        buf.values[T].add_(buf.obs[T][:, 3])
        buf.finish(normalize=True)

    (env, twin), (buf, tbuf), (act, tact) = envs, bufs, acts
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one_rollout(env, buf, act)
    torch.cuda.synchronize()
    assert not bool(env.timestep.any()) and not bool(buf.flags.any())          # capture does not execute
    gc.collect()
    m0 = torch.cuda.memory_allocated()
    gen = torch.Generator(device=DEV).manual_seed(6)
    names = ("obs", "actions", "rewards", "values", "flags", "advantages", "returns", "adv_norm", "t_seen", "_stats")
    for rnd in range(3):
        for k in range(T):
            u = box_actions(env, gen)
            act[k].copy_(u)
            tact[k].copy_(u)
        del u
        m1 = torch.cuda.memory_allocated()
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m1 == m0
        one_rollout(twin, tbuf, tact)
        for n in names:
            assert tsame(getattr(buf, n), getattr(tbuf, n)), "replay %d: %s" % (rnd, n)
        assert torch.equal(env.state, twin.state) and torch.equal(env.timestep, twin.timestep)
    assert buf.stats()["n_valid"] > 0 and bool((buf.flags & U).any())
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    tbuf.begin()                         # eager begin / add / finish allocate nothing either
    for k in range(T):
        out = twin.step(tbuf.actions[k])
        tbuf.add(*out[:4])
    tbuf.finish()
    assert torch.cuda.memory_allocated() == m0


# ---- 6. refusals of the C ABI -------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_carry_a_message_and_launch_nothing():
    L = lib()
    err = lambda: L.anm_last_error()  # noqa: E731
    raw = Raw(3, 1025, F32, F32, D=2)
    src = torch.ones((1025, 2), dtype=F32, device=DEV)
    rew = torch.ones(1025, dtype=F32, device=DEV)
    u8 = torch.ones(1025, dtype=torch.uint8, device=DEV)
    ts = torch.full((1025,), 5, dtype=torch.int32, device=DEV)
    ref = C.byref(raw.struct)
    add = lambda r, k, o=src: L.anm_rollout_add(r, k, o.data_ptr() if o is not None else None, rew.data_ptr(), u8.data_ptr(),  # noqa: E731
                                                 u8.data_ptr(), ts.data_ptr(), None)
    for k in (-1, 3, 2**40):
        assert add(ref, k) != 0 and b"outside [0, T)" in err()
    assert add(None, 0) != 0 and b"null anm_rollout" in err()
    assert add(ref, 0, None) != 0 and b"must be set" in err()
    assert L.anm_rollout_begin(ref, None, ts.data_ptr(), None) != 0 and b"must be set" in err()
    assert L.anm_rollout_begin(None, src.data_ptr(), ts.data_ptr(), None) != 0 and b"null anm_rollout" in err()
    assert L.anm_rollout_gae(None, None) != 0 and L.anm_rollout_adv_norm(None, None) != 0 and b"null anm_rollout" in err()

    def changed(**kw):
        s = _lib.Rollout.from_buffer_copy(raw.struct)
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)

    assert L.anm_rollout_adv_norm(changed(n_slab_doubles=3 * 3), None) != 0 and b"slab buffer is too short" in err()   # 3075 slots: 4 slabs
    assert L.anm_rollout_adv_norm(changed(slabs=None), None) != 0 and b"slab buffer is too short" in err()
    assert L.anm_rollout_adv_norm(changed(stats=None), None) != 0 and b"must be set" in err()
    assert L.anm_rollout_adv_norm(changed(T=2**17), None) != 0 and b"67 108 864" in err()
    assert L.anm_rollout_gae(changed(values=None), None) != 0 and b"must be set" in err()
    assert add(changed(flags=None), 0) != 0 and b"must be set" in err()
    for kw, msg in ((dict(T=0), b"at least 1"), (dict(E=0), b"at least 1"), (dict(D=0), b"at least 1"), (dict(io_dtype=2), b"dtype"),
                    (dict(value_dtype=-1), b"dtype"), (dict(gamma=1.5), b"gamma"), (dict(gae_lambda=float("nan")), b"gae_lambda"),
                    (dict(eps=0.0), b"eps")):
        for call in (lambda r: add(r, 0), lambda r: L.anm_rollout_begin(r, src.data_ptr(), ts.data_ptr(), None),
                     lambda r: L.anm_rollout_gae(r, None), lambda r: L.anm_rollout_adv_norm(r, None)):
            assert call(changed(**kw)) != 0 and msg in err(), kw
    torch.cuda.synchronize()
    for t in (raw.obs, raw.rewards, raw.flags, raw.t_seen, raw.advantages, raw.returns, raw.adv_norm, raw.stats, raw.slabs):
        assert not bool(t.any())         # nothing was launched
    assert add(ref, 2) == 0 and L.anm_rollout_adv_norm(changed(n_slab_doubles=3 * 4), None) == 0       # (four slabs: enough)
    torch.cuda.synchronize()
    assert bool((raw.obs[3] == 1).all()) and not bool(raw.obs[:3].any()) and bool((raw.flags[2] == (V | T_ | U)).all())
    assert bool((raw.t_seen == 5).all()) and bool((raw.rewards[2] == 1).all()) and raw.stats_dict()["n_valid"] == 1025
