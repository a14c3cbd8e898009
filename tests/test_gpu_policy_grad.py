"""GPU tier: the PPO gradient (``gym_anm_amd.policy_grad.PPOGradient``, ``anm_policy_ppo_grad``; the specification is
gym_anm_amd/policy_grad.py).  The two transcendental stages -- ``inv_std`` and ``ratio`` -- are held to mpmath within 1 float32 ulp,
no exclusions; with the device's ``ratio`` and ``inv_std`` read back, ``grad``, ``stats``, ``logp``, ``values`` (and the partials) equal
``policy_grad.backward`` bit for bit.
  1. through the C ABI on synthetic tensors, over the shapes;  2. padding rows, NaN padding, n = 0;  3. refusals;  4. end to end
  behind a real rollout, with Adam;  5. HIP graph."""
import ctypes as C
import gc

import mpmath as mp
import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, errors, policy, policy_grad as PG

from test_gpu_policy import CODE, DEV, F32, F64, NP, SENTINEL, T, lib, make_loop, rollout_once, stream, ulp32

pytestmark = pytest.mark.gpu
PAD = 3
DELTA = np.array([0.5, 0.5, -0.5, -0.5, 0.5, -0.5, 0.05, -0.05])
SIGN = np.array([1, -1, -1, 1, 1, -1, 1, -1])


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


class Raw:
    """the C ABI without an environment: parameters at scale 1, a synthetic minibatch whose actions are draws around the mean"""

    def __init__(self, B, D, A, hidden, activation, io=F32, vdt=F32, R=None, vf_clip=None, dead=(), clip=0.2, vf_coef=0.5, ent_coef=0.01):
        g = torch.Generator().manual_seed(1000 * D + 10 * A + len(hidden))
        self.B, self.D, self.A, self.hidden, self.activation, self.io, self.vdt = B, D, A, tuple(hidden), activation, io, vdt
        self.kw = dict(clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip)
        self.R = PG.rows_per_partial(B) if R is None else R
        self.P = P = policy.layout(D, A, hidden)[1]
        flat = torch.randn(P, generator=g, dtype=F32)
        flat[-A:] = torch.linspace(-1.5, 0.5, A)
        obs = torch.randn((B, D), generator=g, dtype=F64).to(io)
        eps = torch.randn((B, A), generator=g, dtype=F32).numpy()
        self.par = policy.unpack(flat.numpy(), D, A, hidden)
        fw = policy.forward(self.par, obs.numpy(), eps, policy.std_of(flat[-A:].numpy()), activation, value_dtype=NP[vdt])
        idx = np.arange(B) % 8
        adv = SIGN[idx] * (0.2 + np.abs(torch.randn(B, generator=g, dtype=F64).numpy()))
        weight = np.ones(B)
        weight[list(dead)] = 0
        self.host = dict(obs=obs.numpy(), actions=fw["actions"], logp=(fw["logp"].astype(np.float64) - DELTA[idx]).astype(NP[vdt]),
                         values=(fw["values"].astype(np.float64) + 0.3 * torch.randn(B, generator=g, dtype=F64).numpy()).astype(NP[vdt]),
                         returns=torch.randn(B, generator=g, dtype=F64).numpy().astype(NP[vdt]), adv=adv.astype(NP[vdt]),
                         weight=weight.astype(NP[vdt]))
        for k in ("obs", "actions", "logp", "values", "returns", "adv"):
            self.host[k][list(dead)] = 0
        self.flat = flat.to(DEV)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in self.host.items()}
        full = lambda n: torch.full((n,), SENTINEL, dtype=F32, device=DEV)  # noqa: E731
        self.G = -(-B // self.R)
        self.grad, self.partials = full(P + PAD), full(self.G * (P + PG.STATS) + PAD)
        self.ratio, self.logp, self.values = full(B + PAD), full(B + PAD), full(B + PAD)
        self.inv_std, self.stats = full(A + PAD), full(PG.STATS + PAD)
        h3 = list(hidden) + [0] * (3 - len(hidden))
        self.pi = _lib.Policy(params=self.flat.data_ptr(), n_params=P, D=D, A=A, n_hidden=len(hidden), hidden=(C.c_int32 * 3)(*h3),
                              activation=policy.ACTIVATIONS[activation], deterministic=1, E=B, io_dtype=CODE[io], value_dtype=CODE[F32])
        d = self.dev
        self.job = _lib.Ppo(obs=d["obs"].data_ptr(), actions=d["actions"].data_ptr(), logp_old=d["logp"].data_ptr(),
                            values_old=d["values"].data_ptr(), returns=d["returns"].data_ptr(), adv=d["adv"].data_ptr(),
                            weight=d["weight"].data_ptr(), grad=self.grad.data_ptr(), partials=self.partials.data_ptr(),
                            ratio=self.ratio.data_ptr(), logp=self.logp.data_ptr(), values=self.values.data_ptr(),
                            inv_std=self.inv_std.data_ptr(), stats=self.stats.data_ptr(), B=B, rows_per_partial=self.R,
                            io_dtype=CODE[io], value_dtype=CODE[vdt], clip=clip, vf_coef=vf_coef, ent_coef=ent_coef,
                            vf_clip=-1.0 if vf_clip is None else vf_clip)

    def outputs(self):
        return (self.grad, self.partials, self.ratio, self.logp, self.values, self.inv_std, self.stats)

    def run(self):
        rc = lib().anm_policy_ppo_grad(C.byref(self.pi), C.byref(self.job), stream())
        assert rc == 0, lib().anm_last_error()
        torch.cuda.synchronize()

    def push(self):
        for k, v in self.host.items():
            self.dev[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))

    def check(self, where):
        """everything one call wrote, against the specification; -> the specification's dict"""
        B, A, P = self.B, self.A, self.P
        live = self.host["weight"] != 0
        ist, ratio = self.inv_std[:A].cpu().numpy(), self.ratio[:B].cpu().numpy()
        mp.mp.prec = 100
        exact = np.array([float(mp.exp(-mp.mpf(float(x)))) for x in self.par["log_std"]])
        err = np.abs(ist.astype(np.float64) - exact) / ulp32(exact)
        assert err.max() <= 1.0, "%s: inv_std %.2f float32 ulp off exp(-log_std)" % (where, err.max())
        lr = PG.log_ratio(self.par, self.host, ist, self.activation)
        assert np.abs(lr).max() < 2
        exact = np.array([float(mp.exp(mp.mpf(float(x)))) for x in lr[live]])
        if live.any():
            err = np.abs(ratio[live].astype(np.float64) - exact) / ulp32(exact)
            assert err.max() <= 1.0, "%s: ratio %.2f float32 ulp off exp(lr)" % (where, err.max())
        assert not bits(ratio[~live]).any(), where + ": the ratio of a dead row is +0"
        want = PG.backward(self.par, self.host, ratio, ist, self.activation, R=self.R, **self.kw)
        for name, got, n in (("grad", self.grad, P), ("stats", self.stats, PG.STATS), ("logp", self.logp, B), ("values", self.values, B),
                             ("partials", self.partials, self.G * (P + PG.STATS))):
            assert np.array_equal(bits(got[:n].cpu().numpy()), bits(want[name].reshape(-1))), "%s: %s" % (where, name)
        for t, n in zip(self.outputs(), (P, self.G * (P + PG.STATS), B, B, B, A, PG.STATS)):
            assert bool((t[n:] == SENTINEL).all()), where + ": written past the end"
        return want


# ---- 1. the shapes, through the C ABI ------------------------------------------------------------------------------------------------
SHAPES = [(3, 1), (18, 6), (17, 5)]
SERVED = [(32,), (64, 64)]
SIZES = [1, 31, 33, 130]          # plus R + 1 with R = 64: a group of two 32-row steps, then a second group


@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden", SERVED, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("D,A", SHAPES)
def test_gradient_against_the_specification(D, A, hidden, activation):
    for B, R, vf_clip in [(b, None, 0.2 if b == 33 else None) for b in SIZES] + [(65, 64, 0.2)]:
        raw = Raw(B, D, A, hidden, activation, R=R, vf_clip=vf_clip)
        where = "B=%d R=%d" % (B, raw.R)
        raw.run()
        want = raw.check(where)
        if B >= 65:
            h1 = np.abs(policy.layer(raw.host["obs"], *raw.par["actor"][0], activation))
            assert h1.max() > (0.99 if activation == "tanh" else 2.0) and h1.min() < 0.1       # weights at scale 1: the range is spanned
            st = want["stats"]
            assert st[6] == B and 0.2 < st[5] < 0.9 and np.isfinite(want["grad"]).all() and np.abs(want["grad"]).max() > 1e-3
        # the value is the one anm_policy_act writes for the same observations (the critic alone)
        v = torch.full((B + PAD,), SENTINEL, dtype=F32, device=DEV)
        rc = lib().anm_policy_act(C.byref(raw.pi), raw.dev["obs"].data_ptr(), None, v.data_ptr(), None, stream())
        assert rc == 0, lib().anm_last_error()
        assert torch.equal(v[:B].view(torch.int32), raw.values[:B].view(torch.int32)), where + ": values against value()"


@pytest.mark.parametrize("io,vdt", [(F64, F64), (F32, F32), (F32, F64)], ids=["f64-v64", "f32-v32", "f32-v64"])
def test_dtype_pairs(io, vdt):
    for B, R in ((33, None), (130, 64)):
        raw = Raw(B, 18, 6, (64, 64), "tanh", io, vdt, R=R, vf_clip=0.3)
        raw.run()
        raw.check("B=%d" % B)


def test_the_unserved_shape_is_refused():
    raw = Raw(33, 18, 6, (32,), "tanh")
    P = policy.layout(18, 6, (32, 96, 32))[1]
    flat = torch.zeros(P, dtype=F32, device=DEV)
    pi = _lib.Policy.from_buffer_copy(raw.pi)
    pi.params, pi.n_params, pi.n_hidden, pi.hidden = flat.data_ptr(), P, 3, (C.c_int32 * 3)(32, 96, 32)
    assert lib().anm_policy_ppo_grad(C.byref(pi), C.byref(raw.job), stream()) != 0 and b"LDS plan" in lib().anm_last_error()
    with pytest.raises(errors.ArgsError, match="backward pass"):
        PG.check_args(18, 6, (32, 96, 32), 33)


# ---- 2. padding rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdt", [F32, F64], ids=["v32", "v64"])
def test_padding_rows_and_nan_padding(vdt):
    B = 70
    dead = [5] + list(range(61, B))                            # a last minibatch: the tail is padding (and one row inside)
    raw = Raw(B, 18, 6, (64, 64), "tanh", F32, vdt, vf_clip=0.2, dead=dead)
    raw.run()
    want = raw.check("padding")
    assert want["stats"][6] == B - len(dead)
    first = [t.clone() for t in raw.outputs()]
    for k in ("obs", "actions", "logp", "values", "returns", "adv"):
        raw.host[k][dead] = np.nan
    raw.push()
    raw.run()
    for a, b in zip(first, raw.outputs()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    raw.check("NaN padding")
    raw.host["weight"][61] = 1                                 # a NaN row that counts poisons the gradient, as in torch
    raw.push()
    raw.run()
    assert bool(torch.isnan(raw.grad[:raw.P]).all())


def test_empty_minibatch():
    raw = Raw(40, 18, 6, (64, 64), "tanh", dead=range(40), vf_clip=0.2)
    for k in ("obs", "actions", "logp", "values", "returns", "adv"):
        raw.host[k][:] = np.nan
    raw.push()
    raw.run()
    raw.check("n = 0")
    for t, n in ((raw.grad, raw.P), (raw.stats, 8), (raw.ratio, 40), (raw.logp, 40), (raw.values, 40)):
        assert not bool(t[:n].view(torch.int32).any())             # every word +0.0


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_carry_a_message_and_launch_nothing():
    L = lib()
    err = lambda: L.anm_last_error()  # noqa: E731
    raw = Raw(33, 18, 6, (64, 64), "tanh", vf_clip=0.2)

    def changed(base, **kw):
        s = type(base).from_buffer_copy(base)
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    pi, job = C.byref(raw.pi), C.byref(raw.job)
    assert L.anm_policy_ppo_grad(None, job, None) != 0 and b"null anm_policy" in err()
    assert L.anm_policy_ppo_grad(pi, None, None) != 0 and b"null anm_ppo" in err()
    for kw, msg in ((dict(D=0), b"D is"), (dict(A=65), b"A is"), (dict(n_hidden=4), b"n_hidden"), (dict(hidden=(C.c_int32 * 3)(64, 48, 0)), b"multiple of 32"),
                    (dict(activation=2), b"activation"), (dict(n_params=11212), b"layout"), (dict(params=None), b"must be set")):
        assert L.anm_policy_ppo_grad(changed(raw.pi, **kw), job, None) != 0 and msg in err(), kw
    big = policy.layout(18, 6, (96, 96))[1]
    assert L.anm_policy_ppo_grad(changed(raw.pi, hidden=(C.c_int32 * 3)(96, 96, 0), n_params=big), job, None) != 0 and b"LDS plan" in err()
    for kw, msg in ((dict(B=0), b"B is"), (dict(B=(1 << 24) + 1), b"B is"), (dict(rows_per_partial=0), b"rows_per_partial"),
                    (dict(rows_per_partial=48), b"rows_per_partial"), (dict(io_dtype=2), b"dtype"), (dict(value_dtype=-1), b"dtype"),
                    (dict(clip=0.0), b"clip"), (dict(clip=float("nan")), b"clip"), (dict(vf_coef=float("inf")), b"finite"),
                    (dict(ent_coef=float("nan")), b"finite"), (dict(vf_clip=float("nan")), b"finite"), (dict(values_old=None), b"values_old"),
                    (dict(obs=None), b"must be set"), (dict(actions=None), b"must be set"), (dict(logp_old=None), b"must be set"),
                    (dict(returns=None), b"must be set"), (dict(adv=None), b"must be set"), (dict(weight=None), b"must be set"),
                    (dict(grad=None), b"must be set"), (dict(partials=None), b"must be set"), (dict(ratio=None), b"must be set"),
                    (dict(logp=None), b"must be set"), (dict(values=None), b"must be set"), (dict(inv_std=None), b"must be set"),
                    (dict(stats=None), b"must be set")):
        assert L.anm_policy_ppo_grad(pi, changed(raw.job, **kw), None) != 0 and msg in err(), kw
    torch.cuda.synchronize()
    for t in raw.outputs():
        assert bool((t == SENTINEL).all())                     # nothing was launched
    assert L.anm_policy_ppo_grad(pi, changed(raw.job, vf_clip=-1.0, values_old=None), None) == 0     # off: values_old is not read
    torch.cuda.synchronize()
    assert bool(torch.isfinite(raw.grad[:raw.P]).all())


# ---- 4. end to end behind a real rollout ---------------------------------------------------------------------------------------------------
BATCH = 96


def train(seed, steps, check=False):
    env, buf, pi = make_loop(65, seed)
    rollout_once(env, buf, pi)
    sampler = buf.sampler(BATCH, seed=4)
    g = pi.ppo_gradient(BATCH, clip=0.2, vf_coef=0.5, ent_coef=0.01, vf_clip=0.2)
    assert pi.flat.grad is not None and g.rows_per_partial == 32 and g.partials.numel() == 3 * (pi.n_params + 8)
    opt = torch.optim.Adam([pi.flat], lr=1e-3)
    sampler.prepare()
    for m in range(steps):
        mb = sampler.gather(m, 0)
        assert g(mb) is None
        if check:
            par = policy.unpack(pi.flat.detach().cpu().numpy(), 18, 6, (64, 64))
            host = {k: getattr(mb, k).cpu().numpy() for k in PG.MB_FIELDS}
            want = PG.backward(par, host, g.ratio.cpu().numpy(), g.inv_std.cpu().numpy(), "tanh", 0.2, 0.5, 0.01, 0.2)
            assert np.array_equal(bits(pi.flat.grad.cpu().numpy()), bits(want["grad"])), m
            assert np.array_equal(bits(g.stats.cpu().numpy()), bits(want["stats"])), m
            st = g.stats_dict()
            if m == 0:                                         # unchanged parameters: z differs from eps by rounding only
                assert abs(st["approx_kl"]) < 1e-6 and st["n"] > 0 and st["clip_frac"] == 0
                assert float((g.ratio[mb.weight != 0] - 1).abs().max()) < 1e-4
        before = pi.flat.detach().clone()
        opt.step()
        assert not torch.equal(before, pi.flat.detach())
    return env, buf, pi, g


def test_end_to_end_with_adam_and_determinism():
    env, buf, pi, g = train(31, 3, check=True)
    v = torch.zeros(65, dtype=F32, device=DEV)
    pi.value(buf.obs[T], v)                                    # the next act sees the steps through the same pointer
    par = policy.unpack(pi.flat.detach().cpu().numpy(), 18, 6, (64, 64))
    want = policy.forward(par, buf.obs[T].cpu().numpy(), np.zeros((65, 6), np.float32), np.ones(6, np.float32), "tanh")
    assert np.array_equal(bits(v.cpu().numpy()), bits(want["values"]))
    old = policy.unpack(policy.init_flat(18, 6, (64, 64), 0.0, 1), 18, 6, (64, 64))
    stale = policy.forward(old, buf.obs[T].cpu().numpy(), np.zeros((65, 6), np.float32), np.ones(6, np.float32), "tanh")
    assert not np.array_equal(bits(v.cpu().numpy()), bits(stale["values"]))
    _, _, pi2, _ = train(31, 3)
    assert torch.equal(pi.flat.detach().view(torch.int32), pi2.flat.detach().view(torch.int32))       # equal seeds: identical bits
    with pytest.raises(errors.ArgsError, match="mb.obs"):
        g(type("M", (), dict(obs=None))())


# ---- 5. HIP graph ------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_of_one_epoch_equals_eager_and_allocates_nothing():
    loops = []
    for _ in range(2):
        env, buf, pi = make_loop(65, 8)
        rollout_once(env, buf, pi)
        sampler = buf.sampler(BATCH, seed=2)
        g = pi.ppo_gradient(BATCH, ent_coef=0.01)
        sampler.prepare()
        loops.append((pi, sampler, g))
    (pi, sampler, g), (tpi, tsampler, tg) = loops
    sums = [torch.zeros_like(p.flat.detach()) for p in (pi, tpi)]

    def epoch(p, s, gr, acc):
        for m in range(s.n_minibatches):
            gr(s.gather(m, 0))
            acc.add_(p.flat.grad)                              # (so that every minibatch of the epoch shows in the result)

    g(sampler.gather(0, 0))                                    # (the first launch raises the kernel's LDS limit: not under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        epoch(pi, sampler, g, sums[0])
    torch.cuda.synchronize()
    gc.collect()
    sums[0].zero_()
    m0 = torch.cuda.memory_allocated()
    for rnd in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0
        epoch(tpi, tsampler, tg, sums[1])
        torch.cuda.synchronize()
        for a, b in ((sums[0], sums[1]), (pi.flat.grad, tpi.flat.grad), (g.stats, tg.stats), (g.ratio, tg.ratio), (g.logp, tg.logp),
                     (g.values, tg.values)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), rnd
        assert bool(sums[0].any())
        for p in (pi, tpi):                                    # a step between replays is seen through the captured pointers
            with torch.no_grad():
                p.flat.add_(p.flat.grad, alpha=-0.01)
        m0 = torch.cuda.memory_allocated()
