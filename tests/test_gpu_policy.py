"""GPU tier: the Gaussian MLP policy (``gym_anm_amd.policy.GaussianMLPPolicy``, ``anm_policy_act``; the specification is
gym_anm_amd/policy.py).  The two transcendental stages -- the noise and ``std`` -- are held to mpmath within 1 float32 ulp, no
exclusions; with the device's ``eps`` and ``std`` read back, ``actions``, ``values`` and ``logp`` equal ``policy.forward`` bit for bit
(integer views, NaNs canonical).
  1. through the C ABI on synthetic tensors, over the shapes;  2. the -0.0 column, a NaN row, an Inf element;  3. the class: global
  indices, refusals;  4. end to end behind real steps, in the rollout buffer;  5. HIP graph;  6. ``evaluate``."""
import ctypes as C
import gc
import math

import mpmath as mp
import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, errors, policy
from gym_anm_amd.policy import GaussianMLPPolicy
from gym_anm_amd.rollout import RolloutBuffer

from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import make_env, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
CODE = {F64: _lib.IO_F64, F32: _lib.IO_F32}
NP = {F64: np.float64, F32: np.float32}
SENTINEL = 7.0
PAD = 3          # rows behind E in every output: the kernel leaves them alone


def lib():
    return _lib.load_for_topology(codegen.stock_topologies()["anm6"]).lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def canon(x):
    x = np.array(x, copy=True)
    if x.dtype.kind == "f":
        x[np.isnan(x)] = np.nan
    return x


def tsame(x, y):
    """a device tensor against an array, bit for bit, NaNs canonical on both sides"""
    return same(canon(x.cpu().numpy()), canon(np.asarray(y)))


def ulp32(exact):
    return np.spacing(np.abs(np.asarray(exact, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def exact_noise(seed, env_offset, rc, ts, A):
    """the exact Box-Muller image of the uniforms of rule 5, as float64 of a 100-bit evaluation: ``[E, A]``"""
    mp.mp.prec = 100
    u1, u2 = policy.uniforms(seed, env_offset, rc, ts, A)
    out = np.empty((u1.shape[0], 2 * u1.shape[1]))
    for e in range(u1.shape[0]):
        for p in range(u1.shape[1]):
            r = mp.sqrt(-2 * mp.log(mp.mpf(float(u1[e, p]))))
            t = 2 * mp.pi * mp.mpf(float(u2[e, p]))
            out[e, 2 * p], out[e, 2 * p + 1] = float(r * mp.cos(t)), float(r * mp.sin(t))
    return out[:, :A]


def assert_noise(noise, seed, env_offset, rc, ts, A, where):
    exact = exact_noise(seed, env_offset, rc, ts, A)
    err = np.abs(noise.astype(np.float64) - exact) / ulp32(exact)
    assert err.max() <= 1.0, "%s: noise %.2f float32 ulp off the exact Box-Muller image" % (where, err.max())


def assert_std(std, log_std, where):
    mp.mp.prec = 100
    exact = np.array([float(mp.exp(mp.mpf(float(x)))) for x in log_std])
    err = np.abs(std.astype(np.float64) - exact) / ulp32(exact)
    assert err.max() <= 1.0, "%s: std %.2f float32 ulp off exp(log_std)" % (where, err.max())


class Raw:
    """the C ABI without an environment: parameters at scale 1 (the tanh spans its range), counters of the test's own"""

    def __init__(self, E_, D, A, hidden, activation, io, vdt, seed=5, env_offset=0):
        g = torch.Generator().manual_seed(1000 * D + 10 * A + len(hidden))
        self.E, self.D, self.A, self.hidden, self.activation, self.io, self.vdt = E_, D, A, tuple(hidden), activation, io, vdt
        self.seed, self.env_offset = seed, env_offset
        self.P = policy.layout(D, A, hidden)[1]
        self.flat = torch.randn(self.P, generator=g, dtype=F32).to(DEV)
        self.flat[-A:] = torch.linspace(-1.5, 0.5, A)
        self.obs = torch.randn((E_, D), generator=g, dtype=F64).to(io).to(DEV)
        self.rc = torch.randint(1, 6, (E_,), generator=g, dtype=torch.int32).to(DEV)
        self.ts = torch.randint(0, 100, (E_,), generator=g, dtype=torch.int32).to(DEV)
        full = lambda shape, dt: torch.full(shape, SENTINEL, dtype=dt, device=DEV)  # noqa: E731
        self.actions, self.values, self.logp = full((E_ + PAD, A), io), full((E_ + PAD,), vdt), full((E_ + PAD,), vdt)
        self.noise, self.std = full((E_ + PAD, A), F32), full((A + PAD,), F32)
        h3 = list(hidden) + [0] * (3 - len(hidden))
        self.struct = _lib.Policy(
            params=self.flat.data_ptr(), n_params=self.P, D=D, A=A, n_hidden=len(hidden), hidden=(C.c_int32 * 3)(*h3),
            activation=policy.ACTIVATIONS[activation], deterministic=0, seed=seed, env_offset=env_offset,
            reset_count=self.rc.data_ptr(), timestep=self.ts.data_ptr(), noise=self.noise.data_ptr(), std=self.std.data_ptr(), E=E_,
            io_dtype=CODE[io], value_dtype=CODE[vdt])

    def act(self, deterministic=False):
        self.struct.deterministic = int(deterministic)
        rc = lib().anm_policy_act(C.byref(self.struct), self.obs.data_ptr(), self.actions.data_ptr(), self.values.data_ptr(),
                                  self.logp.data_ptr(), stream())
        assert rc == 0, lib().anm_last_error()

    def value(self):
        rc = lib().anm_policy_act(C.byref(self.struct), self.obs.data_ptr(), None, self.values.data_ptr(), None, stream())
        assert rc == 0, lib().anm_last_error()

    def params(self):
        return policy.unpack(self.flat.cpu().numpy(), self.D, self.A, self.hidden)

    def spec(self, eps, std):
        return policy.forward(self.params(), self.obs.cpu().numpy(), eps, std, self.activation, value_dtype=NP[self.vdt])

    def check(self, where, exact_stages=True):
        """everything one ``act`` wrote, against the specification; -> (eps, std, spec)"""
        E_, A = self.E, self.A
        eps, std = self.noise[:E_].cpu().numpy(), self.std[:A].cpu().numpy()
        if exact_stages:
            assert_noise(eps, self.seed, self.env_offset, self.rc.cpu().numpy(), self.ts.cpu().numpy(), A, where)
            assert_std(std, self.flat[-A:].cpu().numpy(), where)
        want = self.spec(eps, std)
        assert tsame(self.actions[:E_], want["actions"]), where + ": actions"
        assert tsame(self.values[:E_], want["values"]), where + ": values"
        assert tsame(self.logp[:E_], want["logp"]), where + ": logp"
        for t in (self.actions[E_:], self.values[E_:], self.logp[E_:], self.noise[E_:], self.std[A:]):
            assert bool((t == SENTINEL).all()), where + ": written past the rows"
        return eps, std, want


# ---- 1. the shapes, through the C ABI -----------------------------------------------------------------------------------------------------
SIZES = [1, 31, 33, 130]          # a partial tile; one row short of and one row past a wavefront's 32; a second workgroup of 128
SHAPES = [(3, 1), (18, 6), (17, 5)]
HIDDEN = [(32,), (64, 64), (32, 96, 32)]
DTYPES = [(F64, F64), (F32, F32), (F32, F64)]


@pytest.mark.parametrize("io,vdt", DTYPES, ids=["f64-v64", "f32-v32", "f32-v64"])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("hidden", HIDDEN, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("D,A", SHAPES)
def test_act_against_the_specification(D, A, hidden, activation, io, vdt):
    for E_ in SIZES:
        raw = Raw(E_, D, A, hidden, activation, io, vdt)
        where = "E=%d" % E_
        raw.act()
        eps, std, want = raw.check(where)
        assert E_ < 100 or np.abs(want["mean"]).max() > 0.5                 # weights at scale 1: the activations span their range
        values = raw.values.clone()
        raw.values.fill_(SENTINEL)
        noise = raw.noise.clone()
        raw.value()                                            # the critic alone: the same bits, nothing else touched
        assert torch.equal(raw.values.view(torch.uint8), values.view(torch.uint8)), where + ": value()"
        assert torch.equal(raw.noise, noise)
        raw.act(deterministic=True)
        assert not bool(raw.noise[:E_].any()) and not bool(torch.signbit(raw.noise[:E_]).any())
        mean = want["mean"].astype(NP[io])
        assert tsame(raw.actions[:E_], mean), where + ": deterministic actions are the mean"
        raw.check(where + " deterministic", exact_stages=False)


# ---- 2. signed zeros, NaN and Inf ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_negative_zero_survives_an_odd_k(activation):
    """D = 3 is odd: the critic's first layer all +0 with -0.0 biases gives -0.0 activations on a row of negative observations
    (every product is -0), and a head of positive weights with a -0.0 bias keeps the value at -0.0.  A first layer padded to an
    even k by +0 * +0 would give +0.0.  One positive observation is enough for +0.0 -- as the specification has it."""
    raw = Raw(33, 3, 1, (32,), activation, F32, F32)
    entries, _ = policy.layout(3, 1, (32,))
    at = {(n, i, k): (o, s) for n, i, k, o, s in entries}
    flat = raw.flat.cpu().numpy()
    o, s = at[("critic", 0, "weight")]
    flat[o:o + 96] = 0.0
    o, s = at[("critic", 0, "bias")]
    flat[o:o + 32] = -0.0
    o, s = at[("critic", 1, "weight")]
    flat[o:o + 32] = np.abs(flat[o:o + 32]) + 0.5
    o, s = at[("critic", 1, "bias")]
    flat[o] = -0.0
    raw.flat.copy_(torch.from_numpy(flat))
    obs = -(raw.obs.abs() + 0.25)
    obs[1, 2] = 0.75
    obs[2] = 0.0
    raw.obs.copy_(obs)
    raw.act()
    _, _, want = raw.check("zero column")
    v = raw.values[:33].cpu().numpy().view(np.int32)
    assert v[0] == np.int32(-2 ** 31) and v[1] == 0 and v[2] == 0 and (np.delete(v, [1, 2]) == np.int32(-2 ** 31)).all()


@pytest.mark.parametrize("io,vdt", DTYPES, ids=["f64-v64", "f32-v32", "f32-v64"])
def test_nan_row_and_inf_element_stay_in_their_rows(io, vdt):
    raw = Raw(130, 18, 6, (64, 64), "tanh", io, vdt)
    clean = Raw(130, 18, 6, (64, 64), "tanh", io, vdt)
    raw.obs[7] = float("nan")
    raw.obs[40, 3] = float("inf")
    raw.obs[129, 17] = float("-inf")
    raw.act()
    clean.act()
    _, _, want = raw.check("NaN row")
    a, v, lp = raw.actions[:130].cpu().numpy(), raw.values[:130].cpu().numpy(), raw.logp[:130].cpu().numpy()
    assert np.isnan(a[7]).all() and np.isnan(v[7]) and np.isfinite(lp).all()
    ai = a[7].view(np.int32 if io == F32 else np.int64)
    assert (ai == (0x7fc00000 if io == F32 else 0x7ff8000000000000)).all()          # the canonical quiet NaN
    assert np.isfinite(a[[40, 129]]).all() and np.isfinite(v[[40, 129]]).all()       # the tanh saturates an infinite pre-activation
    rest = np.delete(np.arange(130), [7, 40, 129])
    assert same(a[rest], clean.actions[:130].cpu().numpy()[rest]) and same(v[rest], clean.values[:130].cpu().numpy()[rest])


# ---- 3. the class ---------------------------------------------------------------------------------------------------------------------------
def anm6_env(E_, seed, io=F32, **kw):
    return make_env("anm6", "thread", "uniform", E_, seed, io_dtype=io, **kw)


def outputs(pi, vdt=None):
    E_, A = pi.num_envs, pi.action_dim
    vdt = pi.io_dtype if vdt is None else vdt
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731
    return z((E_, A), pi.io_dtype), z((E_,), vdt), z((E_,), vdt)


def spec_of(pi, obs, eps, vdt):
    par = policy.unpack(pi.flat.detach().cpu().numpy(), pi.obs_dim, pi.action_dim, pi.hidden)
    return policy.forward(par, obs.cpu().numpy(), eps.cpu().numpy(), pi.std.cpu().numpy(), pi.activation, value_dtype=NP[vdt])


@pytest.mark.parametrize("io,vdt", DTYPES, ids=["f64-v64", "f32-v32", "f32-v64"])
def test_class_views_global_indices_and_the_optimiser(io, vdt):
    E_ = 33
    env = anm6_env(E_, 21, io, env_offset=1000)
    obs, _ = device_reset(env)
    pi = GaussianMLPPolicy(env, hidden=(64, 64), log_std_init=-0.5, seed=9, init_seed=4)
    assert isinstance(pi, torch.nn.Module) and [n for n, _ in pi.named_parameters()] == ["flat"] and pi.flat.dtype == F32
    assert pi.flat.numel() == 11213 and tuple(pi.actor[0].weight.shape) == (18, 64) and tuple(pi.critic[2].weight.shape) == (64, 1)
    assert pi.actor[1].bias.data_ptr() == pi.flat.data_ptr() + 4 * (18 * 64 + 64 + 64 * 64) and pi.log_std.numel() == 6
    assert same(pi.flat.detach().cpu().numpy(), policy.init_flat(18, 6, (64, 64), -0.5, 4))
    a, v, lp = outputs(pi, vdt)
    pi.act(obs, a, v, lp)
    rc, ts = env._reset_count.cpu().numpy(), env.timestep.cpu().numpy()
    eps = pi.noise.cpu().numpy()
    assert_noise(eps, 9, 1000, rc, ts, 6, "env_offset=1000")
    assert not np.array_equal(eps, policy.noise(9, 0, rc, ts, 6))
    assert_std(pi.std.cpu().numpy(), np.full(6, -0.5, dtype=np.float32), "std")
    want = spec_of(pi, obs, pi.noise, vdt)
    assert tsame(a, want["actions"]) and tsame(v, want["values"]) and tsame(lp, want["logp"])
    a2, v2, lp2 = outputs(pi, vdt)
    pi.act(obs, a2, v2, lp2)                                   # an unchanged environment row repeats the draw (rule 8)
    assert torch.equal(a, a2) and torch.equal(lp, lp2)
    opt = torch.optim.SGD([pi.flat], lr=0.05)
    pi.flat.grad = torch.ones_like(pi.flat)
    ptr = pi.flat.data_ptr()
    opt.step()
    assert pi.flat.data_ptr() == ptr
    pi.act(obs, a2, v2, lp2)                                   # the step is seen through the same pointer
    want2 = spec_of(pi, obs, pi.noise, vdt)
    assert tsame(a2, want2["actions"]) and tsame(v2, want2["values"]) and not torch.equal(v, v2)
    assert tsame(pi.actor[0].weight, pi.flat.detach().cpu().numpy()[:18 * 64].reshape(18, 64))     # the views follow
    pi.value(obs, v)
    assert torch.equal(v, v2)
    with pytest.raises(errors.ArgsError, match="contiguous"):
        pi.act(obs, a2.double() if io == F32 else a2.float(), v2, lp2)
    with pytest.raises(errors.ArgsError, match="contiguous"):
        pi.act(obs[:, :17], a2, v2, lp2)
    with pytest.raises(errors.ArgsError, match="logp"):
        pi.act(obs, a2, v2, lp2.to(F32 if vdt == F64 else F64))
    with pytest.raises(errors.ArgsError, match="values"):
        pi.value(obs, v2[:5])


def test_c_abi_refusals_carry_a_message_and_launch_nothing():
    L = lib()
    err = lambda: L.anm_last_error()  # noqa: E731
    raw = Raw(33, 18, 6, (64, 64), "tanh", F32, F32)

    def call(ref, obs=raw.obs, a=raw.actions, v=raw.values, lp=raw.logp):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return L.anm_policy_act(ref, p(obs), p(a), p(v), p(lp), None)

    def changed(**kw):
        s = _lib.Policy.from_buffer_copy(raw.struct)
        for k, val in kw.items():
            setattr(s, k, val)
        return C.byref(s)

    ref = C.byref(raw.struct)
    assert call(None) != 0 and b"null anm_policy" in err()
    assert call(ref, obs=None) != 0 and b"must be set" in err()
    assert call(ref, v=None) != 0 and b"must be set" in err()
    assert call(ref, a=None) != 0 and b"both" in err()
    assert call(ref, lp=None) != 0 and b"both" in err()
    for kw, msg in ((dict(D=0), b"D is"), (dict(D=257), b"D is"), (dict(A=0), b"A is"), (dict(A=65), b"A is"), (dict(n_hidden=0), b"n_hidden"),
                    (dict(n_hidden=4), b"n_hidden"), (dict(hidden=(C.c_int32 * 3)(64, 48, 0)), b"multiple of 32"),
                    (dict(hidden=(C.c_int32 * 3)(288, 64, 0)), b"multiple of 32"), (dict(activation=2), b"activation"),
                    (dict(io_dtype=2), b"dtype"), (dict(value_dtype=-1), b"dtype"), (dict(E=0), b"E is"), (dict(n_params=11212), b"layout"),
                    (dict(params=None), b"must be set"), (dict(noise=None), b"noise and std"), (dict(std=None), b"noise and std"),
                    (dict(timestep=None), b"reset_count and timestep"), (dict(reset_count=None), b"reset_count and timestep")):
        assert call(changed(**kw)) != 0 and msg in err(), kw
    big = policy.layout(18, 6, (128, 128))[1]
    assert call(changed(hidden=(C.c_int32 * 3)(128, 128, 0), n_params=big)) != 0 and b"LDS plan" in err()
    torch.cuda.synchronize()
    for t in (raw.actions, raw.values, raw.logp, raw.noise, raw.std):
        assert bool((t == SENTINEL).all())                     # nothing was launched
    assert call(changed(deterministic=1, timestep=None, reset_count=None)) == 0        # a deterministic act reads no counter
    torch.cuda.synchronize()
    assert not bool(raw.noise[:33].any())


# ---- 4. end to end, in the rollout buffer ----------------------------------------------------------------------------------------------------
T = 5
LIMIT = dict(autoreset=True, max_episode_steps=2, action_map="unit")


def rollout_once(env, buf, pi, noises=None):
    buf.begin()
    for k in range(T):
        pi.act(buf.obs[k], buf.actions[k], buf.values[k], buf.logp[k])
        if noises is not None:
            noises.append((pi.noise.clone(), env.timestep.clone(), env._reset_count.clone()))
        buf.add(*env.step(buf.actions[k])[:4])
    pi.value(buf.obs[T], buf.values[T])
    buf.finish(normalize=True)


def make_loop(E_, seed, vdt=None):
    env = anm6_env(E_, seed, F32, **LIMIT)
    obs, _ = device_reset(env)
    buf = RolloutBuffer(env, T, gae_lambda=0.95, value_dtype=vdt)
    buf.obs[T].copy_(obs)                                      # begin() continues from obs[T]
    pi = GaussianMLPPolicy(env, hidden=(64, 64), seed=3, init_seed=1)
    return env, buf, pi


@pytest.fixture(scope="module")
def finished_rollout():
    env, buf, pi = make_loop(65, 31)
    noises = []
    rollout_once(env, buf, pi, noises)
    torch.cuda.synchronize()
    return env, buf, pi, noises


def test_end_to_end_every_slot_equals_the_specification(finished_rollout):
    env, buf, pi, noises = finished_rollout
    for k in range(T):
        eps, ts, rc = noises[k]
        assert_noise(eps.cpu().numpy(), 3, 0, rc.cpu().numpy(), ts.cpu().numpy(), 6, "slot %d" % k)
        want = spec_of(pi, buf.obs[k], eps, F32)
        assert tsame(buf.actions[k], want["actions"]) and tsame(buf.values[k], want["values"]) and tsame(buf.logp[k], want["logp"]), k
        if k:
            assert bool((eps != noises[k - 1][0]).all(dim=1).all())           # fresh noise at every slot ...
    want = spec_of(pi, buf.obs[T], noises[-1][0], F32)
    assert tsame(buf.values[T], want["values"])
    ts = torch.stack([n[1] for n in noises])
    again = (ts[1:] == 0)                                      # ... and across an in-kernel autoreset: step index 0 again, another reset count
    assert bool(again.any())
    k, e = (int(x[0]) for x in again.nonzero(as_tuple=True))
    assert int(noises[k + 1][1][e]) == int(noises[0][1][e]) == 0 and int(noises[k + 1][2][e]) > int(noises[0][2][e])
    assert bool((noises[k + 1][0][e] != noises[0][0][e]).all())
    assert buf.stats()["n_valid"] > 0 and bool(torch.isfinite(buf.adv_norm).all())


# ---- 5. HIP graph -----------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_draws_fresh_noise_equals_eager_and_allocates_nothing():
    (env, buf, pi), (twin, tbuf, tpi) = make_loop(65, 8), make_loop(65, 8)
    a, v, lp = outputs(pi)
    pi.act(buf.obs[T], a, v, lp)                               # (the first launch raises the kernel's LDS limit: not under capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rollout_once(env, buf, pi)
    torch.cuda.synchronize()
    assert not bool(env.timestep.any()) and not bool(buf.flags.any())          # capture does not execute
    gc.collect()
    m0 = torch.cuda.memory_allocated()
    names = ("obs", "actions", "rewards", "values", "logp", "flags", "advantages", "returns", "adv_norm")
    opt, topt = torch.optim.SGD([pi.flat], lr=0.01), torch.optim.SGD([tpi.flat], lr=0.01)
    before = None
    for rnd in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0
        rollout_once(twin, tbuf, tpi)
        for n in names:
            assert tsame(getattr(buf, n), getattr(tbuf, n).cpu().numpy()), "replay %d: %s" % (rnd, n)
        assert torch.equal(pi.noise, tpi.noise) and torch.equal(env.timestep, twin.timestep)
        if rnd == 1:
            assert not torch.equal(buf.actions, before[0]) and not torch.equal(buf.logp, before[1])     # replay two is not replay one
            for o, p in ((opt, pi), (topt, tpi)):              # an optimiser step between replays is seen by the next one
                p.flat.grad = torch.full_like(p.flat, 0.5)
                o.step()
        if rnd == 2:
            want = spec_of(pi, buf.obs[T], pi.noise, F32)      # the stepped parameters, through the captured pointer
            assert tsame(buf.values[T], want["values"])
            old = policy.unpack(policy.init_flat(18, 6, (64, 64), 0.0, 1), 18, 6, (64, 64))
            stale = policy.forward(old, buf.obs[T].cpu().numpy(), pi.noise.cpu().numpy(), pi.std.cpu().numpy(), "tanh")
            assert not tsame(buf.values[T], stale["values"])
        before = (buf.actions.clone(), buf.logp.clone())
        m0 = torch.cuda.memory_allocated()


# ---- 6. evaluate --------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_is_consistent_with_act(finished_rollout, capsys):
    """The PPO ratio at epoch 0: the kernel's logp and torch's float32 ``evaluate`` on the stored (obs, actions), each against a
    float64 evaluation of the same network.  Both are float32 evaluations that differ in summation order and, by a few ulp, in
    the tanh: the kernel's largest error is at most 4 x torch's own."""
    env, buf, pi, _ = finished_rollout
    obs, act = buf.obs[:T].reshape(-1, 18), buf.actions.reshape(-1, 6)
    logp32, entropy, values32 = pi.evaluate(obs, act)
    assert logp32.requires_grad and values32.requires_grad and logp32.dtype == F32
    par = policy.unpack(pi.flat.detach().cpu().numpy(), 18, 6, (64, 64))

    def net64(layers, x):
        for i, (W, b) in enumerate(layers):
            x = x @ torch.from_numpy(W).double().to(DEV) + torch.from_numpy(b).double().to(DEV)
            if i + 1 < len(layers):
                x = torch.tanh(x)
        return x

    ls = torch.from_numpy(par["log_std"]).double().to(DEV)
    mean = net64(par["actor"], obs.double())
    z = (act.double() - mean) * torch.exp(-ls)
    ref = (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(dim=1)
    e_kernel = float((buf.logp.reshape(-1).double() - ref).abs().max())
    e_torch = float((logp32.detach().double() - ref).abs().max())
    with capsys.disabled():
        print("\n  logp against float64: kernel %.3g, torch float32 evaluate %.3g (%d rows)" % (e_kernel, e_torch, ref.numel()))
    assert e_kernel <= 4 * e_torch
    v64 = net64(par["critic"], obs.double())[:, 0]
    assert float((values32.detach().double() - v64).abs().max()) < 1e-5 and float((buf.values[:T].reshape(-1).double() - v64).abs().max()) < 1e-5
    want = float(ls.sum()) + 6 * (0.5 + 0.5 * math.log(2 * math.pi))
    assert entropy.shape == (obs.shape[0],) and float((entropy.detach().double() - want).abs().max()) < 1e-6
    logp32.sum().backward()
    assert pi.flat.grad is not None and bool(torch.isfinite(pi.flat.grad).all()) and bool(pi.flat.grad.any())
