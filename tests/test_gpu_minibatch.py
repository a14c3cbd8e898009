"""GPU tier: the minibatch sampler of the rollout buffer (``RolloutBuffer.sampler``, ``anm_minibatch_prepare`` / ``_gather``; the
specification is gym_anm_amd/minibatch.py).  Everything is integers and copies of bits, so every comparison is on bit patterns
(integer views) and there is no tolerance anywhere.
  1. ``prepare`` alone, through the C ABI, on synthetic flags over the grids of the range plan;  2. ``gather`` alone on synthetic
  buffers whose words name their own (array, slot, word);  3. end to end behind real steps;  4. HIP graph, nothing allocated;
  5. refusals of the C ABI."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

from gym_anm_amd import _lib, codegen, minibatch as mbs, rollout
from gym_anm_amd.rollout import RolloutBuffer

from test_gpu_io_f32 import device_reset
from test_gpu_io_norm import box_actions, make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
V = rollout.VALID
CODE = {F64: _lib.IO_F64, F32: _lib.IO_F32}
INT = {F32: torch.int32, F64: torch.int64}
SEED = 0x9E3779B97F4A7C15          # (both words of the key are used)
FIELDS = mbs.FIELDS
DTYPES = [(F64, F64), (F32, F32), (F32, F64)]          # io / value, the pairs of test_gpu_rollout_guard.py
DT_IDS = ["f64", "f32", "f32-v64"]


def lib():
    return _lib.load_for_topology(codegen.stock_topologies()["anm6"]).lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ibits(x):
    """a tensor or an array as integers of its own width, on the host"""
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view({1: np.uint8, 4: np.int32, 8: np.int64}[x.dtype.itemsize])


def changed(struct, **kw):
    s = _lib.Minibatch.from_buffer_copy(struct)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# ---- 1. prepare alone -----------------------------------------------------------------------------------------------------------
# one slot; a partial chunk; one slot past a chunk; one range; one slot past it; one slot past three ranges; the first size
# whose range doubles to 2048
@pytest.mark.parametrize("N", [1, 63, 65, 1024, 1025, 3073, 4096 * 1024 + 1])
def test_prepare_alone_against_the_specification(N):
    gen = torch.Generator().manual_seed(N)
    flags = torch.zeros(N, dtype=torch.uint8, device=DEV)
    index = torch.full((N,), 7, dtype=torch.int32, device=DEV)
    n_counts = mbs.range_counts(N)
    assert n_counts == -(-N // (2048 if N > 4096 * 1024 else 1024))
    counts, offsets = (torch.zeros(n_counts, dtype=torch.int32, device=DEV) for _ in range(2))
    state = torch.zeros(mbs.STATE_SIZE, dtype=torch.int64, device=DEV)
    s = _lib.Minibatch(flags=flags.data_ptr(), index=index.data_ptr(), counts=counts.data_ptr(), offsets=offsets.data_ptr(),
                       n_counts=n_counts, state=state.data_ptr(), T=1, E=N, D=1, A=1, B=1, io_dtype=_lib.IO_F32, value_dtype=_lib.IO_F32)
    last = torch.zeros(N, dtype=torch.uint8)
    last[-1] = V | rollout.TRUNCATED
    other = (torch.rand(N, generator=gen) < 0.5).to(torch.uint8) * (rollout.TERMINATED | rollout.TRUNCATED)   # bits that are not VALID
    cases = [("all", torch.full((N,), V, dtype=torch.uint8) | other), ("none", other), ("last", last),
             ("0.5", (torch.rand(N, generator=gen) < 0.5).to(torch.uint8) * V | other),
             ("0.97", (torch.rand(N, generator=gen) < 0.97).to(torch.uint8) * V)]
    for count, (name, f) in enumerate(cases, start=1):
        flags.copy_(f)
        assert lib().anm_minibatch_prepare(C.byref(s), stream()) == 0, lib().anm_last_error()
        want, n = mbs.compact(f.numpy())
        assert state.cpu().tolist() == [n, count], (N, name)
        assert np.array_equal(index.cpu().numpy(), want), (N, name)


# ---- 2. gather alone ------------------------------------------------------------------------------------------------------------
TAGS = dict(obs=1, actions=2, logp=3, values=4, returns=5, adv=6)


def named_words(shape, tag, dtype):
    """a float tensor whose every word names (array, flat slot, word): bits 0x3.. | tag << 24 | slot << 5 | word, all of them
    finite positive numbers of their format; the last axis of a rank-3 shape is the word"""
    n = int(np.prod(shape))
    it = INT[dtype]
    i = torch.arange(n, dtype=torch.int64)
    if len(shape) == 3:
        i = (i // shape[2]) * 32 + i % shape[2]
    else:
        i = i * 32
    base = 0x30000000 if dtype == F32 else 0x3000000000000000
    return (i + base + (tag << 24)).to(it).view(dtype).reshape(shape).to(DEV)


SPECIAL32 = [0x7fc12345, -0x3fffff, 0x7f800001, -0x80000000, 0x7f800000, 0x00000001]          # NaN payloads (quiet, negative, signalling), -0.0, inf, a subnormal
SPECIAL64 = [0x7ff8000000012345, -0x7ffffffffffff, 0x7ff0000000000001, -0x8000000000000000, 0x7ff0000000000000, 1]


class RawSampler:
    """the buffers of the C ABI without an environment; destinations for every minibatch of every epoch side by side, so a
    pass is launches alone and one comparison"""

    def __init__(self, T, E_, D, A, io, vdt, B, epochs=2):
        self.T, self.E, self.D, self.A, self.B, self.io, self.vdt = T, E_, D, A, B, io, vdt
        N = self.N = T * E_
        self.src = dict(obs=named_words((T + 1, E_, D), 1, io), actions=named_words((T, E_, A), 2, io), logp=named_words((T, E_), 3, vdt),
                        values=named_words((T + 1, E_), 4, vdt), returns=named_words((T, E_), 5, vdt), adv=named_words((T, E_), 6, vdt))
        for k, t in self.src.items():          # special words, spread over the slots
            flat, sp = t.view(-1).view(INT[t.dtype]), SPECIAL32 if t.dtype == F32 else SPECIAL64
            for j, b in enumerate(sp):
                flat[(TAGS[k] + 5 * j) % flat.numel()] = b
        self.flags = torch.zeros(N, dtype=torch.uint8, device=DEV)
        self.index = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        nc = mbs.range_counts(N)
        self.counts, self.offsets = (torch.zeros(nc, dtype=torch.int32, device=DEV) for _ in range(2))
        self.state = torch.zeros(mbs.STATE_SIZE, dtype=torch.int64, device=DEV)
        self.n_mb = -(-N // B)
        R = epochs * self.n_mb * B
        fill = lambda shape, dt: torch.full(shape, 9, dtype=dt, device=DEV)  # noqa: E731
        self.dst = dict(obs=fill((R, D), io), actions=fill((R, A), io), logp=fill((R,), vdt), values=fill((R,), vdt), returns=fill((R,), vdt),
                        adv=fill((R,), vdt), weight=fill((R,), vdt), slot=fill((R,), torch.int32))
        self.struct = _lib.Minibatch(
            flags=self.flags.data_ptr(), index=self.index.data_ptr(), counts=self.counts.data_ptr(), offsets=self.offsets.data_ptr(),
            n_counts=nc, state=self.state.data_ptr(), T=T, E=E_, D=D, A=A, B=B, io_dtype=CODE[io], value_dtype=CODE[vdt], seed=SEED,
            **{k: t.data_ptr() for k, t in self.src.items()}, **{"mb_" + k: t.data_ptr() for k, t in self.dst.items()})

    def run(self, flags, epochs=2):
        """prepare, then every minibatch of every epoch into its own rows of the destinations -> (n, rollout_count)"""
        L = lib()
        self.flags.copy_(flags)
        assert L.anm_minibatch_prepare(C.byref(self.struct), stream()) == 0, L.anm_last_error()
        for ep in range(epochs):
            for m in range(self.n_mb):
                row = (ep * self.n_mb + m) * self.B
                s = changed(self.struct, **{"mb_" + k: t[row:].data_ptr() for k, t in self.dst.items()})
                assert L.anm_minibatch_gather(C.byref(s), m, ep, stream()) == 0, L.anm_last_error()
        n, count = self.state.cpu().tolist()
        return n, count

    def expected(self, flags, count, epochs=2):
        """rule 3 for whole epochs at once: the rows of epoch ep are the valid slots in the order index[perm(0 .. n-1)], then padding"""
        index, n = mbs.compact(flags.numpy())
        rows = self.n_mb * self.B
        out = {k: np.zeros((epochs * rows,) + tuple(t.shape[2:]), dtype=ibits(t).dtype) for k, t in self.src.items()}
        out["weight"] = np.zeros(epochs * rows, dtype=out["values"].dtype)
        out["slot"] = np.full(epochs * rows, -1, dtype=np.int32)
        one = np.ones(1, dtype=np.float32 if self.vdt == F32 else np.float64).view(out["weight"].dtype)[0]
        for ep in range(epochs):
            s = index[mbs.perm_v(np.arange(n), n, SEED, count, ep)] if n else np.zeros(0, dtype=np.int64)
            at = slice(ep * rows, ep * rows + n)
            for k, t in self.src.items():
                out[k][at] = ibits(t).reshape((-1,) + tuple(t.shape[2:]))[s]
            out["weight"][at] = one
            out["slot"][at] = s
        return out, index, n

    def check(self, flags, where):
        n, count = self.run(flags)
        want, index, n_want = self.expected(flags, count)
        assert n == n_want, where
        for k in FIELDS:
            assert np.array_equal(ibits(self.dst[k]), want[k]), "%s: %s" % (where, k)
        return want, index, n, count


def random_valid(N, gen, p=0.8):
    return (torch.rand(N, generator=gen) < p).to(torch.uint8) * V | (torch.rand(N, generator=gen) < 0.2).to(torch.uint8) * rollout.TRUNCATED


@pytest.mark.parametrize("io,vdt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D,A", [(1, 1), (1, 6), (18, 1), (18, 6)])
@pytest.mark.parametrize("T,E_", [(1, 1), (3, 63), (3, 65), (17, 130)])
def test_gather_alone_against_the_specification(T, E_, D, A, io, vdt):
    N = T * E_
    gen = torch.Generator().manual_seed(1000 * N + 10 * D + A)
    flags = random_valid(N, gen)
    flags[:32] = V                    # the slots that hold the special words, the first and the last slot count
    flags[-1] = V
    n = int((flags & V).ne(0).sum())
    count = 0
    for B in sorted({1, 64, 65, n + 3}):
        raw = RawSampler(T, E_, D, A, io, vdt, B)
        raw.state[1] = count          # one rollout count per B: the orders differ
        want, index, n_got, count = raw.check(flags, "T=%d E=%d D=%d A=%d B=%d" % (T, E_, D, A, B))
        assert n_got == n
        rows = raw.n_mb * B
        for ep in range(2):
            slots = want["slot"][ep * rows:(ep + 1) * rows]
            assert np.array_equal(np.sort(slots[:n]), index[:n]) and bool((slots[n:] == -1).all())
        if n > 8:
            assert not np.array_equal(want["slot"][:n], want["slot"][rows:rows + n])          # two epochs, two orders
        if B == 64 and N > 64:          # the specification's own minibatch, for one of them
            one = mbs.minibatch(1, B, index, n, SEED, count, 1, **{k: t.cpu().numpy() for k, t in raw.src.items()})
            at = slice(rows + B, rows + 2 * B)
            for k in FIELDS:
                assert np.array_equal(ibits(one[k]), want[k][at]), k
    # the special words went through: a NaN keeps its payload and its sign, -0.0 its sign
    got = ibits(raw.dst["obs"]).reshape(-1)
    placed = {(TAGS["obs"] + 5 * j) % raw.src["obs"].numel(): b for j, b in enumerate(SPECIAL32 if io == F32 else SPECIAL64)}
    for at, b in placed.items():
        if at // D < N:          # (not in slot T, which no minibatch reads)
            assert (got == b).any(), hex(b)


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257])
def test_gather_at_the_minimum_width_and_the_first_widths_above_it(n):
    T, E_, B = 3, 130, 64
    gen = torch.Generator().manual_seed(n)
    flags = torch.zeros(T * E_, dtype=torch.uint8)
    flags[torch.randperm(T * E_, generator=gen)[:n]] = V
    flags |= (torch.rand(T * E_, generator=gen) < 0.3).to(torch.uint8) * rollout.TERMINATED
    raw = RawSampler(T, E_, 18, 6, F32, F32, B)
    want, index, n_got, count = raw.check(flags, "n=%d" % n)
    assert n_got == n and count == 1
    live = want["slot"][:raw.n_mb * B] >= 0
    assert int(live.sum()) == n and not live[n:].any()
    pad = ~(want["slot"] >= 0)
    for k in FIELDS[:-1]:          # padding rows: all-zero bits, weight +0.0
        assert not ibits(raw.dst[k])[pad].any(), k
    assert bool((ibits(raw.dst["slot"])[pad] == -1).all())


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------------
def rolled(E_, T, io, vdt, seed=2718):
    """an environment and its buffer after one finished rollout under a limit of two steps: reset slots among the transitions"""
    env = make_env("anm6", "thread", "uniform", E_, seed, io_dtype=io, autoreset=True, max_episode_steps=2)
    obs, _ = device_reset(env)
    buf = RolloutBuffer(env, T, gae_lambda=0.95, value_dtype=vdt)
    gen = torch.Generator(device=DEV).manual_seed(7)
    buf.begin(obs)
    for k in range(T):
        buf.actions[k].copy_(box_actions(env, gen))
        buf.values[k].copy_(buf.obs[k][:, 0] - 0.5 * buf.obs[k][:, 1])
        buf.logp[k].copy_(torch.randn(E_, generator=gen, device=DEV, dtype=F64))
        buf.add(*env.step(buf.actions[k])[:4])
    buf.values[T].copy_(buf.obs[T][:, 0] - 0.5 * buf.obs[T][:, 1])
    buf.finish(normalize=True)
    return env, buf


@functools.lru_cache(maxsize=None)
def shared_rollout():
    return rolled(200, 6, F32, None)


def sources_of(buf, advantage):
    return dict(obs=buf.obs, actions=buf.actions, logp=buf.logp, values=buf.values, returns=buf.returns,
                adv=buf.adv_norm if advantage == "norm" else buf.advantages)


@pytest.mark.parametrize("advantage", ["norm", "raw"])
def test_end_to_end_behind_real_steps(advantage):
    env, buf = shared_rollout()
    T, E_ = buf.n_steps, buf.num_envs
    valid = np.flatnonzero(buf.valid.cpu().numpy().reshape(-1))
    n = len(valid)
    B = 37 if n % 37 else 41          # a batch size that does not divide n
    sampler = buf.sampler(B, seed=5, advantage=advantage)
    assert sampler.n_minibatches == -(-T * E_ // B) and sampler.state() == dict(rollout_count=0)
    assert 0 < n < T * E_ and n % B != 0
    assert not torch.equal(buf.adv_norm, buf.advantages)
    src = {k: ibits(t).reshape((-1,) + tuple(t.shape[2:])) for k, t in sources_of(buf, advantage).items()}
    sampler.prepare()
    assert sampler.count_minibatches() == -(-n // B) and sampler.state() == dict(rollout_count=1)
    index, _ = mbs.compact(buf.flags.cpu().numpy())
    assert np.array_equal(sampler.index.cpu().numpy(), index)
    host = {k: t.cpu().numpy() for k, t in sources_of(buf, advantage).items()}
    for ep in range(2):
        slots = []
        for m in range(sampler.n_minibatches):
            mb = sampler.gather(m, ep)
            assert mb is sampler.mb and mb.obs.shape == (B, buf.obs.shape[2]) and mb.actions.shape == (B, buf.actions.shape[2])
            want = mbs.minibatch(m, B, index, n, 5, 1, ep, **host)
            s = mb.slot.cpu().numpy()
            live = s >= 0
            assert int(live.sum()) == max(0, min(B, n - m * B))
            for k in FIELDS:
                assert np.array_equal(ibits(getattr(mb, k)), ibits(want[k])), (ep, m, k)
            for k in src:                    # every gathered row is the buffer's row
                assert np.array_equal(ibits(getattr(mb, k))[live], src[k][s[live]]), (ep, m, k)
            slots.append(s[live])
        assert np.array_equal(np.sort(np.concatenate(slots)), valid)          # every valid slot exactly once
    sampler.load_state(dict(rollout_count=41))
    sampler.prepare()
    assert sampler.state() == dict(rollout_count=42)
    s42 = sampler.gather(0, 0).slot.cpu().numpy()
    assert np.array_equal(s42, index[mbs.perm_v(np.arange(B), n, 5, 42, 0)])


# ---- 4. HIP graph: prepare and two epochs, nothing allocated -------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_allocates_nothing():
    env, buf = shared_rollout()
    B, K = 300, 2
    a, b = buf.sampler(B, seed=9), buf.sampler(B, seed=9)
    n_mb = a.n_minibatches
    assert n_mb == 4

    def staging():
        return [[{k: torch.zeros_like(getattr(a.mb, k)) for k in FIELDS} for _ in range(n_mb)] for _ in range(K)]

    def epochs(s, out):
        s.prepare()
        for ep in range(K):
            for m in range(n_mb):
                mb = s.gather(m, ep)
                for k in FIELDS:
                    out[ep][m][k].copy_(getattr(mb, k))

    sa, sb = staging(), staging()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        epochs(a, sa)
    torch.cuda.synchronize()
    assert a.state() == dict(rollout_count=0)          # capture does not execute
    gc.collect()
    m0 = torch.cuda.memory_allocated()
    firsts = []
    for rnd in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0
        epochs(b, sb)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0          # eager prepare / gather allocate nothing either
        assert a.state() == b.state() == dict(rollout_count=rnd + 1)
        for ep in range(K):
            for m in range(n_mb):
                for k in FIELDS:
                    assert np.array_equal(ibits(sa[ep][m][k]), ibits(sb[ep][m][k])), (rnd, ep, m, k)
        firsts.append(sa[0][0]["slot"].cpu().numpy().copy())
        assert not np.array_equal(firsts[-1], sa[1][0]["slot"].cpu().numpy())          # the epochs differ
        assert bool((sa[0][0]["weight"] == 1).all()) and not bool(sa[0][n_mb - 1]["weight"].all())
    assert not np.array_equal(firsts[0], firsts[1])          # and so do the rollout counts


# ---- 5. refusals of the C ABI ---------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_carry_a_message_and_launch_nothing():
    L = lib()
    err = lambda: L.anm_last_error()  # noqa: E731
    raw = RawSampler(3, 1025, 2, 3, F32, F32, 64, epochs=1)
    raw.flags.fill_(V)
    prepare = lambda s: L.anm_minibatch_prepare(C.byref(s) if s is not None else None, None)  # noqa: E731
    gather = lambda s, m=0, ep=0: L.anm_minibatch_gather(C.byref(s) if s is not None else None, m, ep, None)  # noqa: E731
    both = (prepare, gather)
    for call in both:
        assert call(None) != 0 and b"null anm_minibatch" in err()
        for kw, msg in ((dict(T=0), b"at least 1"), (dict(E=0), b"at least 1"), (dict(D=0), b"at least 1"), (dict(A=0), b"at least 1"),
                        (dict(B=0), b"at least 1"), (dict(B=-5), b"at least 1"), (dict(T=2**17), b"67 108 864"), (dict(io_dtype=2), b"dtype"),
                        (dict(value_dtype=-1), b"dtype"), (dict(n_counts=3), b"counts buffer is too short"),       # 3075 slots: 4 ranges
                        (dict(counts=None), b"counts buffer is too short"), (dict(offsets=None), b"counts buffer is too short"),
                        (dict(index=None), b"must be set"), (dict(state=None), b"must be set")):
            assert call(changed(raw.struct, **kw)) != 0 and msg in err(), kw
    assert prepare(changed(raw.struct, flags=None)) != 0 and b"flags must be set" in err()
    for k in ("obs", "actions", "logp", "values", "returns", "adv"):
        assert gather(changed(raw.struct, **{k: None})) != 0 and b"sources" in err(), k
    for k in FIELDS:
        assert gather(changed(raw.struct, **{"mb_" + k: None})) != 0 and b"destinations" in err(), k
    for m in (-1, raw.n_mb, 2**40):          # m B >= T E
        assert gather(raw.struct, m=m) != 0 and b"m is outside" in err()
    for ep in (-1, 2**32, 2**40):
        assert gather(raw.struct, ep=ep) != 0 and b"ep is outside" in err()
    torch.cuda.synchronize()
    assert not bool(raw.state.any()) and bool((raw.index == -1).all()) and not bool(raw.counts.any())          # nothing was launched
    assert all(bool((ibits(t) == ibits(torch.full((1,), 9, dtype=t.dtype))[0]).all()) for t in raw.dst.values())
    assert prepare(changed(raw.struct, n_counts=4)) == 0 and gather(raw.struct, m=raw.n_mb - 1, ep=2**32 - 1) == 0
    torch.cuda.synchronize()
    assert raw.state.cpu().tolist() == [3075, 1]
    assert int((raw.dst["slot"][:64] >= 0).sum()) == 3075 - (raw.n_mb - 1) * 64
