"""Minibatch sampler of the device rollout buffer: compact the valid slots, shuffle them, gather rows of fixed shape
(``MinibatchSampler``, from ``RolloutBuffer.sampler``; ``anm_minibatch_prepare`` / ``_gather`` in the C ABI): the specification
the kernels of csrc/anm_minibatch.hpp follow.  Like ``rollout.py`` and ``rng.py`` this text is normative: the kernels are tested
against it bit for bit, and since everything here is integers and copies of bits there is no tolerance at all.

A PPO epoch draws its minibatches from the valid slots of the buffer only (``rollout.py`` rule 2).  In torch that is
``valid.nonzero()`` -- a result of dynamic shape, hence a host synchronisation -- a ``randperm`` and six ``index_select`` per
minibatch.  Here the shapes are fixed, nothing allocates or synchronises, and the same key gives the same order on every run.

Notation: ``N = T * E`` slots, the flat slot index ``s = k * E + e``, ``B = batch_size``.

1. Compaction.  ``n`` is the number of slots with ``flags & VALID``; ``index[j]``, ``j < n``, is the flat index of the ``j``-th
   valid slot in ascending flat order and ``index[j] = -1`` for ``n <= j < N``.  ``index`` is int32 (``N <= 67 108 864``).  Every
   ``prepare`` adds 1 to the device-resident ``rollout_count``, an int64 that starts at 0: the first prepared rollout has
   count 1.  (:func:`compact`)
2. The permutation of ``[0, n)`` of epoch ``ep >= 0``: a 4-round alternating Feistel network with cycle walking.
   ``b = max(8, bit_length(n - 1))``, ``a = b // 2``, ``c = b - a``; ``x = hi << a | lo`` with ``lo`` of ``a`` and ``hi`` of ``c`` bits.
   Round ``r = 0, 1, 2, 3``: even ``r``: ``hi ^= F(r, lo) & (2^c - 1)``; odd ``r``: ``lo ^= F(r, hi) & (2^a - 1)``, with
   ``F(r, v) = rng.philox4x32(seed, v | ep << 32, rollout_count, MB_TAG + r)[0]`` and ``MB_TAG = 0x4D425348``.  The four rounds
   are repeated on the result while it is ``>= n``.  Every round is a bijection of ``[0, 2^b)``, so the walk is a bijection of
   ``[0, n)``; it ends after at most ``2^b - n + 1`` passes, and the kernel's loop carries that bound as its trip limit.  A
   width below 8 shuffles visibly unevenly (a minimum of 2 gives a chi-square of 146 on 4 degrees of freedom for the images
   of ``n = 5``), which is why the minimum is 8.  (:func:`perm`, :func:`perm_v`)
3. Minibatch ``m``, rows ``i = 0 .. B-1`` at position ``p = m * B + i``.  If ``p < n`` the row is slot ``s = index[perm(p)]`` and
   carries ``obs[k, e, :]``, ``actions[k, e, :]``, ``logp[k, e]``, ``values[k, e]``, ``returns[k, e]``, the advantage
   (``adv_norm[k, e]`` for ``advantage="norm"``, ``advantages[k, e]`` for ``"raw"``), ``weight = 1`` and ``slot = s``: copies of
   bits, no conversion and no NaN canonicalisation.  Otherwise it is a padding row: every word 0, ``weight = 0``,
   ``slot = -1``.  With ``n = 0`` every row is padding and rule 2 is never evaluated.  ``weight`` has the value dtype,
   ``slot`` is int32.  The minibatches ``0 .. ceil(n / B) - 1`` of one ``(rollout_count, ep)`` hold every valid slot exactly
   once.  (:func:`minibatch`)
4. Not served: what rule 5 of ``rollout.py`` excludes; per-minibatch advantage normalisation; sampling with replacement;
   recurrent (sequence) minibatches; a cross-rank shuffle; ``exo_forecast`` rows.  ``prepare()`` before ``finish()`` is the
   caller's error: it reads whatever the buffers hold.
"""

from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import errors as E
from . import rng
from .rollout import VALID, slab_range

MB_TAG = 0x4D425348
MIN_WIDTH, ROUNDS = 8, 4
STATE_SIZE = 2          # the device state block: int64 n_valid, rollout_count
FIELDS = ("obs", "actions", "logp", "values", "returns", "adv", "weight", "slot")


# ---- the specification ---------------------------------------------------------------------------------------------------------
def compact(flags):
    """Rule 1: ``(index, n)`` of a flags array (any shape; the flat order is C order)."""
    valid = (np.asarray(flags).reshape(-1) & VALID) != 0
    index = np.full(valid.shape[0], -1, dtype=np.int32)
    rank = np.cumsum(valid, dtype=np.int64) - 1          # of a valid slot: the valid slots before it
    index[rank[valid]] = np.arange(valid.shape[0], dtype=np.int32)[valid]
    return index, int(valid.sum())


def width(n):
    """Rule 2: ``(b, a, c)`` of ``n >= 1``."""
    b = max(MIN_WIDTH, (int(n) - 1).bit_length())
    return b, b // 2, b - b // 2


def walk_limit(n):
    """Rule 2: the passes the walk can take at most."""
    return (1 << width(n)[0]) - int(n) + 1


def _pass(x, a, c, seed, rollout_count, ep):
    lo, hi = x & ((1 << a) - 1), x >> a
    for r in range(ROUNDS):
        if r % 2 == 0:
            hi ^= rng.philox4x32(seed, lo | ep << 32, rollout_count, MB_TAG + r)[0] & ((1 << c) - 1)
        else:
            lo ^= rng.philox4x32(seed, hi | ep << 32, rollout_count, MB_TAG + r)[0] & ((1 << a) - 1)
    return hi << a | lo


def perm_walk(p, n, seed, rollout_count, ep):
    """Rule 2: ``(image of p, passes taken)``."""
    p, n, ep = int(p), int(n), int(ep)
    if not 0 <= p < n:
        raise E.ArgsError("perm: p is %d but should be in [0, %d)" % (p, n))
    _, a, c = width(n)
    x, passes = p, 0
    while True:
        x = _pass(x, a, c, int(seed), int(rollout_count), ep)
        passes += 1
        if x < n:
            return x, passes


def perm(p, n, seed, rollout_count, ep):
    """Rule 2: the image of ``p`` under the permutation of ``[0, n)`` of ``(seed, rollout_count, ep)``."""
    return perm_walk(p, n, seed, rollout_count, ep)[0]


def perm_v(p, n, seed, rollout_count, ep):
    """``perm`` over arrays of positions, rollout counts and epochs (broadcast; built on ``rng.philox4x32_v``): int64."""
    n = int(n)
    p, rollout_count, ep = np.broadcast_arrays(np.asarray(p, dtype=np.int64), np.asarray(rollout_count, dtype=np.int64),
                                               np.asarray(ep, dtype=np.int64))
    if p.size == 0:
        return p.copy()
    if int(p.min()) < 0 or int(p.max()) >= n:
        raise E.ArgsError("perm_v: a position is outside [0, %d)" % n)
    _, a, c = width(n)
    am, cm, sa = np.uint64((1 << a) - 1), np.uint64((1 << c) - 1), np.uint64(a)
    sd = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    x = p.astype(np.uint64)
    rc, e32 = (rollout_count & rng.MASK).astype(np.uint64), ep.astype(np.uint64) << np.uint64(32)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v, rcv, ev = x[todo], rc[todo], e32[todo]
        lo, hi = v & am, v >> sa
        for r in range(ROUNDS):
            if r % 2 == 0:
                hi = hi ^ (rng.philox4x32_v(sd, lo | ev, rcv, np.uint64(MB_TAG + r))[..., 0] & cm)
            else:
                lo = lo ^ (rng.philox4x32_v(sd, hi | ev, rcv, np.uint64(MB_TAG + r))[..., 0] & am)
        x[todo] = (hi << sa) | lo
        todo = x >= np.uint64(n)
    return x.astype(np.int64)


def minibatch(m, B, index, n, seed, rollout_count, ep, obs, actions, logp, values, returns, adv):
    """Rule 3: the dict ``obs, actions, logp, values, returns, adv, weight, slot`` of minibatch ``m``; the sources are ``[T, E, ...]``
    arrays (``obs`` and ``values`` may carry the buffer's slot ``T`` behind them) and keep their dtypes."""
    m, B, n = int(m), int(B), int(n)
    index = np.asarray(index)
    N = index.shape[0]
    rows = lambda x, w: np.asarray(x).reshape(-1, *w)[:N]  # noqa: E731
    obs, actions = np.asarray(obs), np.asarray(actions)
    src = dict(obs=rows(obs, obs.shape[2:]), actions=rows(actions, actions.shape[2:]), logp=rows(logp, ()), values=rows(values, ()),
               returns=rows(returns, ()), adv=rows(adv, ()))
    out = {k: np.zeros((B,) + v.shape[1:], dtype=v.dtype) for k, v in src.items()}
    out["weight"] = np.zeros(B, dtype=src["values"].dtype)
    out["slot"] = np.full(B, -1, dtype=np.int32)
    live = max(0, min(B, n - m * B))
    if live:
        s = index[perm_v(m * B + np.arange(live), n, seed, rollout_count, ep)]
        for k, v in src.items():
            out[k][:live] = v[s]          # (fancy indexing copies bits: no arithmetic touches a NaN's payload)
        out["weight"][:live] = 1
        out["slot"][:live] = s
    return out


def check_args(batch_size, seed=0, advantage="norm"):
    """``(B, seed, advantage)``; what needs no device to refuse raises ``ArgsError``."""
    try:
        if isinstance(batch_size, bool):
            raise TypeError
        B = operator.index(batch_size)
    except TypeError:
        raise E.ArgsError("The argument batch_size is %r but should be a positive integer." % (batch_size,)) from None
    if B < 1:
        raise E.ArgsError("The argument batch_size is %r but should be a positive integer." % (batch_size,))
    if B > 1 << 30:
        raise E.ArgsError("The argument batch_size is %r but a minibatch takes at most 2^30 rows." % (batch_size,))
    if not (isinstance(advantage, str) and advantage in ("norm", "raw")):
        raise E.ArgsError("The argument advantage is %r but should be 'norm' or 'raw'." % (advantage,))
    try:
        if isinstance(seed, bool):
            raise TypeError
        sd = operator.index(seed)
    except TypeError:
        raise E.ArgsError("The argument seed is %r but should be an integer in [0, 2^64)." % (seed,)) from None
    if not 0 <= sd < 1 << 64:
        raise E.ArgsError("The argument seed is %r but should be an integer in [0, 2^64)." % (seed,))
    return B, sd, advantage


def range_counts(n_slots):
    """Length of the counts and the offsets buffer: one int32 each per aligned range of ``prepare`` (``rollout.slab_range``)."""
    return -(-int(n_slots) // slab_range(n_slots))


# ---- the device half -------------------------------------------------------------------------------------------------------------
class Minibatch:
    """What ``MinibatchSampler.gather`` returns: the same persistent tensors at every call.  ``obs [B, D]``, ``actions [B, A]``
    (io dtype); ``logp``, ``values``, ``returns``, ``adv``, ``weight`` ``[B]`` (value dtype); ``slot [B]`` int32."""
    __slots__ = FIELDS

    def __init__(self, **kw):
        for k in FIELDS:
            setattr(self, k, kw[k])


class MinibatchSampler:
    """Shuffled minibatches of a ``RolloutBuffer``, every tensor allocated once here (``buf.sampler(batch_size, seed=0,
    advantage="norm")``)::

        buf.finish(normalize=True)
        sampler.prepare()                                   # three launches
        for ep in range(K):
            for m in range(sampler.n_minibatches):          # ceil(T E / B): the bound that needs no sync
                mb = sampler.gather(m, ep)                  # one launch
                # the loss, weighted by mb.weight

    ``prepare`` and ``gather`` allocate nothing, do not synchronise and can be captured into a graph (``m`` and ``ep`` are
    constants of the captured launch).  Minibatches from ``count_minibatches()`` on are all padding."""

    def __init__(self, buf, batch_size, seed=0, advantage="norm"):
        from . import _lib

        B, sd, adv = check_args(batch_size, seed, advantage)
        torch = buf._torch
        lib = buf._backend.lib
        if not hasattr(lib, "anm_minibatch_gather"):
            raise E.EnvInitializationError("MinibatchSampler needs the GPU library (minibatch.py rule 4)")
        self.buf, self.batch_size, self.seed, self.advantage = buf, B, sd, adv
        T, E_ = buf.n_steps, buf.num_envs
        D, A = buf.obs.shape[2], buf.actions.shape[2]
        N = T * E_
        self.n_minibatches = -(-N // B)
        dev = buf.device
        fio, fv = dict(dtype=buf.io_dtype, device=dev), dict(dtype=buf.value_dtype, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.index = torch.full((N,), -1, **i32)
        self._counts = torch.zeros(range_counts(N), **i32)
        self._offsets = torch.zeros(range_counts(N), **i32)
        self._state = torch.zeros(STATE_SIZE, dtype=torch.int64, device=dev)
        self.mb = Minibatch(obs=torch.zeros((B, D), **fio), actions=torch.zeros((B, A), **fio), logp=torch.zeros(B, **fv),
                            values=torch.zeros(B, **fv), returns=torch.zeros(B, **fv), adv=torch.zeros(B, **fv),
                            weight=torch.zeros(B, **fv), slot=torch.full((B,), -1, **i32))
        code = {torch.float64: _lib.IO_F64, torch.float32: _lib.IO_F32}
        src_adv = buf.adv_norm if adv == "norm" else buf.advantages
        o = self.mb
        self._struct = _lib.Minibatch(
            obs=buf.obs.data_ptr(), actions=buf.actions.data_ptr(), logp=buf.logp.data_ptr(), values=buf.values.data_ptr(),
            returns=buf.returns.data_ptr(), adv=src_adv.data_ptr(), flags=buf.flags.data_ptr(), index=self.index.data_ptr(),
            counts=self._counts.data_ptr(), offsets=self._offsets.data_ptr(), n_counts=self._counts.numel(),
            state=self._state.data_ptr(), mb_obs=o.obs.data_ptr(), mb_actions=o.actions.data_ptr(), mb_logp=o.logp.data_ptr(),
            mb_values=o.values.data_ptr(), mb_returns=o.returns.data_ptr(), mb_adv=o.adv.data_ptr(), mb_weight=o.weight.data_ptr(),
            mb_slot=o.slot.data_ptr(), T=T, E=E_, D=D, A=A, B=B, io_dtype=code[buf.io_dtype], value_dtype=code[buf.value_dtype],
            seed=sd)
        self._ref = C.byref(self._struct)
        self._lib, self._check = lib, buf._backend.check

    def prepare(self):
        """Rule 1 over the buffer's flags: ``index``, ``n_valid``, and ``rollout_count`` one higher."""
        rc = self._lib.anm_minibatch_prepare(self._ref, self.buf._stream())
        if rc != 0:
            self._check(rc, "anm_minibatch_prepare")

    def gather(self, m, ep=0):
        """Rule 3: minibatch ``m`` of epoch ``ep`` of the rollout prepared last, in the persistent tensors of ``self.mb``."""
        rc = self._lib.anm_minibatch_gather(self._ref, m, ep, self.buf._stream())
        if rc != 0:
            self._check(rc, "anm_minibatch_gather")
        return self.mb

    def count_minibatches(self):
        """``ceil(n_valid / B)`` of the rollout prepared last (one small copy to the host): the minibatches that are not
        all padding."""
        return -(-int(self._state[0].item()) // self.batch_size)

    def state(self):
        """What a checkpoint keeps (one small copy to the host)."""
        return dict(rollout_count=int(self._state[1].item()))

    def load_state(self, state):
        try:
            count = operator.index(state["rollout_count"])
        except (TypeError, KeyError):
            raise E.ArgsError("load_state takes what state() returned: a dict with the integer rollout_count") from None
        if not 0 <= count < 1 << 63:
            raise E.ArgsError("rollout_count is %r but should be in [0, 2^63)" % (count,))
        self._state[1] = count
