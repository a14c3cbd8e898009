"""Device rollout buffer of an on-policy loop: an in-stream transition store, GAE(lambda) and the advantage normalisation
(``RolloutBuffer``; ``anm_rollout_begin`` / ``_add`` / ``_gae`` / ``_adv_norm`` in the C ABI): the specification the kernels of
csrc/anm_rollout.hpp follow.  Like ``io_norm.py``, ``episode.py`` and ``rng.py`` this text is normative: the kernels are tested
against it bit for bit.

``step()`` returns the same persistent tensors at every call.  The buffer copies them into ``[T, num_envs, ...]`` slots with one
launch per step, and turns the slots into advantages and returns with one launch more (three more for the normalisation), all
in stream order behind the steps: nothing allocates, nothing synchronises with the host, and every result has the same bits
on every run.  It also settles WHICH slots are transitions at all.  The kernels use next-step autoreset (``episode.py`` rule
1): the call after an episode end re-initialises the environment, ignores the action and stores reward 0; a failed reset
draw looks absorbing and is retried; a terminated environment without autoreset is stepped as a no-op.  None of these calls
is a transition, and a slot that holds one must neither feed a loss nor carry a trace.

Buffers, ``T`` slots over ``E`` environments, ``D = obs_dim``, ``A = action_dim``::

    obs         [T+1, E, D]  io dtype          actions  [T, E, A]  io dtype       rewards  [T, E]  io dtype
    values      [T+1, E]     value dtype       logp     [T, E]     value dtype    flags    [T, E]  uint8
    advantages, returns, adv_norm  [T, E]  value dtype            t_seen  [E] int32
    statistics  float64 n, mean, var, std | int64 n_valid, n_norm_skipped

The io dtype is the environment's; the value dtype is float32 or float64, chosen at construction (default: the io dtype).
``actions``, ``values`` and ``logp`` are the policy's to write; no rule below reads ``actions`` or ``logp``.

Every product that feeds a sum is an explicit fma (``io_affine._fma`` here, ``fma()`` in the kernel); every other operation is
one IEEE double operation (``+ - * / sqrt``).  A float32 input is widened, which is exact.  An output is rounded ONCE to its
dtype, and a NaN is stored as the canonical quiet NaN (sign 0, payload 0): which NaN an operation produces is the one thing
IEEE leaves to the machine.

1. Begin.  ``obs[0]`` <- the observation the policy will act on; ``t_seen[e]`` <- ``timestep[e]``.
2. Add, after step call ``k``, from what the call stored: ``obs[k+1]`` <- the observation and ``rewards[k]`` <- the reward, plain
   copies in the io dtype.  ``VALID`` iff ``timestep[e] != t_seen[e] and timestep[e] != 0``: a real step.  Everything else is
   not a transition: the in-kernel autoreset call (``timestep == 0``), a failed or retried reset draw and the absorbing no-op
   (``timestep`` unchanged).  ``flags[k][e] = VALID | TERMINATED << 1 | TRUNCATED << 2``, the last two from the buffers after
   the call.  Then ``t_seen[e] = timestep[e]``.  (:func:`classify`)
   A host ``reset()`` between ``begin`` and the last ``add`` is NOT SERVED: it moves ``timestep`` behind the buffer's back
   (a masked reset followed by one step leaves ``timestep == 1``, which a row at ``t_seen == 1`` reads as a no-op).  ``begin``
   again after it.
3. GAE, in float64.  ``g = gamma``; ``gl = gamma * gae_lambda``, one double product, formed once.  Per environment
   ``A_next = +0.0``, then for ``k = T-1 ... 0``, with ``r = rewards[k]``, ``v = values[k]``:
   an invalid slot: ``advantages[k] = returns[k] = +0.0`` and ``A_next = +0.0``;
   a valid slot: ``delta = r - v`` if terminated, else ``fma(g, values[k+1], r) - v``; ``A = delta`` if terminated or truncated,
   else ``fma(gl, A_next, delta)``; ``advantages[k] = A``, ``returns[k] = A + v``, ``A_next = A`` (the double, not the rounded
   output).
   These are selects, not products by 0 / 1: a NaN in a value the rule does not use -- the value of a zeroed terminal
   observation -- reaches no output.  A truncated step bootstraps from ``values[k+1]``: with next-step autoreset ``obs[k+1]`` is
   the episode's true last observation (the reset happens in the NEXT call, whose slot is invalid and cuts the trace).
   (:func:`gae`)
4. Advantage moments, over valid slots only, by ONE fixed tree: ``io_norm.tree_sum`` over the flat index ``k * E + e``.  With
   ``a`` the STORED advantage, widened, a valid slot contributes the leaves ``a + 0.0`` and ``a * a``, an invalid slot ``+0.0`` and
   ``+0.0``; the leaves are padded by ``+0.0`` to a power of two; ``n``, the number of valid slots, is exact.  ``S1``, ``S2`` the
   roots: ``m = S1 / n``, ``t = fma(-m, m, S2 / n)``, ``var = 0.0 if t < 0.0 else t`` (a NaN passes),
   ``var_u = var * (n / (n - 1))`` (Bessel, as ``torch.std`` in SB3 and CleanRL), ``sd = sqrt(var_u)``.
   ``adv_norm = (a - m) / (sd + eps)`` on valid slots and ``+0.0`` elsewhere; ``eps`` defaults to 1e-8.  If ``n < 2``, or ``m``
   or ``sd`` is not finite, ``adv_norm`` is a copy of ``advantages`` and ``n_norm_skipped += 1``.  The statistics hold ``n``,
   ``mean = m``, ``var = var_u``, ``std = sd`` (all ``+0.0`` when ``n < 2``) and ``n_valid = n``.
   (:func:`adv_moments`, :func:`adv_normalise`)
   The kernels partition the flat index into aligned power-of-two ranges (``slab_range``); IEEE addition commutes, so the
   result does not depend on that grid.  ``T * E`` is at most 67 108 864 (4096 ranges of 16 384 slots).
5. Not served: ``MixedBatchedANMEnv``, batch views, a backend other than the GPU library, and a cross-rank merge of the
   moments (a sharded run normalises per rank).  Shuffled minibatches of the valid slots are ``RolloutBuffer.sampler``
   (``minibatch.py``); the loss stays with the caller.
"""

from __future__ import annotations

import ctypes as C
import operator

import numpy as np

from . import errors as E
from .io_affine import _fma
from .io_norm import tree_sum

VALID, TERMINATED, TRUNCATED = 1, 2, 4
EPS_DEFAULT = 1e-8
MIN_RANGE, MAX_RANGE, MAX_SLABS = 1024, 16384, 4096   # csrc/anm_rollout.hpp
MAX_SLOTS = MAX_RANGE * MAX_SLABS
STATS_SIZE = 8          # the device statistics block: float64 n, mean, var, std, std + eps, normalised | int64 n_valid, n_norm_skipped


# ---- the specification ---------------------------------------------------------------------------------------------------------
def classify(timestep, t_seen, terminated, truncated=None):
    """Rule 2: ``(flags, t_seen')`` of one add."""
    ts, seen = np.asarray(timestep).astype(np.int32), np.asarray(t_seen).astype(np.int32)
    term = np.asarray(terminated).astype(bool)
    trunc = np.zeros_like(term) if truncated is None else np.asarray(truncated).astype(bool)
    valid = (ts != seen) & (ts != 0)
    flags = valid.astype(np.uint8) * VALID | term.astype(np.uint8) * TERMINATED | trunc.astype(np.uint8) * TRUNCATED
    return flags.astype(np.uint8), ts.copy()


def _store(x, dtype):
    """One rounding to ``dtype``; a NaN becomes the canonical quiet NaN."""
    with np.errstate(all="ignore"):
        out = np.asarray(x, dtype=np.float64).astype(dtype)
    out[np.isnan(out)] = np.nan
    return out


def gae(rewards, values, flags, gamma, gae_lambda, value_dtype=None):
    """Rule 3: ``(advantages, returns)`` in the value dtype (default: that of ``values``)."""
    rewards, values, flags = np.asarray(rewards), np.asarray(values), np.asarray(flags)
    T = rewards.shape[0]
    if values.shape[0] != T + 1 or flags.shape != rewards.shape or values.shape[1:] != rewards.shape[1:]:
        raise E.ArgsError("gae: rewards and flags are [T, E], values is [T + 1, E]")
    vdt = np.dtype(values.dtype if value_dtype is None else value_dtype)
    r64, v64 = rewards.astype(np.float64), values.astype(np.float64)
    g = np.float64(gamma)
    gl = np.float64(gamma) * np.float64(gae_lambda)
    adv, ret = np.zeros(rewards.shape), np.zeros(rewards.shape)
    a_next = np.zeros(rewards.shape[1:])
    with np.errstate(all="ignore"):
        for k in range(T - 1, -1, -1):
            valid, term, trunc = (flags[k] & VALID) != 0, (flags[k] & TERMINATED) != 0, (flags[k] & TRUNCATED) != 0
            r, v = r64[k], v64[k]
            delta = np.where(term, r, _fma(g, v64[k + 1], r)) - v
            a = np.where(term | trunc, delta, _fma(gl, a_next, delta))
            a = np.where(valid, a, 0.0)
            adv[k], ret[k] = a, np.where(valid, a + v, 0.0)
            a_next = a
    return _store(adv, vdt), _store(ret, vdt)


def adv_moments(advantages, flags, eps=EPS_DEFAULT):
    """Rule 4: the statistics of the stored advantages, a dict ``n, mean, var, std, den, ok`` (``den = sd + eps``; ``ok``: the
    normalisation is not skipped)."""
    a = np.asarray(advantages).astype(np.float64).reshape(-1)
    valid = (np.asarray(flags).reshape(-1) & VALID) != 0
    n = int(valid.sum())
    with np.errstate(all="ignore"):
        s1 = tree_sum(np.where(valid, a + 0.0, 0.0))
        s2 = tree_sum(np.where(valid, a * a, 0.0))
        if n < 2:
            return dict(n=n, mean=0.0, var=0.0, std=0.0, den=1.0, ok=False)
        nn = np.float64(n)
        m = s1 / nn
        t = np.float64(np.reshape(_fma(-m, m, s2 / nn), ()))
        var = np.float64(0.0) if t < 0.0 else t
        var_u = var * (nn / (nn - 1.0))
        sd = np.sqrt(var_u)
        den = sd + np.float64(eps)
    canon = lambda x: float("nan") if np.isnan(x) else float(x)  # noqa: E731
    return dict(n=n, mean=canon(m), var=canon(var_u), std=canon(sd), den=canon(den), ok=bool(np.isfinite(m) and np.isfinite(sd)))


def adv_normalise(advantages, flags, moments):
    """Rule 4: ``adv_norm`` from the statistics of :func:`adv_moments`, in the dtype of ``advantages``."""
    advantages = np.asarray(advantages)
    if not moments["ok"]:
        return advantages.copy()
    valid = (np.asarray(flags) & VALID) != 0
    with np.errstate(all="ignore"):
        y = (advantages.astype(np.float64) - np.float64(moments["mean"])) / np.float64(moments["den"])
    return _store(np.where(valid, y, 0.0), advantages.dtype)


def normalise(advantages, flags, eps=EPS_DEFAULT, n_norm_skipped=0):
    """Rule 4 whole: ``(adv_norm, statistics)``, the statistics as ``RolloutBuffer.stats()`` reports them after this pass
    (``n_norm_skipped``: the count before it)."""
    mo = adv_moments(advantages, flags, eps)
    st = dict(n=float(mo["n"]), mean=mo["mean"], var=mo["var"], std=mo["std"], n_valid=mo["n"],
              n_norm_skipped=int(n_norm_skipped) + (0 if mo["ok"] else 1))
    return adv_normalise(advantages, flags, mo), st


def slab_range(n_slots):
    """Slots of one aligned range of k_adv_partial: 1024, doubled while that leaves more than 4096 ranges."""
    r = MIN_RANGE
    while r < MAX_RANGE and -(-int(n_slots) // r) > MAX_SLABS:
        r *= 2
    return r


def slab_doubles(n_slots):
    """Length of the slab buffer: one slab ``[S1, S2, n]`` per range."""
    return 3 * -(-int(n_slots) // slab_range(n_slots))


def _dtype_name(dtype, what):
    """'float32' | 'float64' of a torch or NumPy dtype (no torch import: the name is enough)"""
    name = str(dtype)[len("torch."):] if str(dtype).startswith("torch.") else None
    if name is None and not isinstance(dtype, str):
        try:
            name = np.dtype(dtype).name
        except TypeError:
            name = None
    if name not in ("float32", "float64"):
        raise E.ArgsError("The argument %s is %r but should be torch.float32 or torch.float64." % (what, dtype))
    return name


def check_args(n_steps, gae_lambda, gamma, value_dtype, adv_eps, io_dtype, num_envs=1):
    """``(T, gae_lambda, gamma, value dtype name, eps)``; what needs no device to refuse raises ``ArgsError``.  ``value_dtype``
    None: the io dtype."""
    try:
        if isinstance(n_steps, bool):
            raise TypeError
        T = operator.index(n_steps)
    except TypeError:
        raise E.ArgsError("The argument n_steps is %r but should be a positive integer." % (n_steps,)) from None
    if T < 1:
        raise E.ArgsError("The argument n_steps is %r but should be a positive integer." % (n_steps,))
    if T * int(num_envs) > MAX_SLOTS:
        raise E.ArgsError("n_steps * num_envs is %d but the buffer takes at most %d slots." % (T * int(num_envs), MAX_SLOTS))
    out = []
    for name, val in (("gae_lambda", gae_lambda), ("gamma", gamma)):
        try:
            x = float(val)
        except (TypeError, ValueError):
            x = np.nan
        if not 0.0 <= x <= 1.0:
            raise E.ArgsError("The argument %s is %r but should be a number in [0, 1]." % (name, val))
        out.append(x)
    try:
        eps = float(adv_eps)
    except (TypeError, ValueError):
        eps = np.nan
    if not (np.isfinite(eps) and eps > 0):
        raise E.ArgsError("The argument adv_eps is %r but should be a finite number > 0." % (adv_eps,))
    vname = _dtype_name(io_dtype if value_dtype is None else value_dtype, "value_dtype")
    return T, out[0], out[1], vname, eps


# ---- the device half -------------------------------------------------------------------------------------------------------------
class RolloutBuffer:
    """``T = n_steps`` slots of a ``BatchedANMEnv`` on the GPU library, every tensor allocated once here::

        buf.begin(obs)                                  # one launch
        for k in range(T):
            pi.act(buf.obs[k], buf.actions[k], buf.values[k], buf.logp[k])     # one launch (policy.py); or any policy that
            out = env.step(buf.actions[k])                                     # writes these contiguous slot views in place
            buf.add(*out[:4])                           # one launch; reads env.timestep
        pi.value(buf.obs[T], buf.values[T])             # one launch: the critic alone
        buf.finish(normalize=True)                      # the GAE launch (+ three for rule 4)

    ``begin()`` without an argument continues from ``obs[T]``.  ``begin``, ``add`` and ``finish`` allocate nothing, do not
    synchronise and can be captured into a graph.  A host ``reset()`` between ``begin`` and the last ``add`` is not served
    (rule 2): ``begin`` again after it."""

    def __init__(self, env, n_steps, gae_lambda=0.95, gamma=None, value_dtype=None, adv_eps=EPS_DEFAULT):
        import torch

        from . import _lib
        from .envs.anm_env import BatchedANMEnv

        if not isinstance(env, BatchedANMEnv):   # (MixedBatchedANMEnv is no BatchedANMEnv; its per-topology views stay inside it)
            raise E.EnvInitializationError("RolloutBuffer serves a BatchedANMEnv (not %s: rollout.py rule 5)" % type(env).__name__)
        T, lam, g, vname, eps = check_args(n_steps, gae_lambda, env.gamma if gamma is None else gamma, value_dtype, adv_eps,
                                           env.io_dtype, env.num_envs)
        sim = env.simulator
        if sim.backend.device_type != "cuda" or not hasattr(sim.backend.lib, "anm_rollout_add"):
            raise E.EnvInitializationError("RolloutBuffer needs the GPU library (rollout.py rule 5)")
        self.env, self.n_steps, self.gae_lambda, self.gamma, self.adv_eps = env, T, lam, g, eps
        self.device, self.io_dtype = env.device, env.io_dtype
        self.value_dtype = getattr(torch, vname)
        E_, D, A = env.num_envs, env.observation_N, sim.dims.action_dim
        self.num_envs = E_
        fio, fv = dict(dtype=self.io_dtype, device=self.device), dict(dtype=self.value_dtype, device=self.device)
        self.obs = torch.zeros((T + 1, E_, D), **fio)
        self.actions = torch.zeros((T, E_, A), **fio)
        self.rewards = torch.zeros((T, E_), **fio)
        self.values = torch.zeros((T + 1, E_), **fv)
        self.logp = torch.zeros((T, E_), **fv)
        self.flags = torch.zeros((T, E_), dtype=torch.uint8, device=self.device)
        self.advantages = torch.zeros((T, E_), **fv)
        self.returns = torch.zeros((T, E_), **fv)
        self.adv_norm = torch.zeros((T, E_), **fv)
        self.t_seen = torch.zeros(E_, dtype=torch.int32, device=self.device)
        self._stats = torch.zeros(STATS_SIZE, dtype=torch.float64, device=self.device)
        self._slabs = torch.zeros(slab_doubles(T * E_), dtype=torch.float64, device=self.device)
        code = {torch.float64: _lib.IO_F64, torch.float32: _lib.IO_F32}
        self._struct = _lib.Rollout(
            obs=self.obs.data_ptr(), rewards=self.rewards.data_ptr(), values=self.values.data_ptr(), flags=self.flags.data_ptr(),
            advantages=self.advantages.data_ptr(), returns=self.returns.data_ptr(), adv_norm=self.adv_norm.data_ptr(),
            t_seen=self.t_seen.data_ptr(), stats=self._stats.data_ptr(), slabs=self._slabs.data_ptr(),
            n_slab_doubles=self._slabs.numel(), T=T, E=E_, D=D, io_dtype=code[self.io_dtype], value_dtype=code[self.value_dtype],
            gamma=g, gae_lambda=lam, eps=eps)
        self._ref = C.byref(self._struct)
        self._backend, self._torch = sim.backend, torch
        self._k = 0
        self._timestep_ptr = env.timestep.data_ptr()

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _io_tensor(self, x, shape, what):
        if not (isinstance(x, self._torch.Tensor) and x.dtype == self.io_dtype and x.device == self.device
                and tuple(x.shape) == shape and x.is_contiguous()):
            raise E.ArgsError("%s should be a contiguous %s tensor of shape %r on %s" % (what, self.io_dtype, shape, self.device))
        return x.data_ptr()

    def begin(self, obs=None):
        """Rule 1; without ``obs``: continue from the last observation of the rollout before (``obs[T]``)."""
        E_, D = self.num_envs, self.obs.shape[2]
        src = self.obs[self.n_steps].data_ptr() if obs is None else self._io_tensor(obs, (E_, D), "obs")
        rc = self._backend.lib.anm_rollout_begin(self._ref, src, self._timestep_ptr, self._stream())
        if rc != 0:
            self._backend.check(rc, "anm_rollout_begin")
        self._k = 0

    def add(self, obs, reward, terminated, truncated):
        """Rule 2 for the next slot, from what ``step()`` returned (and ``env.timestep``)."""
        E_, k = self.num_envs, self._k
        if k >= self.n_steps:
            raise E.ArgsError("the rollout is full (%d slots): finish() and begin()" % self.n_steps)
        for name, f in (("terminated", terminated), ("truncated", truncated)):
            if not (isinstance(f, self._torch.Tensor) and f.element_size() == 1 and f.device == self.device and tuple(f.shape) == (E_,)):
                raise E.ArgsError("%s should be the bool / uint8 tensor of shape (%d,) that step() returned" % (name, E_))
        rc = self._backend.lib.anm_rollout_add(self._ref, k, self._io_tensor(obs, (E_, self.obs.shape[2]), "obs"),
                                               self._io_tensor(reward, (E_,), "reward"), terminated.data_ptr(), truncated.data_ptr(),
                                               self._timestep_ptr, self._stream())
        if rc != 0:
            self._backend.check(rc, "anm_rollout_add")
        self._k = k + 1

    def finish(self, normalize=True):
        """Rules 3 and (``normalize``) 4 over the whole buffer."""
        lib = self._backend.lib
        stream = self._stream()
        rc = lib.anm_rollout_gae(self._ref, stream)
        if rc != 0:
            self._backend.check(rc, "anm_rollout_gae")
        if normalize:
            rc = lib.anm_rollout_adv_norm(self._ref, stream)
            if rc != 0:
                self._backend.check(rc, "anm_rollout_adv_norm")

    def sampler(self, batch_size, seed=0, advantage="norm"):
        """A :class:`~gym_anm_amd.minibatch.MinibatchSampler` over this buffer: shuffled minibatches of ``batch_size`` rows
        drawn from the valid slots (``minibatch.py``); ``advantage``: ``"norm"`` reads ``adv_norm``, ``"raw"`` ``advantages``.
        It allocates everything it needs once, here."""
        from .minibatch import MinibatchSampler

        return MinibatchSampler(self, batch_size, seed=seed, advantage=advantage)

    @property
    def valid(self):
        """``[T, E]`` bool: the slots that are transitions (rule 2)"""
        return (self.flags & VALID).view(self._torch.bool)

    def stats(self):
        """The statistics of the last ``finish(normalize=True)`` (one small copy to the host)."""
        s = self._stats.cpu().numpy()
        c = s.view(np.int64)
        return dict(n=float(s[0]), mean=float(s[1]), var=float(s[2]), std=float(s[3]), n_valid=int(c[6]), n_norm_skipped=int(c[7]))
