"""Diagonal-Gaussian actor-critic of two MLPs whose ``act()`` is ONE launch (``GaussianMLPPolicy``; ``anm_policy_act`` in the C
ABI): the specification the kernel of csrc/anm_policy.hpp follows.  Like ``rollout.py``, ``minibatch.py`` and ``rng.py`` this text
is normative.  Two stages are transcendental and device-only -- the Box-Muller noise of rule 5 and ``std`` of rule 4 -- and are
pinned to exact references by derived bounds of 1 float32 ulp; everything downstream of them takes ``eps`` and ``std`` as
ARGUMENTS (:func:`forward`) and is compared on bit patterns.

The layout is SB3's / CleanRL's for continuous control: a separate actor MLP ``D -> hidden -> A`` and critic MLP
``D -> hidden -> 1``, a state-independent ``log_std [A]``.  All parameters are ONE flat float32 vector (:func:`layout`): the actor's
layers in order, each ``W [K, N]`` row-major (so a layer is ``x @ W + b``) then ``b [N]``; the critic's layers the same way; then
``log_std``.  Everything below is float32 unless said otherwise.

1. Input.  ``x0 = float32(obs[e, :])``: one round-to-nearest for a float64 row, the identity for float32.
2. Layer.  For output ``n``: ``acc = b[n]``, then for ``k = 0 .. K-1`` ascending ``acc = fmaf(x[k], W[k, n], acc)`` -- a chain over the
   real ``K`` only, no padding term (``+0 * +0`` added to an accumulator ``-0.0`` would give ``+0.0``).  Hidden layers apply the
   activation; the heads (mean ``[A]``, the value scalar) apply none.  (:func:`layer`; ``fmaf`` is :func:`fma32_v`)
3. Activations.  ``relu(x) = +0 if x < 0 else x`` (a NaN passes, ``-0`` stays).  ``tanh32`` is a device-only function written out as
   operations: ``c = 7.90531110763549805 if x > 7.9.. else (-7.9.. if x < -7.9.. else x)`` (selects: a NaN passes);
   ``x2 = c * c``; ``p`` the Horner chain ``fmaf(x2, p, a_i)`` over the odd numerator's coefficients ``TANH_ALPHA`` (from ``a13`` down
   to ``a1``), then ``p = c * p``; ``q`` the same chain over the even denominator's ``TANH_BETA`` (``b6`` down to ``b0``); ``r = p / q``,
   ONE IEEE float32 division; ``r`` is then clamped to ``[-1, 1]`` by selects; the result is ``x`` itself where ``|x| < 0.0004`` and
   ``r`` elsewhere.  The coefficients are the 13/6 rational minimax fit of Eigen's ``generic_fast_tanh_float`` (MPL2).  Odd,
   ``|tanh32| <= 1``, ``tanh32(+-0) = +-0``, ``tanh32(NaN) = NaN``.  (:func:`tanh32`)
4. ``std[j] = float32(exp(float64(log_std[j])))``.  The kernel writes what it used to ``pi.std``.  Bound, derived: the float64 library
   ``exp`` is within a few float64 ulp, so the stored float32 is the correctly rounded value or its neighbour: at most 1 float32 ulp
   from the exact value.  (:func:`std_of`)
5. Noise: a pure function of the environment's own counters.  Environment ``e`` (global index ``g = env_offset + e``) takes the key
   ``K' = words 0, 1 of rng.philox4x32(seed, g, reset_count[e], POLICY_KEY_DRAW)`` and pair ``p = j // 2`` the block
   ``q = rng.philox4x32(K', timestep[e] | p << 32, 0, POLICY_TAG)``; ``reset_count`` and ``timestep`` enter as uint32.  No other
   stream uses either tag (``rng.EXO_KEY_DRAW``, ``rng.EXO_TAG``, ``minibatch.MB_TAG + r``, the init sampler's small draw numbers), so
   equal seeds never collide with the task's draws.  ``u1 = 1 - u01(q0, q1)`` in ``(0, 1]``, ``u2 = u01(q2, q3)``; in float64
   ``r = sqrt(-2 * log(u1))``, ``t = TWO_PI * u2`` (one rounded product, ``TWO_PI = float64(2 pi)``), ``eps[2p] = float32(r * cos t)``,
   ``eps[2p + 1] = float32(r * sin t)`` (``sincos_medium`` of csrc/anm_device.hpp); an odd ``A`` drops the last sine.  The kernel writes
   ``eps`` to ``pi.noise``.  Bound, derived as in rule 4: at most 1 float32 ulp from the exact Box-Muller image
   ``sqrt(-2 ln u1) cos / sin (2 pi u2)`` of the uniforms.  (The float64 angle carries an ABSOLUTE error of about 1.5e-15, so the
   bound is lost where ``|cos|`` or ``|sin|`` is below 2.5e-8: ``u2`` within 4e-9 of a multiple of 1/4, about 3 draws in 10^8; there
   the error stays below 2e-15 times ``r``.)  ``deterministic=True`` draws nothing: ``eps = +0``.  (:func:`uniforms`, :func:`noise`)
6. Outputs.  ``action[j] = fmaf(std[j], eps[j], mean[j])`` (with ``eps = +0`` that is ``mean[j]``, a ``-0.0`` mean becoming ``+0.0``).
   ``logp``: ``acc = float32(-0.5 * A * ln(2 pi))``, formed in float64 and rounded once; then for ``j`` ascending
   ``acc = fmaf(-0.5f * eps[j], eps[j], acc)`` (the product by ``-0.5f`` is exact) and ``acc = acc - log_std[j]``, one subtraction of
   its own.  ``value`` is the critic's head.
7. Stores widen exactly to the output dtype (``actions``: the io dtype; ``values``, ``logp``: float32 or float64, read from the tensors;
   ``noise``, ``std``: float32); a NaN is stored as the canonical quiet NaN, the convention of ``rollout.py``.  Rows are independent: a
   NaN observation row makes its own actions and value NaN (``logp`` is a function of ``eps`` and ``log_std`` alone) and touches no
   neighbour.  Rows past ``E`` are neither read nor written.
8. Limits.  1 to 3 hidden layers, each width a multiple of 32 in ``[32, 256]``; ``D`` in ``[1, 256]``; ``A`` in ``[1, 64]``; and the
   kernel's LDS plan: both nets' weights are staged whole, beside two activation tiles and one noise tile of 32 rows per
   wavefront.  With ``P`` the parameter count, ``H`` the widest hidden layer and ``x|1`` the next odd number, a workgroup of ``w``
   wavefronts takes ``P + 96 + 32 w (2 (max(D, H, A)|1) + (A|1))`` floats of the 40 960 (160 KiB) a workgroup can have; the library
   launches ``w = 4`` where that fits, else 2, else 1, and a network that does not fit ``w = 1`` is refused.  ANM6 (``D = 18``,
   ``A = 6``) with ``(64, 64)`` takes 28 845 floats at ``w = 4``; ``(96, 96)`` runs at ``w = 2``, ``(256,)`` at ``w = 1``; ``(128, 128)``
   (38 797 parameters) is refused.
   (:func:`lds_floats`)
   Not served: float64 or bf16 parameters, a shared trunk, state-dependent ``std``, tanh-squashed actions, recurrent policies,
   ``MixedBatchedANMEnv``, a backend other than the GPU library; the optimiser and gradient-norm clipping stay torch's (the
   gradient of the PPO loss is ``ppo_gradient``, policy_grad.py; ``evaluate`` remains for other losses).  The policy emits the unbounded Gaussian: clamping stays in the step kernel (``action_map="unit"``).  Acting twice
   on an unchanged environment row repeats the draw, by construction.
"""

from __future__ import annotations

import ctypes as C
import math
import operator

import numpy as np

from . import errors as E
from . import rng

POLICY_KEY_DRAW = 0x504F4C4B          # "POLK"
POLICY_TAG = 0x504F4C31               # "POL1"
TWO_PI = 6.283185307179586            # float64(2 pi)
TANH_CLAMP = np.float32(7.90531110763549805)
TANH_TINY = np.float32(0.0004)
TANH_ALPHA = tuple(np.float32(x) for x in (   # a13 .. a1
    -2.76076847742355e-16, 2.00018790482477e-13, -8.60467152213735e-11, 5.12229709037114e-08, 1.48572235717979e-05,
    6.37261928875436e-04, 4.89352455891786e-03))
TANH_BETA = tuple(np.float32(x) for x in (1.19825839466702e-06, 1.18534705686654e-04, 2.26843463243900e-03,   # b6 .. b0
                                          4.89352518554385e-03))
ACT_TANH, ACT_RELU = 0, 1
ACTIVATIONS = {"tanh": ACT_TANH, "relu": ACT_RELU}
MAX_HIDDEN_LAYERS, MIN_WIDTH, MAX_WIDTH, MAX_D, MAX_A = 3, 32, 256, 256, 64
LDS_FLOATS = 160 * 1024 // 4


# ---- the specification ---------------------------------------------------------------------------------------------------------
def fma32_v(a, b, c):
    """Correctly rounded float32 ``a * b + c`` over arrays (broadcast).  The float64 product of two float32 is exact; its sum
    with ``c`` is kept as an exact two-term expansion (``rng._two_sum``), rounded to odd, and rounded once to float32 (Boldo and
    Melquiond 2008: 53 >= 24 + 2 bits make the second rounding innocuous)."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s, e = rng._two_sum(p, c)
        fix = np.isfinite(s) & (e != 0) & ((np.asarray(s).view(np.int64) & 1) == 0)     # (a NaN e compares unequal: s is not finite then)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return np.asarray(s).astype(np.float32)


def relu32(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x < 0, np.float32(0.0), x).astype(np.float32)


def tanh32(x):
    """Rule 3."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        c = np.where(x > TANH_CLAMP, TANH_CLAMP, np.where(x < -TANH_CLAMP, -TANH_CLAMP, x)).astype(np.float32)
        x2 = (c * c).astype(np.float32)
        p = np.broadcast_to(TANH_ALPHA[0], x2.shape)
        for a in TANH_ALPHA[1:]:
            p = fma32_v(x2, p, a)
        p = (c * p).astype(np.float32)
        q = np.broadcast_to(TANH_BETA[0], x2.shape)
        for b in TANH_BETA[1:]:
            q = fma32_v(x2, q, b)
        r = (p / q).astype(np.float32)
        one = np.float32(1.0)
        r = np.where(r > one, one, np.where(r < -one, -one, r)).astype(np.float32)
        return np.where(np.abs(x) < TANH_TINY, x, r).astype(np.float32)


def layer(x, W, b, activation=None):
    """Rule 2: ``[E, K]`` through ``W [K, N]``, ``b [N]``; ``activation`` None (a head), "tanh" or "relu"."""
    x, W, b = (np.asarray(v, dtype=np.float32) for v in (x, W, b))
    acc = np.broadcast_to(b[None, :], (x.shape[0], W.shape[1])).astype(np.float32)
    for k in range(W.shape[0]):
        acc = fma32_v(x[:, k, None], W[k][None, :], acc)
    if activation is None:
        return acc
    return tanh32(acc) if activation == "tanh" else relu32(acc)


def std_of(log_std):
    """Rule 4."""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(log_std, dtype=np.float32).astype(np.float64)).astype(np.float32)


def uniforms(seed, env_offset, reset_count, timestep, A):
    """Rule 5: ``(u1, u2)``, float64 ``[E, ceil(A / 2)]`` each."""
    rc = (np.asarray(reset_count).astype(np.int64).reshape(-1) & rng.MASK).astype(np.uint64)
    ts = (np.asarray(timestep).astype(np.int64).reshape(-1) & rng.MASK).astype(np.uint64)
    g = np.uint64(int(env_offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(rc.shape[0], dtype=np.uint64)
    kw = rng.philox4x32_v(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), g, rc, np.uint64(POLICY_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))
    P = (int(A) + 1) // 2
    p = np.arange(P, dtype=np.uint64)[None, :]
    q = rng.philox4x32_v(key[:, None], ts[:, None] | (p << np.uint64(32)), np.uint64(0), np.uint64(POLICY_TAG))
    return 1.0 - rng.u01_v(q[..., 0], q[..., 1]), rng.u01_v(q[..., 2], q[..., 3])


def box_muller(u1, u2):
    """Rule 5: ``(z_cos, z_sin)`` in float64, before the rounding to float32 (NumPy's library functions stand in for the
    device's here: the device is held to the exact image, not to these bits)."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    t = TWO_PI * u2
    return r * np.cos(t), r * np.sin(t)


def noise(seed, env_offset, reset_count, timestep, A, deterministic=False):
    """Rule 5: ``eps``, float32 ``[E, A]``."""
    n = np.asarray(reset_count).reshape(-1).shape[0]
    if deterministic:
        return np.zeros((n, int(A)), dtype=np.float32)
    zc, zs = box_muller(*uniforms(seed, env_offset, reset_count, timestep, A))
    out = np.empty((n, 2 * zc.shape[1]), dtype=np.float32)
    out[:, 0::2], out[:, 1::2] = zc.astype(np.float32), zs.astype(np.float32)
    return np.ascontiguousarray(out[:, :int(A)])


def logp_const(A):
    """Rule 6: ``float32(-0.5 * A * ln(2 pi))``."""
    return np.float32(-0.5 * float(int(A)) * math.log(2.0 * math.pi))


def layout(D, A, hidden):
    """The flat parameter vector: ``(entries, P)``, entries ``(net, layer, "weight" | "bias", offset, shape)`` with ``net`` "actor" or
    "critic", and ``("log_std", 0, "log_std", offset, (A,))`` last."""
    out, at = [], 0
    for net, n_out in (("actor", int(A)), ("critic", 1)):
        widths = [int(D)] + [int(h) for h in hidden] + [n_out]
        for i in range(len(widths) - 1):
            K, N = widths[i], widths[i + 1]
            out.append((net, i, "weight", at, (K, N)))
            at += K * N
            out.append((net, i, "bias", at, (N,)))
            at += N
    out.append(("log_std", 0, "log_std", at, (int(A),)))
    return out, at + int(A)


def unpack(flat, D, A, hidden):
    """``dict(actor=[(W, b), ...], critic=[(W, b), ...], log_std=...)``: float32 views of a flat NumPy vector."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    entries, P = layout(D, A, hidden)
    if flat.shape[0] != P:
        raise E.ArgsError("the flat parameter vector has %d entries but the layout takes %d" % (flat.shape[0], P))
    nets = dict(actor=[], critic=[])
    for net, i, kind, at, shape in entries:
        v = flat[at:at + int(np.prod(shape))].reshape(shape)
        if kind == "log_std":
            nets["log_std"] = v
        elif kind == "weight":
            nets[net].append([v, None])
        else:
            nets[net][i][1] = v
    return dict(actor=[tuple(x) for x in nets["actor"]], critic=[tuple(x) for x in nets["critic"]], log_std=nets["log_std"])


def _store(x, dtype):
    out = np.asarray(x, dtype=np.float32).astype(dtype)
    out[np.isnan(out)] = np.nan
    return out


def mlp(layers, x0, activation):
    x = x0
    for i, (W, b) in enumerate(layers):
        x = layer(x, W, b, activation if i + 1 < len(layers) else None)
    return x


def forward(params, obs, eps, std, activation="tanh", value_dtype=None):
    """Rules 1, 2, 3, 6, 7 from the noise and ``std`` of rules 4 and 5: a dict ``actions`` (the dtype of ``obs``), ``values``, ``logp``
    (``value_dtype``, default the dtype of ``obs``) and ``mean`` (float32, before the store)."""
    obs = np.asarray(obs)
    vdt = np.dtype(obs.dtype if value_dtype is None else value_dtype)
    eps, std = np.asarray(eps, dtype=np.float32), np.asarray(std, dtype=np.float32)
    log_std = np.asarray(params["log_std"], dtype=np.float32)
    with np.errstate(all="ignore"):
        x0 = obs.astype(np.float32)
        mean = mlp(params["actor"], x0, activation)
        value = mlp(params["critic"], x0, activation)[:, 0]
        A = mean.shape[1]
        actions = fma32_v(std[None, :], eps, mean)
        acc = np.full(obs.shape[0], logp_const(A), dtype=np.float32)
        for j in range(A):
            acc = fma32_v(np.float32(-0.5) * eps[:, j], eps[:, j], acc)
            acc = (acc - log_std[j]).astype(np.float32)
    return dict(actions=_store(actions, obs.dtype), values=_store(value, vdt), logp=_store(acc, vdt), mean=mean)


def lds_floats(D, A, hidden, waves=1):
    """Rule 8: the floats of the kernel's LDS plan with ``waves`` wavefronts per workgroup."""
    odd = lambda x: int(x) | 1  # noqa: E731
    return layout(D, A, hidden)[1] + 96 + 32 * int(waves) * (2 * odd(max(D, max(hidden), A)) + odd(A))


def _index(x, what, lo, hi):
    try:
        if isinstance(x, bool):
            raise TypeError
        v = operator.index(x)
    except TypeError:
        raise E.ArgsError("The argument %s is %r but should be an integer in [%d, %d]." % (what, x, lo, hi)) from None
    if not lo <= v <= hi:
        raise E.ArgsError("The argument %s is %r but should be an integer in [%d, %d]." % (what, x, lo, hi))
    return v


def check_args(D, A, hidden=(64, 64), activation="tanh", log_std_init=0.0, seed=0, init_seed=0):
    """``(D, A, hidden, activation code, log_std_init, seed, init_seed)``; what needs no device to refuse raises ``ArgsError``."""
    D, A = _index(D, "D (obs_dim)", 1, MAX_D), _index(A, "A (action_dim)", 1, MAX_A)
    try:
        hidden = tuple(hidden)
    except TypeError:
        raise E.ArgsError("The argument hidden is %r but should be a sequence of 1 to 3 widths." % (hidden,)) from None
    if not 1 <= len(hidden) <= MAX_HIDDEN_LAYERS:
        raise E.ArgsError("The argument hidden is %r but should hold 1 to 3 widths." % (hidden,))
    hidden = tuple(_index(h, "hidden[%d]" % i, MIN_WIDTH, MAX_WIDTH) for i, h in enumerate(hidden))
    if any(h % 32 for h in hidden):
        raise E.ArgsError("The argument hidden is %r but every width should be a multiple of 32." % (hidden,))
    if not (isinstance(activation, str) and activation in ACTIVATIONS):
        raise E.ArgsError("The argument activation is %r but should be 'tanh' or 'relu'." % (activation,))
    try:
        ls = float(log_std_init)
    except (TypeError, ValueError):
        ls = np.nan
    if not np.isfinite(ls):
        raise E.ArgsError("The argument log_std_init is %r but should be a finite number." % (log_std_init,))
    need = lds_floats(D, A, hidden)
    if need > LDS_FLOATS:
        raise E.ArgsError("A network of D = %d, hidden = %r, A = %d takes %d floats of LDS but the kernel's plan has %d "
                          "(policy.py rule 8)." % (D, hidden, A, need, LDS_FLOATS))
    return (D, A, hidden, ACTIVATIONS[activation], ls, _index(seed, "seed", 0, (1 << 64) - 1),
            _index(init_seed, "init_seed", 0, (1 << 64) - 1))


def orthogonal(rows, cols, gain, gen):
    """``[rows, cols]`` with orthonormal rows or columns times ``gain`` (the QR recipe of ``torch.nn.init.orthogonal_``), drawn
    from a NumPy ``Generator`` on the host."""
    a = gen.standard_normal((max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.where(np.diag(r) == 0, 1.0, np.diag(r)))[None, :]
    if rows < cols:
        q = q.T
    return (gain * q).astype(np.float32)


def init_flat(D, A, hidden, log_std_init=0.0, init_seed=0):
    """The flat vector at construction: orthogonal weights (gain sqrt(2) for hidden layers, 0.01 for the policy head, 1 for the
    value head), zero biases, ``log_std = log_std_init``."""
    entries, P = layout(D, A, hidden)
    flat = np.zeros(P, dtype=np.float32)
    gen = np.random.default_rng(int(init_seed))
    for net, i, kind, at, shape in entries:
        if kind == "weight":
            head = i == len(hidden)
            gain = math.sqrt(2.0) if not head else (0.01 if net == "actor" else 1.0)
            flat[at:at + shape[0] * shape[1]] = orthogonal(shape[0], shape[1], gain, gen).reshape(-1)
        elif kind == "log_std":
            flat[at:at + shape[0]] = np.float32(log_std_init)
    return flat


# ---- the device half -------------------------------------------------------------------------------------------------------------
class _Layer:
    """``weight [K, N]`` and ``bias [N]``: views of the policy's flat parameter."""
    __slots__ = ("weight", "bias")

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def _module_base():
    import torch

    return torch.nn.Module


class GaussianMLPPolicy(_module_base()):
    """A diagonal-Gaussian actor-critic for a ``BatchedANMEnv`` on the GPU library, every tensor allocated once here::

        pi = GaussianMLPPolicy(env, hidden=(64, 64), activation="tanh", log_std_init=0.0, seed=0, init_seed=0)
        buf.begin(obs)
        for k in range(T):
            pi.act(buf.obs[k], buf.actions[k], buf.values[k], buf.logp[k])     # one launch
            out = env.step(buf.actions[k])
            buf.add(*out[:4])
        pi.value(buf.obs[T], buf.values[T])                                    # one launch, the critic alone
        buf.finish()
        logp, entropy, values = pi.evaluate(mb.obs, mb.actions)                # plain differentiable torch, for the loss

    ``act`` and ``value`` allocate nothing, do not synchronise and can be captured into a graph; the noise of a captured ``act`` is
    fresh at every replay because it is keyed by ``env.timestep`` and the environment's reset count (rule 5).  All parameters are
    the one flat ``nn.Parameter`` ``flat``; ``actor[i].weight`` (``[K, N]``), ``actor[i].bias``, ``critic[i]`` and ``log_std`` are views of
    it, and an optimiser that steps ``flat`` in place is seen by the next ``act`` through the same pointer.  ``noise`` ``[E, A]`` holds
    the ``eps`` the last ``act`` drew (zeros when deterministic), ``std`` ``[A]`` the ``exp(log_std)`` it used."""

    def __init__(self, env, hidden=(64, 64), activation="tanh", log_std_init=0.0, seed=0, init_seed=0):
        import torch

        from . import _lib
        from .envs.anm_env import BatchedANMEnv

        super().__init__()
        if not isinstance(env, BatchedANMEnv):
            raise E.EnvInitializationError("GaussianMLPPolicy serves a BatchedANMEnv (not %s: policy.py rule 8)" % type(env).__name__)
        sim = env.simulator
        D, A, hidden, act, ls, sd, isd = check_args(env.observation_N, sim.dims.action_dim, hidden, activation, log_std_init, seed,
                                                    init_seed)
        if sim.backend.device_type != "cuda" or not hasattr(sim.backend.lib, "anm_policy_act"):
            raise E.EnvInitializationError("GaussianMLPPolicy needs the GPU library (policy.py rule 8)")
        self.env, self.hidden, self.activation, self.seed = env, hidden, activation, sd
        self.obs_dim, self.action_dim, self.num_envs = D, A, env.num_envs
        self.device, self.io_dtype = env.device, env.io_dtype
        self.flat = torch.nn.Parameter(torch.from_numpy(init_flat(D, A, hidden, ls, isd)).to(self.device))
        self._entries, self.n_params = layout(D, A, hidden)
        self.actor, self.critic = [], []
        self._bind_views()
        self.noise = torch.zeros((env.num_envs, A), dtype=torch.float32, device=self.device)
        self.std = torch.zeros(A, dtype=torch.float32, device=self.device)
        self._code = {torch.float64: _lib.IO_F64, torch.float32: _lib.IO_F32}
        h3 = list(hidden) + [0] * (MAX_HIDDEN_LAYERS - len(hidden))
        self._struct = _lib.Policy(
            params=self.flat.data_ptr(), n_params=self.n_params, D=D, A=A, n_hidden=len(hidden), hidden=(C.c_int32 * 3)(*h3),
            activation=act, seed=sd, env_offset=env.env_offset, reset_count=env._reset_count.data_ptr(),
            timestep=env.timestep.data_ptr(), noise=self.noise.data_ptr(), std=self.std.data_ptr(), E=env.num_envs,
            io_dtype=self._code[self.io_dtype], value_dtype=self._code[self.io_dtype], deterministic=0)
        self._ref = C.byref(self._struct)
        self._backend, self._torch = sim.backend, torch

    def _bind_views(self):
        data = self.flat.data
        nets = dict(actor=self.actor, critic=self.critic)
        for lst in nets.values():
            del lst[:]
        for net, i, kind, at, shape in self._entries:
            v = data[at:at + int(np.prod(shape))].view(shape)
            if kind == "log_std":
                self.log_std = v
            elif kind == "weight":
                nets[net].append(_Layer(v, None))
            else:
                nets[net][i].bias = v

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _tensor(self, x, shape, what, dtypes):
        t = self._torch
        if not (isinstance(x, t.Tensor) and x.dtype in dtypes and x.device == self.device and tuple(x.shape) == shape
                and x.is_contiguous()):
            raise E.ArgsError("%s should be a contiguous %s tensor of shape %r on %s" % (
                what, " or ".join(str(d) for d in dtypes), shape, self.device))
        return x.data_ptr()

    def _launch(self, obs, actions, values, logp, deterministic):
        t = self._torch
        E_, D, A = self.num_envs, self.obs_dim, self.action_dim
        both = (t.float32, t.float64)
        po = self._tensor(obs, (E_, D), "obs", (self.io_dtype,))
        pv = self._tensor(values, (E_,), "values", both)
        pa = pl = None
        if actions is not None:
            pa = self._tensor(actions, (E_, A), "actions", (self.io_dtype,))
            pl = self._tensor(logp, (E_,), "logp", (values.dtype,))
        if self.flat.data_ptr() != self._struct.params:      # (a caller that re-assigned flat.data: follow it)
            self._struct.params = self.flat.data_ptr()
            self._bind_views()
        self._struct.value_dtype = self._code[values.dtype]
        self._struct.deterministic = 1 if deterministic else 0
        rc = self._backend.lib.anm_policy_act(self._ref, po, pa, pv, pl, self._stream())
        if rc != 0:
            self._backend.check(rc, "anm_policy_act")

    def act(self, obs, actions, values, logp, deterministic=False):
        """Rules 1 to 7 in one launch: reads ``obs [E, D]``, writes ``actions [E, A]`` (io dtype), ``values [E]`` and ``logp [E]`` (float32 or
        float64, both the same), ``self.noise`` and ``self.std``."""
        if actions is None or logp is None:
            raise E.ArgsError("act() writes actions and logp: both should be tensors (value() is the critic alone)")
        self._launch(obs, actions, values, logp, deterministic)

    def value(self, obs, values):
        """The critic alone, one launch: ``values [E]`` as ``act`` would write it, bit for bit; nothing else is touched."""
        self._launch(obs, None, values, None, True)

    def ppo_gradient(self, batch_size, clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None):
        """A ``policy_grad.PPOGradient``: ``g(mb)`` overwrites ``flat.grad`` with the gradient of the clipped PPO loss of a gathered
        minibatch, in two launches (policy_grad.py)."""
        from .policy_grad import PPOGradient

        return PPOGradient(self, batch_size, clip, vf_coef, ent_coef, vf_clip)

    def evaluate(self, obs, actions):
        """``(logp [B], entropy [B], values [B])`` of ``actions`` under the current parameters: plain differentiable float32 torch on
        the views of ``flat``, for the loss.  Same network, not the same bits as ``act``: torch sums in another order."""
        t = self._torch
        fn = t.tanh if self.activation == "tanh" else t.relu
        at = {(net, i, kind): (o, shape) for net, i, kind, o, shape in self._entries}

        def view(net, i, kind):
            o, shape = at[(net, i, kind)]
            return self.flat[o:o + int(np.prod(shape))].view(shape)

        def net_of(name, x):
            n = len(self.hidden) + 1
            for i in range(n):
                x = x @ view(name, i, "weight") + view(name, i, "bias")
                if i + 1 < n:
                    x = fn(x)
            return x

        x = obs.to(t.float32)
        mean, values = net_of("actor", x), net_of("critic", x)[:, 0]
        log_std = view("log_std", 0, "log_std")
        z = (actions.to(t.float32) - mean) * t.exp(-log_std)
        half_log_2pi = 0.5 * math.log(2.0 * math.pi)
        logp = (-0.5 * z * z - log_std - half_log_2pi).sum(dim=1)
        entropy = (log_std + (0.5 + half_log_2pi)).sum().expand(x.shape[0])
        return logp, entropy, values
