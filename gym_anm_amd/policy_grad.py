"""Gradient of the clipped PPO loss with respect to the flat parameter vector of ``GaussianMLPPolicy``, in TWO launches
(``PPOGradient``, from ``pi.ppo_gradient``; ``anm_policy_ppo_grad`` in the C ABI): the specification the kernels of
csrc/anm_policy_grad.hpp follow.  Like ``policy.py`` this text is normative.  Two stages are transcendental and device-only --
``inv_std`` of rule 2 and ``ratio`` of rule 4 -- and are pinned to exact references by derived bounds of 1 float32 ulp;
everything downstream of them takes ``ratio`` and ``inv_std`` as ARGUMENTS (:func:`backward`) and is compared on bit patterns.

Notation: a minibatch of ``B`` rows (the fields of ``minibatch.Minibatch``); ``w_i`` the row weight, a row is LIVE where
``w_i != 0`` (a NaN weight is live) and ``n`` counts the live rows; ``c = clip``, ``vc = vf_clip``, ``ls = log_std``; ``P`` parameters in
the layout of ``policy.layout``.  Everything is float32 unless said otherwise; ``fmaf`` is ``policy.fma32_v``; a product or a sum
written without ``fmaf`` is one rounded operation of its own.

1. Rows.  The rows are padded with dead rows to a multiple of 32.  Of a dead row nothing but the weight is read: its
   observation is ``+0`` in every column, its ``dY`` (rules 5, 6) and its statistics are ``+0``, and ``logp``, ``values`` and ``ratio`` store
   ``+0`` for it.  The forward pass of a live row is rules 1 to 3 of ``policy.py``, unchanged: ``mean`` and ``v`` are the chains of
   ``act``, so ``values`` equals what ``pi.value`` writes, bit for bit.  Every layer's activation is kept.
2. ``inv_std[j] = float32(exp(-float64(ls[j])))``, written to ``g.inv_std``.  Bound, derived as in rule 4 of ``policy.py``: the negation
   is exact and the float64 library ``exp`` is within a few float64 ulp, so the float32 is the correctly rounded value or its
   neighbour: at most 1 float32 ulp.  (:func:`inv_std_of`)
3. ``z[j] = (float32(a[j]) - mean[j]) * inv_std[j]``.  ``logp``: ``acc = logp_const(A)``, then for ``j`` ascending
   ``acc = fmaf(-0.5f * z[j], z[j], acc)`` and ``acc = acc - ls[j]`` (rule 6 of ``policy.py`` with ``z`` for ``eps``).
   ``lr = logp - float32(logp_old)``.  (:func:`log_ratio`)
4. ``ratio = float32(exp(float64(lr)))``, written per row to ``g.ratio``.  Bound: 1 float32 ulp, as in rule 2 (the widening of
   ``lr`` is exact).  (:func:`ratio_of`)
5. Policy term.  ``lo = 1 - c``, ``hi = 1 + c``; ``s1 = ratio * adv``; ``rc = lo if ratio < lo else (hi if ratio > hi else ratio)``
   (selects: a NaN passes); ``s2 = rc * adv``; ``pg = -(s2 if s2 < s1 else s1)``.  The clipped branch is active where
   ``adv >= 0 and ratio > hi`` or ``adv < 0 and ratio < lo`` (a NaN is never clipped: it poisons).  ``cl = w * (+0 if clipped else -s1)``
   is ``d loss / d logp`` times ``n``.  Head: ``dY[j] = cl * (z[j] * inv_std[j])``; ``g_ls[j] = cl * fmaf(z[j], z[j], -1)``.
6. Value term.  ``d = v - ret``, ``big = d * d``, ``gr = d``.  With ``vf_clip``: ``dv = v - v_old``,
   ``dc = -vc if dv < -vc else (vc if dv > vc else dv)``, ``d2 = (v_old + dc) - ret``, ``e2 = d2 * d2``; where ``e2 > big``:
   ``big = e2`` and ``gr = +0 if the clamp is active else d2``.  Head: ``dY[0] = (w * vf_coef) * gr``.
7. Statistics of a row: ``w * pg``, ``w * (0.5f * big)``, ``w * ((ratio - 1) - lr)``, ``1 if ratio > hi or ratio < lo else 0``, and ``1``
   (the count).
8. Partial gradients.  ``R = rows_per_partial(B)``; group ``g`` is the rows ``[g R, min((g + 1) R, B'))`` with ``B'`` the padded row
   count.  For every layer the augmented input is ``x' = [x, 1]`` (so row ``K`` of ``W' = [W; b]`` is the bias) and entry
   ``(k, n)`` of the group's partial is ``acc = +0``, then for the group's rows ascending ``acc = fmaf(x'[row, k], dY[row, n], acc)``:
   what ``v_mfma_f32_32x32x2_f32`` computes with the row as its ``k``.  ``log_std`` and the five statistics are the same chain with
   ``x' = [1]`` over ``g_ls`` and rule 7.  A partial is ``P + 8`` floats: the gradient words, the five sums, three zeros.
   (:func:`chain_rows`)
9. Through a layer, ``dX = dY W^T``: ``acc = +0``, then for ``n = 0 .. N-1`` ascending ``acc = fmaf(dY[row, n], W[k, n], acc)``, and for
   an odd ``N`` (a head) one more ``acc = fmaf(+0, +0, acc)`` (the instruction takes ``n`` in pairs; it turns a ``-0.0`` that an
   underflow left into ``+0.0``).  Through the activation, from its stored output ``y``: tanh ``dY' = acc * fmaf(-y, y, 1)``; relu
   ``dY' = acc if y > 0 else +0``.  The critic's backward pass runs first, then the actor's; they share nothing.
10. Reduction.  ``S = +0``, then ``S = S + partial[g]`` for ``g`` ascending.  ``nf = S[count]``.  With ``nf == 0`` every gradient word
    and every statistic is ``+0``.  Otherwise ``grad[p] = S[p] / nf`` (one IEEE division), and for the ``log_std`` entries then
    ``grad[p] = grad[p] - ent_coef``.  ``grad`` is OVERWRITTEN: there is no ``zero_grad``.  Statistics:
    ``H``: ``acc = +0``, ``acc = acc + (ls[j] + float32(0.5 + 0.5 ln 2 pi))`` for ``j`` ascending; ``pg_loss = S[pg] / nf``;
    ``v_loss = S[v] / nf``; ``loss = fmaf(-ent_coef, H, fmaf(vf_coef, v_loss, pg_loss))``; ``approx_kl = S[kl] / nf``;
    ``clip_frac = S[clip] / nf``; ``stats = (loss, pg_loss, v_loss, H, approx_kl, clip_frac, nf, 0)``.  (:func:`reduce_partials`)
11. Determinism.  Every order above is a function of ``B``, ``R`` and the network's shape: no atomics, and neither the grid nor
    the number of compute units enters.  ``rows_per_partial(B)`` is 32 doubled while that leaves more than 512 partials (128 at ``B = 65 536``: one group per wavefront
    of a device of 256 compute units at two wavefronts each; measured).
12. Limits.  Those of ``policy.py`` rule 8 for the shape; ``B`` in ``[1, 2^24]`` (the count is exact in float32); ``clip > 0``;
    and the backward LDS plan: the parameters staged whole, a transposed copy ``[N | even, K]`` of every layer that has a
    hidden layer below it (``T`` floats), and per wavefront ``n_hidden + 2`` activation tiles of 32 rows and stride
    ``S = (max(D, H, A) + 1) | 1`` (one column more for the 1.0 of the bias) beside one tile of stride ``SE = (A + 8) | 1``:
    ``P + T + 128 + 32 w ((n_hidden + 2) S + SE)`` floats of the 40 960, ``w = 4``, else 2, else 1.  ANM6 (``D = 18``, ``A = 6``)
    with ``(64, 64)`` takes 37 645 floats at ``w = 2``; ``(32,)`` runs at ``w = 4``, ``(128,)`` at ``w = 2``, ``(256,)`` at ``w = 1``;
    ``(32, 96, 32)`` (42 669 floats at ``w = 1``: five tiles of stride 97), ``(64, 64, 64)`` and ``(96, 96)`` are refused -- ``act``
    serves them, their gradient stays ``evaluate`` and autograd.
    (:func:`grad_lds_floats`)
    All outputs are float32.  Not served: what ``policy.py`` rule 8 excludes; the optimiser and gradient-norm clipping (torch's,
    on the one flat tensor); accumulation across minibatches; KL early stopping (``stats`` makes it possible on the host).
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import errors as E
from . import policy as PL
from .policy import fma32_v

STATS = 8
ST_PG, ST_V, ST_KL, ST_CLIP, ST_N = 0, 1, 2, 3, 4
STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "approx_kl", "clip_frac", "n", "reserved")
MAX_PARTIALS = 512
MAX_B = 1 << 24
ENT_CONST = np.float32(0.5 + 0.5 * math.log(2.0 * math.pi))
MB_FIELDS = ("obs", "actions", "logp", "values", "returns", "adv", "weight")
_F32 = np.float32


# ---- the specification ---------------------------------------------------------------------------------------------------------
def rows_per_partial(B):
    """Rule 11."""
    R = 32
    while -(-int(B) // R) > MAX_PARTIALS:
        R *= 2
    return R


def inv_std_of(log_std):
    """Rule 2."""
    with np.errstate(all="ignore"):
        return np.exp(-np.asarray(log_std, dtype=np.float32).astype(np.float64)).astype(np.float32)


def ratio_of(lr):
    """Rule 4."""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(lr, dtype=np.float32).astype(np.float64)).astype(np.float32)


def _field(mb, name):
    return np.asarray(mb[name] if isinstance(mb, dict) else getattr(mb, name))


def _padded(mb):
    """Rule 1: ``(B, B', live, w, x0)``."""
    w = _field(mb, "weight").astype(np.float32)
    B = w.shape[0]
    Bp = -(-B // 32) * 32
    w = np.concatenate([w, np.zeros(Bp - B, dtype=np.float32)])
    live = w != 0
    obs = _field(mb, "obs")
    x0 = np.zeros((Bp, obs.shape[1]), dtype=np.float32)
    with np.errstate(all="ignore"):
        x0[:B][live[:B]] = obs[live[:B]].astype(np.float32)
    return B, Bp, live, w, x0


def _rows(mb, name, B, Bp, live):
    """a per-row field as float32 ``[B']``, ``+0`` on dead rows (which are not read)"""
    v = _field(mb, name)
    out = np.zeros((Bp,) + v.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        out[:B][live[:B]] = v[live[:B]].astype(np.float32)
    return out


def _forward(layers, x0, activation):
    acts = [x0]
    for i, (W, b) in enumerate(layers):
        acts.append(PL.layer(acts[-1], W, b, activation if i + 1 < len(layers) else None))
    return acts


def _logp(params, mb, inv_std, activation, pad):
    B, Bp, live, w, x0 = pad
    acts = _forward(params["actor"], x0, activation)
    ls = np.asarray(params["log_std"], dtype=np.float32)
    a = _rows(mb, "actions", B, Bp, live)
    with np.errstate(all="ignore"):
        z = ((a - acts[-1]) * np.asarray(inv_std, dtype=np.float32)[None, :]).astype(np.float32)
        acc = np.full(Bp, PL.logp_const(ls.shape[0]), dtype=np.float32)
        for j in range(ls.shape[0]):
            acc = fma32_v(_F32(-0.5) * z[:, j], z[:, j], acc)
            acc = (acc - ls[j]).astype(np.float32)
        lr = (acc - _rows(mb, "logp", B, Bp, live)).astype(np.float32)
    return acts, z, acc, lr


def log_ratio(params, mb, inv_std, activation="tanh"):
    """Rule 3: ``lr [B]`` (``+0`` on dead rows)."""
    pad = _padded(mb)
    lr = _logp(params, mb, inv_std, activation, pad)[3]
    return np.where(pad[2], lr, _F32(0))[:pad[0]].astype(np.float32)


def chain_rows(x, dy, R):
    """Rule 8: ``[G, K', N]`` from ``x [B', K']`` and ``dy [B', N]``."""
    Bp = x.shape[0]
    G = -(-Bp // R)
    acc = np.zeros((G, x.shape[1], dy.shape[1]), dtype=np.float32)
    for i in range(min(R, Bp)):
        rows = np.arange(G) * R + i
        sel = rows < Bp
        acc[sel] = fma32_v(x[rows[sel]][:, :, None], dy[rows[sel]][:, None, :], acc[sel])
    return acc


def _net_backward(part, entries, layers, acts, dy, activation, R):
    """Rules 8 and 9 for one net; ``entries``: the weight offsets of its layers"""
    for i in range(len(layers) - 1, -1, -1):
        W = np.asarray(layers[i][0], dtype=np.float32)
        K, N = W.shape
        x = np.concatenate([acts[i], np.ones((acts[i].shape[0], 1), dtype=np.float32)], axis=1)
        part[:, entries[i]:entries[i] + (K + 1) * N] = chain_rows(x, dy, R).reshape(part.shape[0], -1)
        if i == 0:
            break
        acc = np.zeros((dy.shape[0], K), dtype=np.float32)
        for n in range(N):
            acc = fma32_v(dy[:, n, None], W[None, :, n], acc)
        if N & 1:
            acc = fma32_v(_F32(0), _F32(0), acc)
        y = acts[i]
        with np.errstate(all="ignore"):
            if activation == "tanh":
                dy = (acc * fma32_v(-y, y, _F32(1))).astype(np.float32)
            else:
                dy = np.where(y > 0, acc, _F32(0)).astype(np.float32)


def reduce_partials(part, log_std, P, vf_coef, ent_coef):
    """Rule 10: ``(grad [P], stats [8])``."""
    ls = np.asarray(log_std, dtype=np.float32)
    A = ls.shape[0]
    vf_coef, ent_coef = _F32(vf_coef), _F32(ent_coef)
    with np.errstate(all="ignore"):
        S = np.zeros(P + STATS, dtype=np.float32)
        for g in range(part.shape[0]):
            S = (S + part[g]).astype(np.float32)
        nf = S[P + ST_N]
        grad, stats = np.zeros(P, dtype=np.float32), np.zeros(STATS, dtype=np.float32)
        if nf != 0:
            grad = (S[:P] / nf).astype(np.float32)
            grad[P - A:] = (grad[P - A:] - ent_coef).astype(np.float32)
            H = _F32(0)
            for j in range(A):
                H = _F32(H + _F32(ls[j] + ENT_CONST))
            pg, v = _F32(S[P + ST_PG] / nf), _F32(S[P + ST_V] / nf)
            loss = fma32_v(-ent_coef, H, fma32_v(vf_coef, v, pg))
            stats[:] = (loss, pg, v, H, _F32(S[P + ST_KL] / nf), _F32(S[P + ST_CLIP] / nf), nf, 0)
    return grad, stats


def backward(params, mb, ratio, inv_std, activation="tanh", clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None, R=None):
    """Rules 1, 3 and 5 to 10 from the ``ratio [B]`` and ``inv_std [A]`` of rules 4 and 2: a dict ``grad [P]``, ``stats [8]``, ``logp [B]``,
    ``values [B]`` (all float32) and ``partials [G, P + 8]``.  ``params`` is what ``policy.unpack`` returns, ``mb`` a dict or an object
    with the fields of a ``Minibatch``."""
    pad = _padded(mb)
    B, Bp, live, w, x0 = pad
    R = rows_per_partial(B) if R is None else int(R)
    if R < 32 or R % 32:
        raise E.ArgsError("R is %r but should be a positive multiple of 32" % (R,))
    D, A = x0.shape[1], np.asarray(params["log_std"]).shape[0]
    hidden = tuple(int(np.asarray(Wb[0]).shape[1]) for Wb in params["actor"][:-1])
    entries, P = PL.layout(D, A, hidden)
    at = {net: [o for n_, i, kind, o, s in entries if n_ == net and kind == "weight"] for net in ("actor", "critic")}
    G = -(-Bp // R)
    part = np.zeros((G, P + STATS), dtype=np.float32)
    clip, vf_coef = _F32(clip), _F32(vf_coef)
    lo, hi = _F32(_F32(1) - clip), _F32(_F32(1) + clip)
    zero = _F32(0)
    extra = np.zeros((Bp, A + STATS), dtype=np.float32)
    with np.errstate(all="ignore"):
        # the critic: rule 6
        acts = _forward(params["critic"], x0, activation)
        v, ret = acts[-1][:, 0], _rows(mb, "returns", B, Bp, live)
        d = (v - ret).astype(np.float32)
        big, gr = (d * d).astype(np.float32), d
        if vf_clip is not None:
            vc = _F32(vf_clip)
            vo = _rows(mb, "values", B, Bp, live)
            dv = (v - vo).astype(np.float32)
            active = (dv < -vc) | (dv > vc)
            dc = np.where(dv < -vc, -vc, np.where(dv > vc, vc, dv)).astype(np.float32)
            d2 = ((vo + dc).astype(np.float32) - ret).astype(np.float32)
            e2 = (d2 * d2).astype(np.float32)
            gr = np.where(e2 > big, np.where(active, zero, d2), gr).astype(np.float32)
            big = np.where(e2 > big, e2, big).astype(np.float32)
        dyv = np.where(live, ((w * vf_coef).astype(np.float32) * gr).astype(np.float32), zero).astype(np.float32)
        extra[:, A + ST_V] = np.where(live, (w * (_F32(0.5) * big).astype(np.float32)).astype(np.float32), zero)
        extra[:, A + ST_N] = live
        values = np.where(live, v, zero).astype(np.float32)
        _net_backward(part, at["critic"], params["critic"], acts, dyv[:, None], activation, R)
        # the actor: rules 3 and 5
        acts, z, logp, lr = _logp(params, mb, inv_std, activation, pad)
        ist = np.asarray(inv_std, dtype=np.float32)
        rt = np.zeros(Bp, dtype=np.float32)
        rt[:B] = np.asarray(ratio, dtype=np.float32)
        adv = _rows(mb, "adv", B, Bp, live)
        s1 = (rt * adv).astype(np.float32)
        rc = np.where(rt < lo, lo, np.where(rt > hi, hi, rt)).astype(np.float32)
        s2 = (rc * adv).astype(np.float32)
        pg = -np.where(s2 < s1, s2, s1).astype(np.float32)
        clipped = np.where(adv >= 0, rt > hi, (adv < 0) & (rt < lo))
        cl = np.where(live, (w * np.where(clipped, zero, -s1).astype(np.float32)).astype(np.float32), zero).astype(np.float32)
        lv = live[:, None]
        dy = np.where(lv, (cl[:, None] * (z * ist[None, :]).astype(np.float32)).astype(np.float32), zero).astype(np.float32)
        extra[:, :A] = np.where(lv, (cl[:, None] * fma32_v(z, z, _F32(-1))).astype(np.float32), zero)
        extra[:, A + ST_PG] = np.where(live, (w * pg).astype(np.float32), zero)
        extra[:, A + ST_KL] = np.where(live, (w * ((rt - _F32(1)).astype(np.float32) - lr).astype(np.float32)).astype(np.float32), zero)
        extra[:, A + ST_CLIP] = np.where(live & ((rt > hi) | (rt < lo)), _F32(1), zero)
        _net_backward(part, at["actor"], params["actor"], acts, dy, activation, R)
        part[:, P - A:] = chain_rows(np.ones((Bp, 1), dtype=np.float32), extra, R)[:, 0, :]
    grad, stats = reduce_partials(part, params["log_std"], P, vf_coef, ent_coef)
    return dict(grad=grad, stats=stats, logp=np.where(live, logp, zero)[:B].astype(np.float32), values=values[:B], partials=part)


def grad_lds_floats(D, A, hidden, waves=1):
    """Rule 12: the floats of the backward kernel's LDS plan with ``waves`` wavefronts per workgroup."""
    hidden = [int(h) for h in hidden]
    P = PL.layout(D, A, hidden)[1]
    T = 0
    for n_out in (int(A), 1):
        widths = hidden + [n_out]
        for i in range(1, len(widths)):
            T += ((widths[i] + 1) & ~1) * widths[i - 1]
    S = (max(int(D), max(hidden), int(A)) + 1) | 1
    SE = (int(A) + STATS) | 1
    return P + T + 128 + 32 * int(waves) * ((len(hidden) + 2) * S + SE)


def _number(x, what, positive=False):
    try:
        if isinstance(x, bool):
            raise TypeError
        v = float(x)
    except (TypeError, ValueError):
        v = np.nan
    if not np.isfinite(v) or not np.isfinite(np.float32(v)) or (positive and not v > 0):
        raise E.ArgsError("The argument %s is %r but should be a %sfinite number." % (what, x, "positive " if positive else ""))
    return v


def check_args(D, A, hidden, batch_size, clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None):
    """``(B, clip, vf_coef, ent_coef, vf_clip or None)``; what needs no device to refuse raises ``ArgsError``."""
    D, A, hidden = PL.check_args(D, A, hidden)[:3]
    B = PL._index(batch_size, "batch_size", 1, MAX_B)
    clip = _number(clip, "clip", positive=True)
    vf_coef, ent_coef = _number(vf_coef, "vf_coef"), _number(ent_coef, "ent_coef")
    if vf_clip is not None:
        vf_clip = _number(vf_clip, "vf_clip")
        if vf_clip < 0:
            raise E.ArgsError("The argument vf_clip is %r but should be None (off) or a non-negative number." % (vf_clip,))
    need = grad_lds_floats(D, A, hidden)
    if need > PL.LDS_FLOATS:
        raise E.ArgsError("A network of D = %d, hidden = %r, A = %d takes %d floats of LDS for the backward pass but the kernel's "
                          "plan has %d (policy_grad.py rule 12)." % (D, hidden, A, need, PL.LDS_FLOATS))
    return B, clip, vf_coef, ent_coef, vf_clip


# ---- the device half -------------------------------------------------------------------------------------------------------------
class PPOGradient:
    """``g = pi.ppo_gradient(batch_size, clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None)``; every tensor allocated once here::

        opt = torch.optim.Adam([pi.flat], lr=3e-4)
        for ep in range(K):
            for m in range(sampler.n_minibatches):
                g(sampler.gather(m, ep))                     # two launches: pi.flat.grad and g.stats are overwritten
                opt.step()                                   # no zero_grad, no backward

    ``g(mb)`` takes a ``Minibatch`` (or any object with its fields) of ``batch_size`` rows, allocates nothing, does not synchronise
    and can be captured into a graph.  ``stats [8]`` holds ``STAT_NAMES``; ``ratio``, ``logp``, ``values`` ``[B]`` and ``inv_std [A]`` are what
    the call computed (float32)."""

    def __init__(self, pi, batch_size, clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None):
        from . import _lib

        torch = pi._torch
        B, clip, vf_coef, ent_coef, vf_clip = check_args(pi.obs_dim, pi.action_dim, pi.hidden, batch_size, clip, vf_coef, ent_coef,
                                                         vf_clip)
        lib = pi._backend.lib
        if not hasattr(lib, "anm_policy_ppo_grad"):
            raise E.EnvInitializationError("PPOGradient needs the GPU library (policy_grad.py rule 12)")
        self.pi, self.batch_size = pi, B
        self.clip, self.vf_coef, self.ent_coef, self.vf_clip = clip, vf_coef, ent_coef, vf_clip
        self.rows_per_partial = rows_per_partial(B)
        P, A = pi.n_params, pi.action_dim
        f32 = dict(dtype=torch.float32, device=pi.device)
        self.partials = torch.zeros(-(-B // self.rows_per_partial) * (P + STATS), **f32)
        self.ratio, self.logp, self.values = torch.zeros(B, **f32), torch.zeros(B, **f32), torch.zeros(B, **f32)
        self.inv_std, self.stats = torch.zeros(A, **f32), torch.zeros(STATS, **f32)
        if pi.flat.grad is None:
            pi.flat.grad = torch.zeros(P, **f32)
        self._struct = _lib.Ppo(
            partials=self.partials.data_ptr(), ratio=self.ratio.data_ptr(), logp=self.logp.data_ptr(), values=self.values.data_ptr(),
            inv_std=self.inv_std.data_ptr(), stats=self.stats.data_ptr(), B=B, rows_per_partial=self.rows_per_partial,
            io_dtype=pi._code[pi.io_dtype], value_dtype=pi._code[pi.io_dtype], clip=clip, vf_coef=vf_coef, ent_coef=ent_coef,
            vf_clip=-1.0 if vf_clip is None else vf_clip)
        self._ref = C.byref(self._struct)
        self._lib, self._torch = lib, torch

    def __call__(self, mb):
        t, pi, B = self._torch, self.pi, self.batch_size
        s = self._struct
        s.obs = pi._tensor(mb.obs, (B, pi.obs_dim), "mb.obs", (pi.io_dtype,))
        s.actions = pi._tensor(mb.actions, (B, pi.action_dim), "mb.actions", (pi.io_dtype,))
        vdt = mb.weight.dtype if isinstance(mb.weight, t.Tensor) else None
        for name, field in (("weight", "weight"), ("logp", "logp_old"), ("values", "values_old"), ("returns", "returns"),
                            ("adv", "adv")):
            dtypes = (t.float32, t.float64) if name == "weight" else (vdt,)
            setattr(s, field, pi._tensor(getattr(mb, name), (B,), "mb." + name, dtypes))
        s.value_dtype = pi._code[vdt]
        grad = pi.flat.grad
        if grad is None:
            raise E.ArgsError("pi.flat.grad is None: PPOGradient writes into it (construction allocates it; set_to_none removed it)")
        s.grad = pi._tensor(grad, (pi.n_params,), "pi.flat.grad", (t.float32,))
        if pi.flat.data_ptr() != pi._struct.params:            # (a caller that re-assigned flat.data: follow it, as _launch does)
            pi._struct.params = pi.flat.data_ptr()
            pi._bind_views()
        rc = self._lib.anm_policy_ppo_grad(pi._ref, self._ref, pi._stream())
        if rc != 0:
            pi._backend.check(rc, "anm_policy_ppo_grad")

    def stats_dict(self):
        """The statistics of the last call by name (one small copy to the host)."""
        return dict(zip(STAT_NAMES[:7], (float(x) for x in self.stats.tolist()[:7])))
