"""Affine policy-facing I/O (``BatchedANMEnv(action_map=, obs_map=, reward_scale=)``; ``anm_model_set_io_map`` in the C ABI):
the specification the kernels follow (csrc/anm_env_ops.hpp: ``IoMap``, ``EnvIO::iomap``, the ``MAP`` instantiations of the
coalesced-row step; the lane-group kernels carry a mapped instance of their output sections).  Like ``io_dtype.py``, ``rng.py``
and ``episode.py`` this text is normative: the kernels are tested against it bit for bit.

A learned policy emits values in ``[-1, 1]``, wants observations of one magnitude and rewards of order one; the environment
speaks MW, MVAr, p.u. and a time index.  The mode moves the three fixed affine maps between them into the step kernels.  It
changes what is stored in ``action``, ``obs`` and ``reward`` and nothing else: *the mapped mode is the plain mode plus the
maps below on three arrays, bit for bit*.  All constants are given at construction; there are no running statistics, no
reduction over environments and no new state (io_norm.py adds those, outside the step kernels).

1. Action.  Tables ``mid[j]``, ``half[j]``, ``lo[j]``, ``hi[j]`` (float64, ``j < action_dim``; ``half`` finite and > 0,
   ``lo <= hi``).  The kernel reads ``u`` (under ``io_dtype=float32`` it widens ``u`` first, which is exact), forms
   ``x = fma(half[j], u, mid[j])`` -- one rounding -- and ``a = lo[j] if x < lo[j] else (hi[j] if x > hi[j] else x)``.  This
   select form is part of the specification: a NaN fails both comparisons and passes through, as it would in the plain mode.
   From there on the step is the plain-mode step fed ``a`` (:func:`map_action`).
2. Observation.  Tables ``scale[k] > 0`` and ``bias[k]`` (float64, finite, ``k < obs_dim``).  Let ``o`` be the double the plain
   mode would have stored: after the clip, in the ``"state"`` form or the list form gathered in the kernel, the zero row of a
   terminated environment and the rows an in-kernel autoreset writes included.  The kernel stores ``fma(o, scale[k], bias[k])``
   -- one rounding; under float32 I/O that double is then rounded once to float (io_dtype.py rule 2).  A zero row therefore
   stores ``bias`` (:func:`map_obs`; a bias of ``-0.0`` stores ``+0.0``, IEEE's sum of the two zeros -- :func:`box_obs_map`
   never produces one).
3. Reward.  The kernel stores ``r * reward_scale`` (``reward_scale`` finite and > 0) -- one rounding -- then the float32
   rounding if float32 I/O is on (:func:`map_reward`).
4. What stays raw.  ``state``, ``soc``, ``e_loss``, ``penalty``, ``terminated``, ``truncated``, ``timestep``, ``reset_count``,
   ``nr_iters``, ``exo_z`` and ``exo_forecast`` -- the forecast stays in MW: it is not scaled -- and every episode statistic,
   which accumulates the raw float64 reward.  All of these are bit-identical to the plain mode fed ``a``.
5. Spaces.  ``observation_space`` is the ``Box`` of images ``fma(low, scale, bias)``, ``fma(high, scale, bias)``: the map is
   monotone for ``scale > 0`` (rounding is monotone), so a clipped observation lies inside it; an infinite end stays infinite.
   Under float32 the bounds are rounded to nearest, as in rule 4 of io_dtype.py.  With ``action_map`` set, ``action_space`` is
   ``Box(-1, 1)`` in ``io_dtype``, ``raw_action_space`` keeps the MW ``Box`` and ``check_actions`` compares against
   ``[-1, 1]``.
6. ``reset()`` returns mapped observations.  The reset kernel writes the mapped ``"state"`` form itself; the list form at
   reset is gathered unmapped and mapped on the host side of the launch, with the same expression (io_dtype.py rule 5:
   ``reset()`` is not the hot path).
7. Both rows are always written, as in float32 mode: ``obs`` is no copy of ``state`` (``anm_model_bind_state_same`` is not used).
8. A part that is not given is not mapped.  (In the kernels its tables hold the exact identity -- ``half = 1, mid = -0.0``,
   infinite ends; ``scale = 1, bias = -0.0``; ``reward_scale = 1`` -- and ``fma(1, u, -0.0) == u``, ``u * 1 == u`` for every
   ``u``, signed zeros included.)

Not served (refused, not ignored): a backend other than the GPU library, parameter classes (``variants=``), batch views and
``MixedBatchedANMEnv``, a list-form observation that is not gathered inside the step kernel, ``track_full`` without such a
list, a callable observation, and ``action_map="unit"`` on a ``Box`` with an infinite end.  Running mean and variance are
not part of this mode: ``obs_norm="running"`` / ``reward_norm="running"`` (io_norm.py) rewrite ``scale``, ``bias`` and
``reward_scale`` of this map on the device between steps, and the kernels below map through whatever the tables hold.
"""

from __future__ import annotations

import numpy as np

from . import errors as E
from . import rng as _rng


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _fma(a, b, c):
    """``fma(a, b, c)`` over arrays with one rounding (``rng.fma_v``); an element with a non-finite argument takes IEEE's
    special-value result, which ``a * b + c`` gives without any rounding to get wrong."""
    a, b, c = np.broadcast_arrays(_f64(a), _f64(b), _f64(c))
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    with np.errstate(all="ignore"):
        out = a * b + c
    if fin.any():
        out = out.copy()
        out[fin] = _rng.fma_v(a[fin], b[fin], c[fin])
    return out


def unit_action_map(low, high):
    """``(mid, half)`` that take ``[-1, 1]`` onto the ``Box`` ``[low, high]``: ``mid = 0.5 * low + 0.5 * high`` and
    ``half = 0.5 * high - 0.5 * low``, as written.  Non-finite ends, ``low > high`` and a degenerate entry (``half`` not > 0)
    raise ``ArgsError``."""
    low, high = _f64(low), _f64(high)
    if low.shape != high.shape or not (np.isfinite(low).all() and np.isfinite(high).all()):
        raise E.ArgsError('action_map="unit" needs an action Box with finite ends')
    mid = 0.5 * low + 0.5 * high
    half = 0.5 * high - 0.5 * low
    if not (half > 0).all():
        raise E.ArgsError('action_map="unit" needs an action Box with low < high in every entry')
    return mid, half


def box_obs_map(low, high):
    """``(scale, bias)`` that take every column of the observation ``Box`` with finite ``low < high`` onto about ``[-1, 1]``:
    ``scale = 2 / (high - low)``, ``bias = -(high + low) / (high - low)``, as written.  Every other column -- an infinite end, a
    degenerate or an overflowing one -- is the identity ``(1, 0)``."""
    low, high = _f64(low), _f64(high)
    with np.errstate(all="ignore"):
        span = high - low
        scale = 2.0 / span
        bias = -(high + low) / span + 0.0   # (+ 0.0: a symmetric column gets +0.0, not -0.0 -- see rule 2 on zero rows)
        ok = np.isfinite(low) & np.isfinite(high) & (low < high) & np.isfinite(scale) & (scale > 0) & np.isfinite(bias)
    return np.where(ok, scale, 1.0), np.where(ok, bias, 0.0)


def check_action_map(mid, half, low, high):
    """The action tables as float64 vectors of one length; what the library would refuse raises ``ArgsError`` here."""
    mid, half, low, high = _f64(mid), _f64(half), _f64(low), _f64(high)
    if not (mid.ndim == 1 and mid.shape == half.shape == low.shape == high.shape):
        raise E.ArgsError("action_map: mid and half must have action_dim = %d entries each" % low.shape[0])
    if not (np.isfinite(half).all() and (half > 0).all() and np.isfinite(mid).all()):
        raise E.ArgsError("action_map: mid must be finite and half finite and > 0")
    if not (low <= high).all():
        raise E.ArgsError("action_map: the action Box has low > high")
    return mid, half, low, high


def check_obs_map(scale, bias, n):
    scale, bias = _f64(scale), _f64(bias)
    if scale.shape != (n,) or bias.shape != (n,):
        raise E.ArgsError("obs_map: scale and bias must have %d entries each (one per observation entry)" % n)
    if not (np.isfinite(scale).all() and (scale > 0).all() and np.isfinite(bias).all()):
        raise E.ArgsError("obs_map: scale must be finite and > 0 and bias finite")
    return scale, bias


def check_reward_scale(reward_scale):
    try:
        r = float(reward_scale)
    except (TypeError, ValueError):
        r = np.nan
    if not (np.isfinite(r) and r > 0):
        raise E.ArgsError("The argument reward_scale is %r but should be a finite number > 0." % (reward_scale,))
    return r


def map_action(u, mid, half, low, high):
    """Rule 1, exactly: ``x = fma(half, u, mid)``; ``low`` where ``x < low``, ``high`` where ``x > high``, else ``x`` (NaN
    passes).  ``u``: ``[..., action_dim]``, float64 or float32 (widened)."""
    u = np.asarray(u).astype(np.float64)
    x = _fma(_f64(half), u, _f64(mid))
    low, high = np.broadcast_to(_f64(low), x.shape), np.broadcast_to(_f64(high), x.shape)
    with np.errstate(invalid="ignore"):
        return np.where(x < low, low, np.where(x > high, high, x))


def map_obs(o, scale, bias):
    """Rule 2, exactly: ``fma(o, scale, bias)`` of the float64 rows the plain mode stores (before any float32 rounding)."""
    return _fma(_f64(o), _f64(scale), _f64(bias))


def map_reward(r, reward_scale):
    """Rule 3: ``r * reward_scale``, one rounding."""
    return _f64(r) * np.float64(reward_scale)


def encode_action(a_mw, mid, half):
    """``(a_mw - mid) / half``, as written: the ``u`` to feed a mapped environment for an action in MW / MVAr (an
    ``MPCAgent``'s, say).  Two roundings, and the kernel's ``fma`` is a third: ``map_action(encode_action(a))`` is close to
    ``a`` but NOT bit-exact -- compare trajectories of such a pair with a tolerance, never bit for bit."""
    if hasattr(a_mw, "new_tensor"):   # a torch tensor: stays on its device
        return (a_mw - a_mw.new_tensor(_f64(mid))) / a_mw.new_tensor(_f64(half))
    return (_f64(a_mw) - _f64(mid)) / _f64(half)


def observation_image(low, high, scale, bias):
    """Rule 5: the bounds of the mapped observation ``Box`` (float64)."""
    return _fma(_f64(low), _f64(scale), _f64(bias)), _fma(_f64(high), _f64(scale), _f64(bias))
