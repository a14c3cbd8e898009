"""Running observation and return normalisation kept on the device (``BatchedANMEnv(obs_norm="running",
reward_norm="running")``; ``anm_model_io_norm_update`` in the C ABI): the specification the kernels of csrc/anm_io_norm.hpp
follow.  Like ``io_affine.py``, ``episode.py`` and ``rng.py`` this text is normative: the kernels are tested against it bit
for bit.

This is Gymnasium's ``NormalizeObservation`` / ``NormalizeReward`` (SB3's ``VecNormalize`` without the clipping) moved behind
the affine I/O map of ``io_affine.py``: the step kernels keep writing ``fma(o, scale, bias)`` and ``r * reward_scale``, and a
small reduction rewrites ``scale``, ``bias`` and ``reward_scale`` on the stream between steps.  No step kernel changes, nothing
allocates, nothing synchronises with the host, and the statistics have the same bits on every run.

Every product that feeds a sum is an explicit fma (``rng.fma_v`` here, ``fma()`` in the kernel); every other operation is
one IEEE double operation (``+ - * / sqrt``).

State.  Observation statistics ``cnt``, ``mean[D]``, ``var[D]`` (``D = obs_dim``), return statistics ``rcnt``, ``rmean``,
``rvar``, all float64; per environment ``G[e]`` (float64, the discounted-return accumulator) and ``t_seen[e]`` (int32); two
counters ``n_updates`` and ``n_skipped``.  Start (Gymnasium's ``RunningMeanStd``): ``cnt = rcnt = 1e-4``, means 0, variances
1, ``G = 0``, ``t_seen = 0``.

1. Tables from statistics.  ``scale[k] = 1 / sqrt(var[k] + eps)``, ``bias[k] = 0.0 - mean[k] * scale[k]`` (never ``-0.0``),
   ``reward_scale = 1 / sqrt(rvar + eps)``; ``eps`` defaults to 1e-8.  At construction the map holds the tables of the
   initial statistics.
2. When.  An update runs after a ``step()`` call and reads what that call stored, so the step at time t is mapped with the
   statistics through step t-1.  THIS LAG OF ONE STEP IS THE DIFFERENCE FROM GYMNASIUM, which updates first and normalises the
   same observation with the result; it is what lets ``step()`` keep writing through the map.  ``reset()`` does not update;
   it zeroes ``G`` and ``t_seen`` of the rows it re-initialises.
3. Observation leaves.  Row ``e`` counts iff ``terminated[e] == 0`` after the call (a terminated row stores ``bias``, not
   data).  ``y`` is the stored ``obs`` entry, widened when float32 (exact).  The leaves of a counted row are ``y + 0.0`` and
   ``y * y``, those of any other row ``+0.0`` and ``+0.0``.  (``+ 0.0``: a leaf is never ``-0.0``, so a column of ``-0.0`` --
   the reactive power of a load with a zero ratio -- sums to ``+0.0`` whatever the padding.)  ``n`` is the number of counted
   rows, exact.
4. The sum is one fixed tree: the leaves padded by ``+0.0`` to the next power of two over the environment index, then level
   by level node ``i`` = node ``2i`` + node ``2i+1``; ``S1[k]``, ``S2[k]`` are the roots (:func:`tree_sum`).  IEEE addition
   commutes, so butterflies over lanes, an LDS stage over wavefronts and a second launch over workgroups of aligned
   power-of-two row ranges reproduce it exactly: the result does not depend on the grid.  No float atomics.
5. Batch moments in the stored space, then back to raw.  With ``s``, ``b`` the tables the step used: ``my = S1 / n``,
   ``q = S2 / n``, ``t = fma(-my, my, q)``, ``vy = 0.0 if t < 0.0 else t`` (a NaN passes), ``mo = (my - b) / s``,
   ``vo = vy / (s * s)``.  (The stored space is the normalised one once the map has settled: ``q - my^2`` stays well
   conditioned, and the list form, float32 and autoreset rows need no raw copy of ``obs``.)  ``n == 0``: the observation part
   changes nothing.  A column whose ``mo`` or ``vo`` is not finite is skipped: its statistics and tables stay and
   ``n_skipped += 1``.
6. Merge (Chan et al., Gymnasium's ``update_mean_var_count_from_moments``).  ``tot = cnt + n``, ``w = n / tot``,
   ``d = mo - mean``, ``mean' = fma(d, w, mean)``, ``M2 = fma(d * d, cnt * w, fma(var, cnt, vo * n))``, ``var' = M2 / tot``;
   after all columns ``cnt = tot``; then rule 1.
7. Return accumulator, per row, ``rs`` the ``reward_scale`` the step used.  ``timestep[e] == t_seen[e]``: untouched, not
   counted (an absorbing no-op, a failed reset draw).  Else ``timestep[e] == 0``: ``G = 0``, ``t_seen = 0``, not counted (an
   in-kernel autoreset).  Else ``r = reward_stored / rs``, ``G = fma(gamma, G, r)``, the row is counted with the leaves
   ``G + 0.0`` and ``G * G``, then ``G = 0`` if ``terminated[e]`` or ``truncated[e]``, then ``t_seen = timestep[e]``.  The tree
   of rule 4, the moments of rule 5 without the conversion (they are raw already), the merge of rule 6 into ``rcnt``,
   ``rmean``, ``rvar`` (moments that are not finite: skipped, ``n_skipped += 1``), then rule 1.
8. ``obs_norm`` and ``reward_norm`` are independent: a part that is off keeps its identity table and is never touched.
   Every update call counts in ``n_updates``.

Not served, as in ``io_affine.py``: a backend other than the GPU library, parameter classes, batch views and
``MixedBatchedANMEnv``, a list-form observation that is not gathered inside the step kernel, a callable observation.
Sharded runs keep statistics per rank (no cross-rank merge); normalised values are not clipped.
"""

from __future__ import annotations

import numpy as np

from . import errors as E
from .io_affine import _fma

EPS_DEFAULT = 1e-8
COUNT0 = 1e-4
SMALL_BATCH = 262144    # rows of one slab of k_norm_partial (csrc/anm_io_norm.hpp): 256 up to here, 1024 above
STATS_HEAD = 8          # the device statistics block: cnt, rcnt, rmean, rvar, reward_scale, 3 unused | mean | var | scale | bias


def check_norm_args(obs_norm, reward_norm, norm_eps, obs_map=None, reward_scale=None):
    """``(obs_on, reward_on, eps)``; what needs no device to refuse raises ``ArgsError``."""
    for name, val in (("obs_norm", obs_norm), ("reward_norm", reward_norm)):
        if val is not None and not (isinstance(val, str) and val == "running"):
            raise E.ArgsError('The argument %s is %r but should be None or "running".' % (name, val))
    if obs_norm is not None and obs_map is not None:
        raise E.ArgsError("obs_norm and obs_map do not go together: both own the observation tables of the map")
    if reward_norm is not None and reward_scale is not None:
        raise E.ArgsError("reward_norm and reward_scale do not go together: both own the reward scale of the map")
    try:
        eps = float(norm_eps)
    except (TypeError, ValueError):
        eps = np.nan
    if not (np.isfinite(eps) and eps > 0):
        raise E.ArgsError("The argument norm_eps is %r but should be a finite number > 0." % (norm_eps,))
    return obs_norm is not None, reward_norm is not None, eps


def rows_per_group(num_envs):
    return 256 if int(num_envs) <= SMALL_BATCH else 1024


def slab_doubles(num_envs, obs_dim):
    """Length of the slab buffer: one slab ``[n, nr, SG1, SG2 | S1[D] | S2[D]]`` per group of rows."""
    return -(-int(num_envs) // rows_per_group(num_envs)) * (4 + 2 * int(obs_dim))


def initial_state(num_envs, obs_dim):
    return dict(cnt=COUNT0, mean=np.zeros(obs_dim), var=np.ones(obs_dim), rcnt=COUNT0, rmean=0.0, rvar=1.0,
                G=np.zeros(num_envs), t_seen=np.zeros(num_envs, dtype=np.int32), n_updates=0, n_skipped=0)


def tables(mean, var, eps=EPS_DEFAULT):
    """Rule 1: ``(scale, bias)``."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        scale = 1.0 / np.sqrt(var + eps)
        return scale, 0.0 - mean * scale


def reward_scale(rvar, eps=EPS_DEFAULT):
    return float(1.0 / np.sqrt(np.float64(rvar) + eps))


def tree_sum(leaves):
    """Rule 4 over axis 0 of ``leaves`` (``[n, ...]``, n >= 1)."""
    x = np.asarray(leaves, dtype=np.float64)
    n = x.shape[0]
    p = 1
    while p < n:
        p *= 2
    buf = np.zeros((p,) + x.shape[1:])
    buf[:n] = x
    with np.errstate(all="ignore"):
        while buf.shape[0] > 1:
            buf = buf[0::2] + buf[1::2]
    return buf[0]


def batch_moments(s1, s2, n):
    """``(my, vy)`` of rule 5 from the roots."""
    with np.errstate(all="ignore"):
        my, q = np.asarray(s1, dtype=np.float64) / n, np.asarray(s2, dtype=np.float64) / n
        t = _fma(-my, my, q)
        return my, np.where(t < 0.0, 0.0, t)


def merge(mean, var, cnt, mo, vo, n):
    """Rule 6 on arrays: ``(mean', var', ok)``; where ``ok`` is False (moments not finite) the old values come back."""
    mean, var, mo, vo = (np.asarray(x, dtype=np.float64) for x in (mean, var, mo, vo))
    ok = np.isfinite(mo) & np.isfinite(vo)
    mo_, vo_ = np.where(ok, mo, 0.0), np.where(ok, vo, 0.0)
    with np.errstate(all="ignore"):
        tot = cnt + np.float64(n)
        w = np.float64(n) / tot
        d = mo_ - mean
        m2 = _fma(d * d, cnt * w, _fma(var, cnt, vo_ * np.float64(n)))
        return np.where(ok, _fma(d, w, mean), mean), np.where(ok, m2 / tot, var), ok


def update(st, obs, reward, terminated, truncated, timestep, obs_tables, rs, gamma, eps=EPS_DEFAULT, obs_on=True,
           reward_on=True):
    """One update (rules 3-8) of the state dict ``st`` in place from what a step stored.  ``obs_tables = (scale, bias)`` and
    ``rs``: the tables that step used.  Returns the new ``(scale, bias, reward_scale)``."""
    obs = np.asarray(obs)
    term = np.asarray(terminated).astype(bool)
    trunc = np.zeros_like(term) if truncated is None else np.asarray(truncated).astype(bool)
    ts = np.asarray(timestep).astype(np.int32)
    scale, bias = (np.array(x, dtype=np.float64) for x in obs_tables)
    rs = float(rs)
    st["n_updates"] += 1
    with np.errstate(all="ignore"):
        if obs_on:
            y = obs.astype(np.float64)
            c = ~term
            n = int(c.sum())
            if n > 0:
                s1 = tree_sum(np.where(c[:, None], y + 0.0, 0.0))
                s2 = tree_sum(np.where(c[:, None], y * y, 0.0))
                my, vy = batch_moments(s1, s2, np.float64(n))
                mo, vo = (my - bias) / scale, vy / (scale * scale)
                st["mean"], st["var"], ok = merge(st["mean"], st["var"], st["cnt"], mo, vo, n)
                st["n_skipped"] += int((~ok).sum())
                st["cnt"] = st["cnt"] + np.float64(n)
                sc, bi = tables(st["mean"], st["var"], eps)
                scale, bias = np.where(ok, sc, scale), np.where(ok, bi, bias)
        if reward_on:
            G, seen = st["G"], st["t_seen"]
            same = ts == seen
            fresh = ~same & (ts == 0)
            live = ~same & ~fresh
            r = np.asarray(reward).astype(np.float64) / rs
            g = _fma(np.float64(gamma), G, np.where(live, r, 0.0))
            l1, l2 = np.where(live, g + 0.0, 0.0), np.where(live, g * g, 0.0)
            st["G"] = np.where(live, np.where(term | trunc, 0.0, g), np.where(fresh, 0.0, G))
            st["t_seen"] = np.where(live, ts, np.where(fresh, 0, seen)).astype(np.int32)
            nr = int(live.sum())
            if nr > 0:
                my, vy = batch_moments(tree_sum(l1), tree_sum(l2), np.float64(nr))
                m, v, ok = merge(st["rmean"], st["rvar"], st["rcnt"], my, vy, nr)
                if bool(np.all(ok)):
                    st["rmean"], st["rvar"] = float(np.reshape(m, ())), float(np.reshape(v, ()))
                    st["rcnt"] = float(st["rcnt"] + np.float64(nr))
                    rs = reward_scale(st["rvar"], eps)
                else:
                    st["n_skipped"] += 1
    return scale, bias, rs
