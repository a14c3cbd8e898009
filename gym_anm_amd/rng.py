"""Host restatement of the device-side counter-based RNG (Philox4x32-10, csrc/anm_device.hpp).

The reference samples initial states on the host with NumPy's PCG64 (``anm6_easy.py:25-52``); for
in-kernel autoreset of tens of thousands of environments this build draws them on the device
instead, keyed by ``(seed, environment index, reset count)`` so that any environment's stream can
be reproduced independently.  This module is the specification the kernel is tested against
(bit-exact integers, identical doubles).
"""

from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(seed: int, env: int, epoch: int, draw: int):
    c = [env & MASK, (env >> 32) & MASK, epoch & MASK, draw & MASK]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def u01(hi: int, lo: int) -> float:
    return float(((hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0)


def series_init_state(model, series, seed, env, epoch):
    """Initial state the step kernel draws for environment ``env`` at its ``epoch``-th autoreset
    (series-mode tasks, layout and quirks of ``ANM6Easy.init_state``)."""
    period = series.shape[1]
    D, nd, ng = model.N_device, model.N_des, model.N_non_slack_gen
    s0 = np.zeros(2 * D + nd + ng + 1)
    r = philox4x32(seed, env, epoch, 0)
    aux = (r[0] * period) >> 32
    s0[-1] = aux

    def uniform(u):
        q = philox4x32(seed, env, epoch, 1 + u // 2)
        return u01(q[2 * (u % 2)], q[2 * (u % 2) + 1])

    for s, k in enumerate(model.load_idx):
        s0[k] = series[s, aux]
    for g, k in enumerate(model.gen_idx):
        pm = series[model.N_load + g, aux]
        s0[k] = pm
        s0[2 * D + nd + g] = pm
        s0[D + k] = model.dev_q_min[k] + (model.dev_q_max[k] - model.dev_q_min[k]) * uniform(g)
    for e, k in enumerate(model.des_idx):
        s0[2 * D + e] = model.dev_soc_min[k] + (model.dev_soc_max[k] - model.dev_soc_min[k]) * uniform(ng + e)
    return s0


# ---------------------------------------------------------------------------------------------------------------------
# Uniform exogenous mode (``BatchedANMEnv(exogenous="uniform")``, anm_env_config.exo_mode = ANM_EXO_UNIFORM).
#
# Every step the kernels draw, per environment, P_i = lo_i + (hi_i - lo_i) u_i MW for unit i -- the loads by device id,
# then the non-slack generators by device id.  NORMATIVE:
#
# * K = 1.  The auxiliary variable is the step index t of the episode: 0 after a reset, aux_{t+1} = aux_t + 1,
#   t < 2^31 (the kernels keep it in an int32).  The draws of a step are keyed by the NEW index, so the stream can be
#   replayed from a state row alone (``next_vars(state)``).
# * An episode is named by (seed, global environment index, epoch); ``epoch`` is the value of the environment's reset
#   count when the episode's initial state was drawn -- every reset leaves the count one above it, so during the episode
#   epoch = reset_count - 1.
# * Stream layout.  One block under the seed gives the episode key,
#       K' = words 0, 1 of philox(seed; counter = (env lo, env hi, epoch, 0xFFFFFFFF)),
#   and block j of step t is
#       philox(K'; counter = (t, j, 0, 0x45584F31)).
#   Unit i takes words 2 (i % 2), 2 (i % 2) + 1 of block i // 2 through u01 -- the layout of the init sampler.
# * The init sampler keeps (seed; (env lo, env hi, epoch, draw)) with draw = 0 .. 1 + ceil((n_gen + n_des) / 2), far below
#   0xFFFFFFFF; the step stream's counters end in 0x45584F31, which no init-sampler counter of a real network does.  So
#   no (key, counter) pair is shared, whatever K' turns out to be (``init_pairs`` / ``exo_pairs`` list them).
# * The affine map is ONE fused multiply-add, fma(fl(hi - lo), u, lo): device, host test double and this file agree bit
#   for bit.  ``fma`` below evaluates it exactly in rationals and rounds once.
# * Initial state of the mode (autoreset, reset(options={"sampler": "device"}), sample_init_state()): aux = 0; loads and
#   generator P / P_max are the step stream at t = 0; generator Q and storage SoC are uniform from the init sampler's
#   blocks 1 + u // 2, quirks included (``series_init_state``); block 0 is unused.
# ---------------------------------------------------------------------------------------------------------------------
EXO_KEY_DRAW = 0xFFFFFFFF
EXO_TAG = 0x45584F31


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with one rounding (finite arguments)."""
    from fractions import Fraction

    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        # an exact zero: the sign IEEE gives a sum of opposite-signed terms (round to nearest) is +0 unless both are -0
        prod_neg = (np.signbit(a) != np.signbit(b))
        return -0.0 if (prod_neg and np.signbit(c)) else 0.0
    return float(r)          # int / int true division: correctly rounded


def episode_key(seed: int, env: int, epoch: int) -> int:
    r = philox4x32(seed, env, epoch, EXO_KEY_DRAW)
    return r[0] | (r[1] << 32)


def exo_block(key: int, t: int, j: int):
    return philox4x32(key, (t & MASK) | ((j & MASK) << 32), 0, EXO_TAG)


def exo_uniform(seed, env, epoch, t, low, high):
    """P_load / P_pot (MW, ``[n_load + n_gen]``) of step ``t`` of the episode (seed, env, epoch)."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    key = episode_key(seed, env, epoch)
    out = np.empty(len(low))
    for i in range(len(low)):
        q = exo_block(key, t, i // 2)
        out[i] = fma(float(high[i] - low[i]), u01(q[2 * (i % 2)], q[2 * (i % 2) + 1]), float(low[i]))
    return out


def default_exo_bounds(model):
    """Default ends in MW: loads [p_min, 0], generators [0, p_max]."""
    low = np.zeros(model.N_load + model.N_non_slack_gen)
    high = np.zeros_like(low)
    for s, k in enumerate(model.load_idx):
        low[s] = model.dev_p_min[k] * model.baseMVA
    for g, k in enumerate(model.gen_idx):
        high[model.N_load + g] = model.dev_p_max[k] * model.baseMVA
    return low, high


def uniform_init_state(model, seed, env, epoch, low, high):
    """Initial state the kernels draw for environment ``env`` at its ``epoch``-th reset in the uniform mode."""
    D, nd, ng = model.N_device, model.N_des, model.N_non_slack_gen
    s0 = np.zeros(2 * D + nd + ng + 1)
    x = exo_uniform(seed, env, epoch, 0, low, high)

    def uniform(u):
        q = philox4x32(seed, env, epoch, 1 + u // 2)
        return u01(q[2 * (u % 2)], q[2 * (u % 2) + 1])

    for s, k in enumerate(model.load_idx):
        s0[k] = x[s]
    for g, k in enumerate(model.gen_idx):
        s0[k] = x[model.N_load + g]
        s0[2 * D + nd + g] = x[model.N_load + g]
        s0[D + k] = model.dev_q_min[k] + (model.dev_q_max[k] - model.dev_q_min[k]) * uniform(g)
    for e, k in enumerate(model.des_idx):
        s0[2 * D + e] = model.dev_soc_min[k] + (model.dev_soc_max[k] - model.dev_soc_min[k]) * uniform(ng + e)
    return s0


def init_pairs(seed, env, epoch, n_gen, n_des):
    """The (key, counter) pairs the init sampler may use for one (seed, env, epoch)."""
    n_draw = 2 + (n_gen + n_des + 1) // 2
    return {(seed & 0xFFFFFFFFFFFFFFFF, (env & MASK, (env >> 32) & MASK, epoch & MASK, d)) for d in range(n_draw)}


def exo_pairs(seed, env, epoch, t, n_exo):
    """The (key, counter) pairs of step ``t`` of the episode (seed, env, epoch): the key block and the step blocks."""
    key = episode_key(seed, env, epoch)
    pairs = {(seed & 0xFFFFFFFFFFFFFFFF, (env & MASK, (env >> 32) & MASK, epoch & MASK, EXO_KEY_DRAW))}
    pairs |= {(key, (t & MASK, j, 0, EXO_TAG)) for j in range((n_exo + 1) // 2)}
    return pairs


# ---------------------------------------------------------------------------------------------------------------------
# Noisy time series (``BatchedANMEnv(exogenous="series_noise")``, anm_env_config.exo_mode = ANM_EXO_SERIES_NOISE).
#
# Every step each load and non-slack generator takes its table value plus bounded noise, clipped to an interval.  NORMATIVE:
#
# * K = 1.  Inputs: the table ``series[n_exo, period]`` of series mode (MW; rows: loads by device id, then the non-slack
#   generators), an amplitude table ``noise[n_exo, period]`` (MW, finite, >= 0) and clip ends ``low``, ``high`` ``[n_exo]``
#   (MW, low <= high, no NaN; an infinite end means "no clip" on that side; defaults: ``default_exo_bounds``).
# * The aux variable is the table index, exactly as in series mode: aux' = int(fmod(aux + 1, period)).  Observations keep
#   ANM6Easy's layout and meaning.
# * Because aux wraps it cannot key the stream.  The step index of the episode does: t' = timestep + 1 on a real step, 0
#   for the initial state (``timestep`` is therefore a mandatory argument of a step in this mode).  Consequence: (state
#   row, timestep, reset count) replays the stream; the state row alone does not -- a ``next_vars(state)`` of this task
#   has to read ``self.timestep`` too.
# * Stream: the step stream of the uniform mode, unchanged -- ``episode_key``, ``exo_block``, the same tag; unit i takes
#   words 2 (i % 2), 2 (i % 2) + 1 of block i // 2 of step t'; the epoch is reset_count - 1 during an episode.  A model has
#   ONE exogenous mode, so the two modes never draw for the same task: sharing the stream is safe.
# * Map, with u = u01(words):
#       w   = fma(2.0, u, -1.0)          exact: u = k 2^-53, so 2u - 1 = (k - 2^52) 2^-52 with |k - 2^52| <= 2^52
#       x   = fma(noise[i, aux'], w, series[i, aux'])                                          the ONE rounding
#       P_i = x < low_i ? low_i : (x > high_i ? high_i : x)
#   Compares and selects, not min / max: the sign of a zero and infinite ends then mean the same on the device and here.
# * Initial state (autoreset, reset() without rows, sample_init_state()): t0 from word 0 of block 0 of the init sampler,
#   exactly as in series mode; loads and generator P / P_max are the map above at aux' = t0, step index 0, epoch = the
#   reset count the draw is made with; generator Q and storage SoC from the init sampler's units, quirks included.  A
#   reset from rows the caller brings uses them as they are and still advances the reset count, as in the uniform mode.
# * Anchor: with noise == 0 and ends that do not bite, fma(0, w, s) = s -- every draw, the initial state and therefore
#   every output equals series mode's bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def noise_clip(x: float, low: float, high: float) -> float:
    """The select-form clip of the mode."""
    return low if x < low else (high if x > high else x)


def exo_series_noise(seed, env, epoch, t, aux, series, noise, low, high):
    """P_load / P_pot (MW, ``[n_load + n_gen]``) of step index ``t`` of the episode (seed, env, epoch) at table index ``aux``."""
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    key = episode_key(seed, env, epoch)
    out = np.empty(series.shape[0])
    for i in range(series.shape[0]):
        q = exo_block(key, t, i // 2)
        w = fma(2.0, u01(q[2 * (i % 2)], q[2 * (i % 2) + 1]), -1.0)
        out[i] = noise_clip(fma(float(noise[i, aux]), w, float(series[i, aux])), float(low[i]), float(high[i]))
    return out


def series_noise_init_state(model, series, noise, low, high, seed, env, epoch):
    """Initial state the kernels draw for environment ``env`` at its ``epoch``-th reset in the series-noise mode."""
    s0 = series_init_state(model, series, seed, env, epoch)
    D, nd = model.N_device, model.N_des
    x = exo_series_noise(seed, env, epoch, 0, int(s0[-1]), series, noise, low, high)
    for s, k in enumerate(model.load_idx):
        s0[k] = x[s]
    for g, k in enumerate(model.gen_idx):
        s0[k] = x[model.N_load + g]
        s0[2 * D + nd + g] = x[model.N_load + g]
    return s0

# ---------------------------------------------------------------------------------------------------------------------
# Correlated noise for the noisy time series (``BatchedANMEnv(exogenous="series_noise", exo_corr=rho)``; an
# anm_env_config_corr, tail = ANM_ENV_TAIL_CORR).
#
# The noise of the mode above is independent from one step to the next; forecast errors of wind, sun and load are not.
# With a correlation the factor w drives an AR(1) chain per unit and the chain's state takes w's place in the map.
# NORMATIVE:
#
# * ``rho``: a scalar or ``[n_exo]`` (rows: loads by device id, then the non-slack generators), every entry finite and in
#   [0, 1).  ``exo_corr=None`` is the mode above with no new buffer; an explicit 0.0 runs the path below.
# * Per unit i the environment keeps a noise state z_i in a persistent tensor ``exo_z`` ``[num_envs, n_exo]`` (float64,
#   allocated once).  The caller may read it and never writes it.
# * c_i = math.sqrt(1.0 - rho_i * rho_i), computed ONCE on the host in Python; both tables travel to the library and the
#   kernels take no square root.  The library refuses rho outside [0, 1) and c outside (0, 1].
# * A real step, with w the mode's factor fma(2, u, -1) from the mode's block of the NEW step index t' and aux' the new
#   table index:
#       t   = c_i * w                      one rounded product, a statement of its own
#       z'  = fma(rho_i, z_i, t)           one rounding; stored to exo_z
#       x   = fma(noise[i, aux'], z', series[i, aux'])
#       P_i = x < low_i ? low_i : (x > high_i ? high_i : x)
#   Stream, key, tag, block layout and the table index update are those of the mode above, unchanged.  z' is stored
#   whether or not the step's power flow converges.
# * Initial state (autoreset, reset() without rows, a failed draw that is redrawn): z_i = w_i at step index 0 of the epoch
#   the draw is made with -- the factor the mode already uses for the initial P, so ``series_noise_init_state`` gives the
#   initial row for every rho.  The process is stationary from step 0: Var z = 1/3 at every step (rho^2 / 3 + c^2 / 3).
# * A reset() from rows the caller brings keeps the rows, stores the same z_i = w_i(step 0) of its epoch -- the reset count
#   as it stands before the call -- and advances the reset count as in the mode above.
# * The step of a terminated environment without autoreset (the absorbing no-op) touches nothing, exo_z included.
# * Consequences: (state row, timestep, reset count, exo_z row) replays the stream.  |z| is bounded by c / (1 - rho) + 1,
#   not by 1 (|w| <= 1 and the geometric sum of the innovations, plus the rounding): the clip ends are what keeps P
#   physical, and their defaults stay ``default_exo_bounds``.
# * Anchor: rho = 0 gives c = 1, t = w, z' = fma(0, z, w) = w (w is never -0 and z is always finite): every draw, exo_z
#   aside, equals the mode above bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def exo_factors(seed, env, epoch, t, n_exo):
    """The factors w = fma(2, u, -1) of the ``n_exo`` units at step index ``t`` of the episode (seed, env, epoch)."""
    key = episode_key(seed, env, epoch)
    out = np.empty(n_exo)
    for i in range(n_exo):
        q = exo_block(key, t, i // 2)
        out[i] = fma(2.0, u01(q[2 * (i % 2)], q[2 * (i % 2) + 1]), -1.0)
    return out


def series_corr_init_z(seed, env, epoch, n_exo):
    """The noise states an episode starts from: the factors of step index 0 of its epoch."""
    return exo_factors(seed, env, epoch, 0, n_exo)


def exo_innovation(rho):
    """c = sqrt(1 - rho^2) per unit, as the host forms it (``math.sqrt`` of the float64 expression, once)."""
    import math

    return np.array([math.sqrt(1.0 - float(r) * float(r)) for r in np.atleast_1d(np.asarray(rho, dtype=np.float64))])


def exo_series_corr(seed, env, epoch, t, aux, z, series, noise, rho, innov, low, high):
    """One real step of the correlated mode: ``(P, z')`` -- P_load / P_pot (MW, ``[n_load + n_gen]``) of step index ``t`` of
    the episode (seed, env, epoch) at table index ``aux`` and the advanced noise states -- from the states ``z`` before it."""
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    n = series.shape[0]
    w = exo_factors(seed, env, epoch, t, n)
    P, z1 = np.empty(n), np.empty(n)
    for i in range(n):
        tt = float(innov[i]) * float(w[i])
        z1[i] = fma(float(rho[i]), float(z[i]), tt)
        P[i] = noise_clip(fma(float(noise[i, aux]), float(z1[i]), float(series[i, aux])), float(low[i]), float(high[i]))
    return P, z1


# ---- vectorised forms (uint64 arithmetic), for batch-sized checks --------------------------------------------------
def philox4x32_v(seed, env, epoch, draw):
    """``philox4x32`` over arrays (broadcast): returns ``uint64 [..., 4]`` holding the four 32-bit words."""
    seed, env, epoch, draw = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (seed, env, epoch, draw)))
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    c0, c1, c2, c3 = env & m, (env >> s32) & m, epoch & m, draw & m
    k0, k1 = seed & m, (seed >> s32) & m
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ k0) & m, p1 & m, ((p0 >> s32) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([c0, c1, c2, c3], axis=-1)


def u01_v(hi, lo):
    v = ((np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)) >> np.uint64(11)
    return v.astype(np.float64) * (1.0 / 9007199254740992.0)


def exo_uniform_v(seed, env, epoch, t, low, high):
    """``exo_uniform`` for arrays of env / epoch / t (broadcast): ``[..., n_load + n_gen]``.  The affine map is plain
    arithmetic here, lo + (hi - lo) u: up to one rounding off the fused one."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    env, epoch, t = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (env, epoch, t)))
    kw = philox4x32_v(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), env, epoch, np.uint64(EXO_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))
    out = np.empty(env.shape + (len(low),))
    for j in range((len(low) + 1) // 2):
        q = philox4x32_v(key, (t & np.uint64(MASK)) | (np.uint64(j) << np.uint64(32)), np.uint64(0), np.uint64(EXO_TAG))
        for h in range(2):
            i = 2 * j + h
            if i < len(low):
                out[..., i] = low[i] + (high[i] - low[i]) * u01_v(q[..., 2 * h], q[..., 2 * h + 1])
    return out


def uniform_init_state_v(model, seed, env, epoch, low, high):
    """``uniform_init_state`` for arrays of env / epoch: ``[n, state_N]`` (affine maps in plain arithmetic)."""
    env, epoch = np.broadcast_arrays(np.asarray(env, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64))
    D, nd, ng = model.N_device, model.N_des, model.N_non_slack_gen
    s0 = np.zeros(env.shape + (2 * D + nd + ng + 1,))
    x = exo_uniform_v(seed, env, epoch, 0, low, high)
    sd = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)

    def uniform(u):
        q = philox4x32_v(sd, env, epoch, np.uint64(1 + u // 2))
        return u01_v(q[..., 2 * (u % 2)], q[..., 2 * (u % 2) + 1])

    for s, k in enumerate(model.load_idx):
        s0[..., k] = x[..., s]
    for g, k in enumerate(model.gen_idx):
        s0[..., k] = x[..., model.N_load + g]
        s0[..., 2 * D + nd + g] = x[..., model.N_load + g]
        s0[..., D + k] = model.dev_q_min[k] + (model.dev_q_max[k] - model.dev_q_min[k]) * uniform(g)
    for e, k in enumerate(model.des_idx):
        s0[..., 2 * D + e] = model.dev_soc_min[k] + (model.dev_soc_max[k] - model.dev_soc_min[k]) * uniform(ng + e)
    return s0


def exo_series_noise_v(seed, env, epoch, t, aux, series, noise, low, high):
    """``exo_series_noise`` for arrays of env / epoch / t / aux (broadcast): ``[..., n_load + n_gen]``.  The map is plain
    arithmetic here, series + noise (2 u - 1): up to one rounding off the fused one (before the clip)."""
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    env, epoch, t, aux = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (env, epoch, t, aux)))
    aux = aux.astype(np.int64)
    kw = philox4x32_v(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), env, epoch, np.uint64(EXO_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))
    n = series.shape[0]
    out = np.empty(env.shape + (n,))
    for j in range((n + 1) // 2):
        q = philox4x32_v(key, (t & np.uint64(MASK)) | (np.uint64(j) << np.uint64(32)), np.uint64(0), np.uint64(EXO_TAG))
        for h in range(2):
            i = 2 * j + h
            if i < n:
                x = series[i][aux] + noise[i][aux] * (2.0 * u01_v(q[..., 2 * h], q[..., 2 * h + 1]) - 1.0)
                out[..., i] = np.where(x < low[i], low[i], np.where(x > high[i], high[i], x))
    return out


def series_noise_init_state_v(model, series, noise, low, high, seed, env, epoch):
    """``series_noise_init_state`` for arrays of env / epoch: ``[n, state_N]`` (maps in plain arithmetic)."""
    env, epoch = np.broadcast_arrays(np.asarray(env, dtype=np.uint64), np.asarray(epoch, dtype=np.uint64))
    series = np.asarray(series, dtype=np.float64)
    D, nd, ng = model.N_device, model.N_des, model.N_non_slack_gen
    sd = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
    s0 = np.zeros(env.shape + (2 * D + nd + ng + 1,))
    aux = (philox4x32_v(sd, env, epoch, np.uint64(0))[..., 0] * np.uint64(series.shape[1])) >> np.uint64(32)
    s0[..., -1] = aux
    x = exo_series_noise_v(seed, env, epoch, 0, aux, series, noise, low, high)

    def uniform(u):
        q = philox4x32_v(sd, env, epoch, np.uint64(1 + u // 2))
        return u01_v(q[..., 2 * (u % 2)], q[..., 2 * (u % 2) + 1])

    for s, k in enumerate(model.load_idx):
        s0[..., k] = x[..., s]
    for g, k in enumerate(model.gen_idx):
        s0[..., k] = x[..., model.N_load + g]
        s0[..., 2 * D + nd + g] = x[..., model.N_load + g]
        s0[..., D + k] = model.dev_q_min[k] + (model.dev_q_max[k] - model.dev_q_min[k]) * uniform(g)
    for e, k in enumerate(model.des_idx):
        s0[..., 2 * D + e] = model.dev_soc_min[k] + (model.dev_soc_max[k] - model.dev_soc_min[k]) * uniform(ng + e)
    return s0


# ---------------------------------------------------------------------------------------------------------------------
# Perfect forecast of the drawn modes (``MPCAgentPerfectStream``, anm_mpc_act_stream_f64; csrc/anm_mpc.hpp, Act mode 3).
#
# The draws of step index t of an episode are a pure function of (seed, global environment index, epoch, t, unit), so the
# future of a running episode is the stream evaluated ahead.  NORMATIVE, for an environment with global index env,
# epoch = uint32(reset_count - 1), current step index t (``timestep``) and, in series-noise mode, current table index aux:
#
# * stage i in [0, N) has step index t_i = uint32(t + 1 + i) and table index aux_i = (aux + 1 + i) % period (series
#   mode's update applied i + 1 times);
# * uniform mode:       unit u of stage i is ``exo_uniform(seed, env, epoch, t_i, low, high)[u]``;
# * series-noise mode:  unit u of stage i is ``exo_series_noise(seed, env, epoch, t_i, aux_i, series, noise, low, high)[u]``;
# * units: loads by slot, then the non-slack generators; values in MW (the program takes value / baseMVA, a true division);
# * the same function for an environment that is terminated or past its episode limit (the step that follows resets it
#   and ignores the action); the horizon is not cut at ``max_episode_steps``.
# ---------------------------------------------------------------------------------------------------------------------
def exo_forecast(seed, env, epoch, t, N, low, high, series=None, noise=None, aux=None):
    """Loads / generator potentials (MW, ``[n_load + n_gen, N]``) of the N steps after step index ``t`` of the episode
    (seed, env, epoch): uniform mode, or -- with ``series``, ``noise`` and the current table index ``aux`` -- series-noise mode."""
    n = len(low)
    out = np.empty((n, int(N)))
    for i in range(int(N)):
        ti = (int(t) + 1 + i) & MASK
        if series is None:
            out[:, i] = exo_uniform(seed, env, epoch, ti, low, high)
        else:
            period = np.asarray(series).shape[1]
            out[:, i] = exo_series_noise(seed, env, epoch, ti, (int(aux) + 1 + i) % period, series, noise, low, high)
    return out


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_v(a, b, c):
    """``fma`` over arrays (broadcast), correctly rounded: the product and the sum are kept as exact two-term expansions and
    the low parts are added with rounding to odd before the one rounding to nearest (Boldo and Melquiond, "Emulation of a FMA
    and correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 57(4), 2008).  The expansions are exact away
    from overflow and underflow only: elements whose product is not comfortably inside the normal range go through ``fma``."""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (a, b, c)))
    with np.errstate(all="ignore"):
        p = a * b

        def split(x):
            g = 134217729.0 * x          # 2^27 + 1 (Veltkamp)
            h = g - (g - x)
            return h, x - h

        ah, al = split(a)
        bh, bl = split(b)
        pl = ((ah * bh - p) + ah * bl + al * bh) + al * bl          # a b = p + pl
        th, tl = _two_sum(c, p)                                      # c + p = th + tl
        s, e = _two_sum(tl, pl)
        # round tl + pl to odd: an inexact sum goes to the neighbour with the odd significand
        even = (s.view(np.int64) & 1) == 0
        s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        z = th + s
    # an exact zero: the sign IEEE gives (see ``fma``)
    z = np.where(z == 0, np.where((np.signbit(a) != np.signbit(b)) & np.signbit(c), -0.0, 0.0), z)
    ap = np.abs(p)
    odd = ~np.isfinite(p) | ~np.isfinite(c) | ((ap != 0) & ((ap < 1e-200) | (ap > 1e200))) | (np.abs(c) > 1e200) | \
        ((p == 0) & (a != 0) & (b != 0))
    if odd.any():
        z = z.copy()
        for k in zip(*np.nonzero(odd)):
            z[k] = fma(float(a[k]), float(b[k]), float(c[k]))
    return z


def exo_forecast_v(seed, env_offset, reset_count, timestep, N, low, high, series=None, noise=None, aux=None):
    """``exo_forecast`` for the environments of a batch: ``[E, n_load + n_gen, N]`` MW from the per-environment arrays
    ``reset_count``, ``timestep`` (and ``aux``, series-noise mode); environment e has global index ``env_offset + e``.
    Unlike the other vectorised forms this one is EXACT (``fma_v``): it is what the unfused path of the agent feeds the
    solver, which has to see the bits the fused kernel draws."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    N = int(N)
    rc = np.asarray(reset_count).astype(np.int64).reshape(-1)
    E, n = rc.shape[0], len(low)
    m = np.uint64(MASK)
    epoch = ((rc - 1) & MASK).astype(np.uint64)[:, None]
    env = (np.uint64(int(env_offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(E, dtype=np.uint64))[:, None]
    ti = ((np.asarray(timestep).astype(np.int64).reshape(-1)[:, None] + 1 + np.arange(N)[None, :]) & MASK).astype(np.uint64)  # [E, N]
    kw = philox4x32_v(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), env, epoch, np.uint64(EXO_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))   # [E, 1]
    if series is not None:
        series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
        auxi = (np.asarray(aux).astype(np.int64).reshape(-1)[:, None] + 1 + np.arange(N)[None, :]) % series.shape[1]   # [E, N]
    out = np.empty((E, n, N))
    for j in range((n + 1) // 2):
        q = philox4x32_v(key, (ti & m) | (np.uint64(j) << np.uint64(32)), np.uint64(0), np.uint64(EXO_TAG))   # [E, N, 4]
        for h in range(2):
            i = 2 * j + h
            if i >= n:
                continue
            u = u01_v(q[..., 2 * h], q[..., 2 * h + 1])
            if series is None:
                out[:, i, :] = fma_v(high[i] - low[i], u, low[i])
            else:
                x = fma_v(noise[i][auxi], 2.0 * u - 1.0, series[i][auxi])   # (2 u - 1: exact, see the mode's map)
                out[:, i, :] = np.where(x < low[i], low[i], np.where(x > high[i], high[i], x))
    return out


def exo_factors_v(seed, env, epoch, t, n_exo):
    """``exo_factors`` for arrays of env / epoch / t (broadcast): ``[..., n_exo]`` (exact: 2 u - 1 does not round)."""
    env, epoch, t = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (env, epoch, t)))
    kw = philox4x32_v(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), env, epoch, np.uint64(EXO_KEY_DRAW))
    key = kw[..., 0] | (kw[..., 1] << np.uint64(32))
    out = np.empty(env.shape + (n_exo,))
    for j in range((n_exo + 1) // 2):
        q = philox4x32_v(key, (t & np.uint64(MASK)) | (np.uint64(j) << np.uint64(32)), np.uint64(0), np.uint64(EXO_TAG))
        for h in range(2):
            if 2 * j + h < n_exo:
                out[..., 2 * j + h] = 2.0 * u01_v(q[..., 2 * h], q[..., 2 * h + 1]) - 1.0
    return out


def series_corr_init_z_v(seed, env, epoch, n_exo):
    """``series_corr_init_z`` for arrays of env / epoch: ``[..., n_exo]``."""
    return exo_factors_v(seed, env, epoch, 0, n_exo)


def exo_series_corr_v(seed, env, epoch, t, aux, z, series, noise, rho, innov, low, high):
    """``exo_series_corr`` for arrays of env / epoch / t / aux (broadcast to ``[...]``) and states ``z`` ``[..., n_exo]``:
    ``(P, z')``, both ``[..., n_exo]``.  EXACT like ``exo_forecast_v``: both fused operations go through ``fma_v``."""
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    rho, innov = np.asarray(rho, dtype=np.float64), np.asarray(innov, dtype=np.float64)
    n = series.shape[0]
    w = exo_factors_v(seed, env, epoch, t, n)
    aux = np.broadcast_to(np.asarray(aux).astype(np.int64), w.shape[:-1])
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), w.shape)
    tt = innov * w                                   # one rounded product per element
    z1 = fma_v(rho, z, tt)
    P = np.empty(w.shape)
    for i in range(n):
        x = fma_v(noise[i][aux], z1[..., i], series[i][aux])
        P[..., i] = np.where(x < low[i], low[i], np.where(x > high[i], high[i], x))
    return P, z1


# ---------------------------------------------------------------------------------------------------------------------
# Perfect forecast of the correlated series-noise task (``MPCAgentPerfectChain``, anm_mpc_act_chain_f64; csrc/anm_mpc.hpp,
# Act mode 4).
#
# With ``exo_corr`` the draws of a step depend on the noise state of every unit, so the future of a running episode is no
# longer a function of the step index alone: it is the step's own recurrence, rolled forward from the environment's row
# of ``exo_z``.  NORMATIVE, for an environment with global index env, epoch = uint32(reset_count - 1), current step index
# t (``timestep``), current table index aux and noise states z (its row of ``exo_z`` at the time of ``act()``):
#
# * z_(-1) = z; for i = 0 .. N-1:
#       (P_i, z_i) = exo_series_corr(seed, env, epoch, (t + 1 + i) & MASK, (aux + 1 + i) % period, z_(i-1), ...)
#   and stage i of the forecast is P_i.  Nothing new is defined: the key, tag, block layout, table index, the rounded
#   product c w, the one fma of the recurrence and the one fma plus compare-selects of the map are those of the mode
#   (above: "Correlated noise for the noisy time series") -- every z_i is produced by the operations the step will
#   perform, in their order, so the forecast is exact and not approximately right;
# * units, MW and the division by baseMVA, "an environment that is terminated or past its limit gets the same function"
#   and "the horizon is not cut at ``max_episode_steps``" as for the stream forecast above;
# * a pure function of (seed, global index, epoch, t, aux, exo_z row).  The agent only reads ``exo_z``;
# * Anchor: rho = 0 gives z_i = fma(0, z_(i-1), w_i) = w_i for any starting z: ``exo_forecast`` of the uncorrelated task,
#   bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def exo_forecast_corr(seed, env, epoch, t, N, aux, z, series, noise, rho, innov, low, high):
    """Loads / generator potentials (MW, ``[n_load + n_gen, N]``) of the N steps after step index ``t`` of the episode
    (seed, env, epoch) of a correlated series-noise task, from the current table index ``aux`` and noise states ``z``."""
    period = np.asarray(series).shape[1]
    out = np.empty((len(low), int(N)))
    z = np.asarray(z, dtype=np.float64)
    for i in range(int(N)):
        out[:, i], z = exo_series_corr(seed, env, epoch, (int(t) + 1 + i) & MASK, (int(aux) + 1 + i) % period, z, series, noise,
                                       rho, innov, low, high)
    return out


def exo_forecast_corr_v(seed, env_offset, reset_count, timestep, N, aux, z, series, noise, rho, innov, low, high):
    """``exo_forecast_corr`` for the environments of a batch: ``[E, n_load + n_gen, N]`` MW from the per-environment arrays
    ``reset_count``, ``timestep``, ``aux`` and the noise states ``z`` ``[E, n_exo]``; environment e has global index
    ``env_offset + e``.  EXACT (``exo_series_corr_v`` applied N times): it is what the unfused path of the agent feeds the
    solver, which has to see the bits the fused kernel computes."""
    N = int(N)
    rc = np.asarray(reset_count).astype(np.int64).reshape(-1)
    E, period = rc.shape[0], np.asarray(series).shape[1]
    epoch = ((rc - 1) & MASK).astype(np.uint64)
    env = np.uint64(int(env_offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(E, dtype=np.uint64)
    t = np.asarray(timestep).astype(np.int64).reshape(-1)
    aux = np.asarray(aux).astype(np.int64).reshape(-1)
    z = np.asarray(z, dtype=np.float64).reshape(E, -1)
    out = np.empty((E, z.shape[1], N))
    for i in range(N):
        out[:, :, i], z = exo_series_corr_v(seed, env, epoch, ((t + 1 + i) & MASK).astype(np.uint64), (aux + 1 + i) % period, z,
                                            series, noise, rho, innov, low, high)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Expected forecast of the tasks drawn inside the step kernels (``MPCAgentExpected``, anm_mpc_act_expect_f64;
# csrc/anm_mpc.hpp, Act mode 5): what an operator forecasts who knows the task's noise model and its current state, but
# not the future draws -- the conditional mean of the noise, mapped like a draw.
#
# The innovations w = fma(2, u, -1) have mean 0 (u is uniform on the 53-bit grid of [0, 1), so the mean is -2^-53: nothing),
# hence the conditional mean of the chain is the step's own recurrence with the innovation at its mean,
# E[z_(t+1+i) | z_t] = rho^(i+1) z_t.  NORMATIVE, for stage i = 0 .. N-1 and unit u (loads by slot, then the non-slack
# generators), MW before the division by baseMVA, from the current table index aux and the environment's row z of ``exo_z``
# at the time of ``act()``:
#
# * ``series_noise`` with ``exo_corr``:  zb_(-1) = z_u;  zb_i = fma(rho_u, zb_(i-1), 0.0) -- the recurrence of the mode
#   (``exo_series_corr``) with w = 0.0: the rounded product c * 0.0 is +0.0 for every valid c, so ``exo_innov`` is no input;
#   at_i = (aux + 1 + i) % period;  P_i = noise_clip(fma(noise[u, at_i], zb_i, series[u, at_i]), low_u, high_u) -- the one
#   fma and the compare-select clip of the mode's map;
# * ``series_noise`` with ``exo_corr=None``:  zb_i = +0.0 at every stage, the same map.  ``exo_corr=0.0`` gives this bit for
#   bit: fma(0, z, +0.0) = +0.0 for every finite z (an exact zero sum of -0 and +0 is +0);
# * ``uniform``:  P_i = fma(high_u - low_u, 0.5, low_u) at every stage: the mode's map at u = 0.5.
#
# The conditional mean of the NOISE is mapped, so where the clip bites P_i is not the mean of the clipped draw; with ends
# the noise does not reach it is (up to the rounding of the recurrence).  A pure function of (aux, the row of exo_z): no
# RNG, ``timestep``, ``reset_count`` or ``env_offset``; an environment that is terminated or past its limit gets the same
# function, the horizon is not cut at ``max_episode_steps``, and ``exo_z`` is only read.
# ---------------------------------------------------------------------------------------------------------------------
def exo_forecast_expected(N, low, high, aux=None, z=None, series=None, noise=None, rho=None):
    """Expected loads / generator potentials (MW, ``[n_load + n_gen, N]``) of the next N steps of a drawn task: the uniform
    mode (``series`` None), the series-noise mode from the table index ``aux`` (``rho`` None: no correlation), and with
    correlated noise from the noise states ``z`` ``[n_exo]`` too."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    n, N = len(low), int(N)
    out = np.empty((n, N))
    if series is None:
        for u in range(n):
            out[u, :] = fma(float(high[u]) - float(low[u]), 0.5, float(low[u]))
        return out
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    period = series.shape[1]
    for u in range(n):
        zb = 0.0 if rho is None else float(z[u])
        for i in range(N):
            if rho is not None:
                zb = fma(float(rho[u]), zb, 0.0)
            at = (int(aux) + 1 + i) % period
            out[u, i] = noise_clip(fma(float(noise[u, at]), zb, float(series[u, at])), float(low[u]), float(high[u]))
    return out


def exo_forecast_expected_v(E, N, low, high, aux=None, z=None, series=None, noise=None, rho=None):
    """``exo_forecast_expected`` for the ``E`` environments of a batch: ``[E, n_load + n_gen, N]`` MW from the per-environment
    table indices ``aux`` ``[E]`` and noise states ``z`` ``[E, n_exo]``.  EXACT (``fma_v``): it is what the unfused path of
    the agent feeds the solver, which has to see the bits the fused kernel computes."""
    low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
    E, n, N = int(E), len(low), int(N)
    out = np.empty((E, n, N))
    if series is None:
        out[:] = fma_v(high - low, 0.5, low)[None, :, None]
        return out
    series, noise = np.asarray(series, dtype=np.float64), np.asarray(noise, dtype=np.float64)
    aux = np.asarray(aux).astype(np.int64).reshape(-1)
    zb = np.zeros((E, n)) if rho is None else np.array(z, dtype=np.float64).reshape(E, n)
    for i in range(N):
        if rho is not None:
            zb = fma_v(np.asarray(rho, dtype=np.float64)[None, :], zb, 0.0)
        at = (aux + 1 + i) % series.shape[1]                               # [E]
        for u in range(n):
            x = fma_v(noise[u][at], zb[:, u], series[u][at])
            out[:, u, i] = np.where(x < low[u], low[u], np.where(x > high[u], high[u], x))
    return out
