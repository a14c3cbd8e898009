// anm_policy_grad.hpp -- the gradient of the clipped PPO loss with respect to the flat parameter vector of the Gaussian MLP
// policy, in two launches (anm_policy_ppo_grad; gym_anm_amd/policy_grad.py is the specification, rule numbers below are its).
// The forward pass is anm_policy.hpp's, by inclusion: layer(), load_rows(), tanh32(), wave_sync().
//
//   k_ppo_grad    the parameters are staged in LDS once per workgroup as they lie in memory (k_policy's loop), and behind them a
//                 TRANSPOSED copy WT [N (even), K] of every layer that has a hidden layer below it.  A wavefront owns a group of R
//                 consecutive minibatch rows and takes them 32 at a time.  Per net (critic, then actor) the forward pass keeps
//                 every layer's activation: tile i holds the input of layer i, and column K_i of it holds 1.0, so that the bias
//                 is row K of the augmented weight.  One lane per row forms the loss coefficients (rules 4 to 7) and leaves dY of
//                 the head in the head's tile.  Then, from the head down:
//                   dW    D[k][n] = sum_row x[row][k] dy[row][n] on v_mfma_f32_32x32x2_f32 with the ROW as the instruction's k:
//                         the A operand is x[row = 2 s + (l >> 5)][k0 + (l & 31)], the B operand dy[row][n0 + (l & 31)] -- both
//                         consecutive words for consecutive lanes -- and the accumulator of lane (n, h) holds k = k0 + (r & 3) +
//                         8 (r >> 2) + 4 h, so a store of one register is 32 consecutive words of the partial.  The accumulator
//                         starts at +0 for the group's first 32 rows and at the words the SAME lane stored before for the later
//                         ones: the chain over the R rows is unbroken (rule 8).
//                   dX    D[k][row] = sum_n WT[n][k] dy[row][n]: the A operand is WT[n = 2 s + (l >> 5)][k0 + (l & 31)] --
//                         consecutive words, which is what the transposed copy is for: W [K, N] as it lies has lanes that differ
//                         in k a multiple of 32 words apart, all on one bank -- the B operand dy[row = l & 31][n] (odd row
//                         stride).  Lane (row, h) then holds dX of ITS row and multiplies by the activation's derivative from
//                         the stored output, IN PLACE: tile i becomes dY of layer i - 1 once dW of layer i has read it.
//                 log_std's gradient and the five sums of the statistics are one more dW tile with x = the ones column.
//   k_ppo_reduce  one thread per parameter adds the partials in ascending group order, divides by n and overwrites grad (no
//                 memset, no accumulation); one more workgroup forms the eight statistics.
//
// No atomics; nothing but the partials crosses a wavefront, and a partial is written and read back by one lane.  Rows past B are
// neither read nor written; the parameters and the minibatch are never written.
#pragma once

#include <cstdint>

#include "anm_policy.hpp"

namespace anm {
namespace ppo {

using policy::MAX_LAYERS;
using policy::ROWS;
using policy::f32x16;
using policy::wave_sync;

constexpr int STATS = 8;                     // floats behind the P gradient words of a partial, and the statistics vector
constexpr int ST_PG = 0, ST_V = 1, ST_KL = 2, ST_CLIP = 3, ST_N = 4;   // columns of a partial's statistics
constexpr int END_PAD = 32;                  // floats behind the last wavefront's tiles: an operand read runs up to 31 words on
constexpr int MAX_WAVES = 4;
constexpr int REDUCE_THREADS = 256;

struct Args {
  policy::Args p;                            // params, the nets, D, A, S, activation, vec4, logp0, obs: what layer() and load_rows() take
  int32_t SE;                                // row stride of the extra tile [ROWS][A + STATS] (odd)
  int32_t n_tiles;                           // activation tiles of a wavefront: hidden layers + 2
  int32_t wt_actor[MAX_LAYERS], wt_critic[MAX_LAYERS];   // offsets of the transposed copies (layer 0 has none)
  int32_t wt_floats;
  const void *actions, *logp_old, *v_old, *returns, *adv, *weight;
  float *partials, *ratio, *logp, *values, *inv_std;
  int64_t B;
  int32_t R;
  float clip_lo, clip_hi, vf_coef, vf_clip;  // 1 - c, 1 + c; vf_clip < 0: off
};

struct ReduceArgs {
  const float* partials;
  const float* params;
  float *grad, *stats;
  int32_t P, A, log_std;
  int64_t G;                                 // partials
  float vf_coef, ent_coef, ent_const;        // float32(0.5 + 0.5 ln 2 pi)
};

// floats of the plan with `waves` wavefronts per workgroup (policy_grad.grad_lds_floats)
inline int64_t lds_floats(int64_t n_params, int64_t wt_floats, int n_tiles, int S, int SE, int waves) {
  return n_params + policy::W_PAD + policy::STD_PAD + wt_floats + int64_t(waves) * ROWS * (int64_t(n_tiles) * S + SE) + END_PAD;
}

template <bool F32>
__device__ inline float ld(const void* p, int64_t i) {
  if constexpr (F32) return static_cast<const float*>(p)[i];
  else return float(static_cast<const double*>(p)[i]);
}

// rule 8: the partial of one augmented weight [K1, N] (row K1 - 1 is the bias) from the input tile x (1.0 in column K1 - 1)
// and the tile dy; `first`: the chain starts here
__device__ inline void grad_w(float* part, int K1, int N, const float* x, int Sx, const float* dy, int Sy, bool first, int lane) {
  const int j = lane & 31, h = lane >> 5;
  for (int k0 = 0; k0 < K1; k0 += 32) {
    for (int n0 = 0; n0 < N; n0 += 32) {
      const int n = n0 + j;
      float* out = part + n;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        acc[r] = (!first && k < K1 && n < N) ? out[k * N] : 0.0f;
      }
      // a lane whose k0 + j is past K1, or whose n is past N, reads what follows in the wavefront's tiles (inside LDS: END_PAD)
      // into a row or a column of the product that is never stored
      const float* xa = x + h * Sx + k0 + j;
      const float* ya = dy + h * Sy + n0 + j;
#pragma unroll
      for (int s = 0; s < ROWS / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s * Sx], ya[2 * s * Sy], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (k < K1 && n < N) out[k * N] = acc[r];
      }
    }
  }
  wave_sync();                                           // (the tile x is written next)
}

// rule 9: y [ROWS][S] holds the activation's output and receives dY of the layer below, in place; g is dY of this layer,
// WT [Np][K] its transposed weight (Np even: a zero row behind an odd N, and g's column N is +0 then)
__device__ inline void grad_x(const float* WT, int K, int Np, const float* g, float* y, int S, int activation, int lane) {
  const int row = lane & 31, h = lane >> 5;
  const float* ga = g + row * S + h;
  for (int k0 = 0; k0 < K; k0 += 32) {
    const float* wa = WT + h * K + k0 + row;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    int n = 0;
    for (; n + 8 <= Np; n += 8) {
      float wv[4], gv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        wv[q] = wa[(n + 2 * q) * K];
        gv[q] = ga[n + 2 * q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[q], gv[q], acc, 0, 0, 0);
    }
    for (; n < Np; n += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[n * K], ga[n], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = k0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const float yv = y[row * S + k];
      y[row * S + k] = activation == policy::ACT_TANH ? acc[r] * __fmaf_rn(-yv, yv, 1.0f) : (yv > 0.0f ? acc[r] : 0.0f);
    }
  }
  wave_sync();
}

// the forward pass of one net, every activation kept: tile i is the input of layer i, tile n_layers the head
__device__ inline void forward(const float* w, const policy::Net& net, float* tile, int S, int activation, int lane) {
  for (int i = 0; i < net.n_layers; ++i)
    policy::layer(w + net.w[i], w + net.b[i], net.K[i], net.N[i], tile + i * ROWS * S, tile + (i + 1) * ROWS * S, S, activation,
                  i + 1 < net.n_layers, lane);
}

// the backward pass of one net from dY of the head in tile n_layers
__device__ inline void backward(float* part, const float* wt, const int32_t* wt_off, const policy::Net& net, float* tile, int S,
                                int activation, bool first, int lane) {
  for (int i = net.n_layers - 1; i >= 0; --i) {
    float* x = tile + i * ROWS * S;
    const float* dy = tile + (i + 1) * ROWS * S;
    grad_w(part + net.w[i], net.K[i] + 1, net.N[i], x, S, dy, S, first, lane);
    if (i > 0) grad_x(wt + wt_off[i], net.K[i], (net.N[i] + 1) & ~1, dy, x, S, activation, lane);
  }
}

// rule 1 for a net's first tile: the observation rows, zeros for a row that does not count
template <bool IO32>
__device__ inline void load_obs(const Args& a, float* tile, int64_t e0, int rows, bool live, int lane) {
  const int row = lane & 31, h = lane >> 5;
  policy::load_rows<IO32>(a.p, tile, e0, rows, lane);
  wave_sync();
  if (!live)
    for (int k = h; k < a.p.D; k += 2) tile[row * a.p.S + k] = 0.0f;
  wave_sync();
}

// 32 rows of one wavefront: rules 1 to 9
template <bool IO32, bool V32>
__device__ inline void rows_of_wave(const Args& a, const float* w, const float* istd, const float* wt, float* tile, float* extra,
                                    float* part, int64_t e0, bool first, int lane) {
  const int rows = a.B - e0 < ROWS ? int(a.B - e0) : ROWS;
  const int row = lane & 31, h = lane >> 5;
  const int S = a.p.S, A = a.p.A, L = a.p.critic.n_layers;
  const bool in_rows = row < rows;
  const int64_t e = e0 + row;
  const float wgt = in_rows ? ld<V32>(a.weight, e) : 0.0f;
  const bool live = in_rows && wgt != 0.0f;              // (a NaN weight counts: it poisons, as in torch)
  float* head = tile + L * ROWS * S;
  float* ex = extra + row * a.SE;

  if (h == 0)
    for (int i = 0; i < L; ++i) tile[i * ROWS * S + row * S + a.p.critic.K[i]] = 1.0f;   // (both nets have the same K)
  for (int c = h; c < A + STATS; c += 2) ex[c] = 0.0f;

  // ---- the critic: rule 6
  load_obs<IO32>(a, tile, e0, rows, live, lane);
  forward(w, a.p.critic, tile, S, a.p.activation, lane);
  if (h == 0) {
    float dyv = 0.0f, v = 0.0f;
    if (live) {
      v = head[row * S];
      const float ret = ld<V32>(a.returns, e);
      const float d = v - ret;
      float big = d * d, gr = d;
      if (a.vf_clip >= 0.0f) {
        const float vo = ld<V32>(a.v_old, e);
        const float dv = v - vo;
        const bool lo = dv < -a.vf_clip, hi = dv > a.vf_clip;
        const float dc = lo ? -a.vf_clip : (hi ? a.vf_clip : dv);
        const float d2 = (vo + dc) - ret;
        const float e2 = d2 * d2;
        if (e2 > big) {
          big = e2;
          gr = (lo || hi) ? 0.0f : d2;
        }
      }
      dyv = (wgt * a.vf_coef) * gr;
      ex[A + ST_V] = wgt * (0.5f * big);
      ex[A + ST_N] = 1.0f;
    }
    head[row * S] = dyv;
    head[row * S + 1] = 0.0f;                            // (the head's N = 1 is odd: the zero column behind it)
    if (in_rows) a.values[e] = policy::canon32(v);
  }
  wave_sync();
  backward(part, wt, a.wt_critic, a.p.critic, tile, S, a.p.activation, first, lane);

  // ---- the actor: rules 3 to 5
  load_obs<IO32>(a, tile, e0, rows, live, lane);
  forward(w, a.p.actor, tile, S, a.p.activation, lane);
  if (h == 0) {
    float lp = 0.0f, ratio = 0.0f;
    if (live) {
      const float* ls = w + a.p.log_std;
      lp = a.p.logp0;
      for (int j = 0; j < A; ++j) {
        const float z = (ld<IO32>(a.actions, e * A + j) - head[row * S + j]) * istd[j];
        head[row * S + j] = z;
        lp = __fmaf_rn(-0.5f * z, z, lp);
        lp = __fsub_rn(lp, ls[j]);
      }
      const float lr = lp - ld<V32>(a.logp_old, e);
      ratio = float(exp(double(lr)));
      const float adv = ld<V32>(a.adv, e);
      const float s1 = ratio * adv;
      const float rc = ratio < a.clip_lo ? a.clip_lo : (ratio > a.clip_hi ? a.clip_hi : ratio);
      const float s2 = rc * adv;
      const float pg = -(s2 < s1 ? s2 : s1);
      const bool clipped = adv >= 0.0f ? ratio > a.clip_hi : (adv < 0.0f ? ratio < a.clip_lo : false);
      const float cl = wgt * (clipped ? 0.0f : -s1);
      for (int j = 0; j < A; ++j) {
        const float z = head[row * S + j];
        head[row * S + j] = cl * (z * istd[j]);
        ex[j] = cl * __fmaf_rn(z, z, -1.0f);
      }
      ex[A + ST_PG] = wgt * pg;
      ex[A + ST_KL] = wgt * ((ratio - 1.0f) - lr);
      ex[A + ST_CLIP] = (ratio > a.clip_hi || ratio < a.clip_lo) ? 1.0f : 0.0f;
    } else {
      for (int j = 0; j < A; ++j) head[row * S + j] = 0.0f;
    }
    if (A & 1) head[row * S + A] = 0.0f;
    if (in_rows) {
      a.logp[e] = policy::canon32(lp);
      a.ratio[e] = policy::canon32(ratio);
    }
  }
  wave_sync();
  backward(part, wt, a.wt_actor, a.p.actor, tile, S, a.p.activation, first, lane);
  // log_std and the statistics: x is the ones column of the first tile
  grad_w(part + a.p.log_std, 1, A + STATS, tile + a.p.D, S, extra, a.SE, first, lane);
}

template <bool IO32, bool V32>
__global__ __launch_bounds__(MAX_WAVES * 64) void k_ppo_grad(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int P = a.p.n_params;
  float* w = lds;                                        // [P + W_PAD]
  float* istd = w + P + policy::W_PAD;                   // [STD_PAD]
  float* wt = istd + policy::STD_PAD;                    // [wt_floats]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  float* tile = wt + a.wt_floats + wave * ROWS * (a.n_tiles * a.p.S + a.SE);
  float* extra = tile + a.n_tiles * ROWS * a.p.S;
  const int n4 = a.p.vec4 ? P >> 2 : 0;                  // the staging loop of k_policy
  {
    const float4* src = reinterpret_cast<const float4*>(a.p.params);
    float4* dst = reinterpret_cast<float4*>(w);
    const int step = blockDim.x;
    for (int i = threadIdx.x; i < n4; i += 4 * step) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = src[i + j * step < n4 ? i + j * step : i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j * step < n4) dst[i + j * step] = v[j];
    }
  }
  for (int i = 4 * n4 + threadIdx.x; i < P + policy::W_PAD; i += blockDim.x) w[i] = i < P ? a.p.params[i] : 0.0f;
  if (int(threadIdx.x) < a.p.A) {                        // rule 2
    const float is = float(exp(-double(a.p.params[a.p.log_std + threadIdx.x])));
    istd[threadIdx.x] = is;
    if (blockIdx.x == 0) a.inv_std[threadIdx.x] = policy::canon32(is);
  }
  __syncthreads();
  for (int net = 0; net < 2; ++net) {                    // the transposed copies
    const policy::Net& nn = net ? a.p.critic : a.p.actor;
    const int32_t* off = net ? a.wt_critic : a.wt_actor;
    for (int i = 1; i < nn.n_layers; ++i) {
      const int K = nn.K[i], N = nn.N[i], words = ((N + 1) & ~1) * K;
      const float* src = w + nn.w[i];
      float* dst = wt + off[i];
      for (int f = threadIdx.x; f < words; f += blockDim.x) {
        const int n = f / K, k = f - n * K;
        dst[f] = n < N ? src[k * N + n] : 0.0f;
      }
    }
  }
  __syncthreads();
  const int64_t G = (a.B + a.R - 1) / a.R;
  for (int64_t g = int64_t(blockIdx.x) * waves + wave; g < G; g += int64_t(gridDim.x) * waves) {
    float* part = a.partials + g * (P + STATS);
    const int64_t end = (g + 1) * a.R < a.B ? (g + 1) * a.R : a.B;
    for (int64_t e0 = g * a.R; e0 < end; e0 += ROWS)
      rows_of_wave<IO32, V32>(a, w, istd, wt, tile, extra, part, e0, e0 == g * a.R, lane);
  }
}

// rule 10: grad and the statistics from the partials, in ascending group order
__global__ __launch_bounds__(REDUCE_THREADS) void k_ppo_reduce(ReduceArgs a) {
  const int PP = a.P + STATS;
  const float* cnt = a.partials + a.P + ST_N;
  if (blockIdx.x + 1 < gridDim.x) {
    const int p = blockIdx.x * REDUCE_THREADS + threadIdx.x;
    if (p >= a.P) return;
    const float* src = a.partials + p;
    float s = 0.0f, n = 0.0f;
#pragma unroll 8
    for (int64_t g = 0; g < a.G; ++g) {
      s += src[g * PP];
      n += cnt[g * PP];
    }
    float out = 0.0f;
    if (n != 0.0f) {
      out = s / n;
      if (p >= a.log_std) out -= a.ent_coef;
    }
    a.grad[p] = out;
    return;
  }
  __shared__ float sum[STATS];
  if (threadIdx.x < STATS) {
    const float* src = a.partials + a.P + threadIdx.x;
    float s = 0.0f;
#pragma unroll 8
    for (int64_t g = 0; g < a.G; ++g) s += src[g * PP];
    sum[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float n = sum[ST_N];
  float st[STATS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (n != 0.0f) {
    float H = 0.0f;
    for (int j = 0; j < a.A; ++j) H += a.params[a.log_std + j] + a.ent_const;
    const float pg = sum[ST_PG] / n, v = sum[ST_V] / n;
    st[0] = __fmaf_rn(-a.ent_coef, H, __fmaf_rn(a.vf_coef, v, pg));
    st[1] = pg;
    st[2] = v;
    st[3] = H;
    st[4] = sum[ST_KL] / n;
    st[5] = sum[ST_CLIP] / n;
    st[6] = n;
  }
  for (int i = 0; i < STATS; ++i) a.stats[i] = st[i];
}

}  // namespace ppo
}  // namespace anm
