// anm_policy.hpp -- the diagonal-Gaussian MLP actor-critic whose act() is one launch (anm_policy_act;
// gym_anm_amd/policy.py is the specification, rule numbers below are its).  No step, reset, MPC, rollout or minibatch kernel
// knows of it: it reads an observation array and the environment's timestep / reset_count, in stream order behind the step.
//
//   k_policy   one workgroup of `waves` wavefronts (4, or 2 or 1 where the LDS plan asks for it) per tile of 32 waves
//              environments; where there are more tiles than the device holds workgroups at once, a workgroup takes several,
//              one after the other.  The whole flat parameter vector is staged into LDS once per workgroup, as it lies in
//              memory.  A wavefront owns 32 rows and runs every layer on v_mfma_f32_32x32x2_f32 as Y^T = W^T X^T: the A operand is W[k][n] (lane l: n =
//              n0 + (l & 31), k = 2 s + (l >> 5): consecutive lanes read consecutive words of a weight row), the B operand is
//              the activation x[env = l & 31][k = 2 s + (l >> 5)] from the wavefront's own LDS tile, and the accumulator --
//              loaded with the bias -- holds, in lane (env, h), the outputs n = n0 + (r & 3) + 8 (r >> 2) + 4 h of ITS
//              environment in registers r = 0 .. 15.  On gfx950 the instruction is, bit for bit, the k-ordered fmaf chain of
//              rule 2 (one rounding per product, subnormals kept), k = 2 s before k = 2 s + 1.  One accumulator serves: the
//              instruction's issue interval equals its dependent latency; the operands of four steps are read ahead.  A layer reads one of the wavefront's two tiles and
//              writes the other; the activation of a hidden layer is then applied in place, by one rolled loop.
//              An odd K (only D can be odd) ends with ONE vector fmaf per output on the accumulator registers: a zero-padded
//              k would add +0 * +0 to an accumulator that may hold -0.0 (rule 2).
//              The critic runs first and its value is stored; the observation rows are then loaded again for the
//              actor, whose head stays in its tile for the epilogue: rule 6 by one lane per environment, then the actions and
//              the noise leave LDS by the flat index of the destination (consecutive lanes write consecutive words).
//              The Box-Muller pairs of rule 5 are computed before the first layer, pairs p = h, h + 2, .. on lane (env, h).
//
// No atomics, nothing crosses a workgroup; a wavefront's tile is its own, so after the staging barrier the wavefronts
// only order their OWN LDS traffic (wave_sync).  Rows past E are neither read nor written.
#pragma once

#include <cstdint>

#include "anm_device.hpp"

namespace anm {
namespace policy {

constexpr int MAX_WAVES = 4, ROWS = 32;                 // rows of one wavefront: the 32 columns of the matrix instruction
constexpr int MAX_HIDDEN = 3, MIN_WIDTH = 32, MAX_WIDTH = 256, MAX_D = 256, MAX_A = 64;
constexpr int MAX_LAYERS = MAX_HIDDEN + 1;
constexpr int W_PAD = 32, STD_PAD = 64;                 // floats behind the staged parameters; the std table
constexpr int LDS_BYTES = 160 * 1024;
constexpr uint32_t KEY_DRAW = 0x504F4C4Bu, TAG = 0x504F4C31u;   // rule 5
constexpr int ACT_TANH = 0, ACT_RELU = 1;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Net {
  int32_t n_layers;                 // hidden layers + the head
  int32_t K[MAX_LAYERS], N[MAX_LAYERS];
  int32_t w[MAX_LAYERS], b[MAX_LAYERS];   // offsets into the flat vector
};

struct Args {
  const float* params;
  int32_t n_params;
  Net actor, critic;
  int32_t log_std;                  // offset
  int32_t D, A;
  int32_t S, SA;                    // row strides of the activation tile and of the noise tile (odd)
  int32_t activation, deterministic, critic_only;
  int32_t vec4;                     // params is 16-byte aligned
  float logp0;                      // float32(-0.5 A ln 2 pi)
  uint64_t seed, env_offset;
  const int32_t *reset_count, *timestep;
  const void* obs;
  void *actions, *values, *logp;
  float *noise, *std;
  int64_t E;
};

// floats of the plan with `waves` wavefronts per workgroup (policy.lds_floats)
inline int64_t lds_floats(int64_t n_params, int S, int SA, int waves) {
  return n_params + W_PAD + STD_PAD + int64_t(waves) * ROWS * (2 * S + SA);
}

// a wavefront orders its own LDS traffic: the hardware runs a wavefront's LDS instructions in order, the fence keeps the
// compiler from moving a read above the write of another lane
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rule 3
__device__ inline float tanh32(float x) {
  const float C = 7.90531110763549805f;
  const float c = x > C ? C : (x < -C ? -C : x);
  const float x2 = c * c;
  float p = __fmaf_rn(x2, -2.76076847742355e-16f, 2.00018790482477e-13f);
  p = __fmaf_rn(x2, p, -8.60467152213735e-11f);
  p = __fmaf_rn(x2, p, 5.12229709037114e-08f);
  p = __fmaf_rn(x2, p, 1.48572235717979e-05f);
  p = __fmaf_rn(x2, p, 6.37261928875436e-04f);
  p = __fmaf_rn(x2, p, 4.89352455891786e-03f);
  p = c * p;
  float q = __fmaf_rn(x2, 1.19825839466702e-06f, 1.18534705686654e-04f);
  q = __fmaf_rn(x2, q, 2.26843463243900e-03f);
  q = __fmaf_rn(x2, q, 4.89352518554385e-03f);
  float r = p / q;                                    // (one IEEE division: hipcc's default, no fast-math in this build)
  r = r > 1.0f ? 1.0f : (r < -1.0f ? -1.0f : r);
  return fabsf(x) < 0.0004f ? x : r;
}

__device__ inline float relu32(float x) { return x < 0.0f ? 0.0f : x; }

__device__ inline float canon32(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }
__device__ inline double canon64(float x) { return x != x ? __longlong_as_double(0x7ff8000000000000ll) : double(x); }

template <bool F32>
__device__ inline void store(void* p, int64_t i, float x) {
  if constexpr (F32) static_cast<float*>(p)[i] = canon32(x);
  else static_cast<double*>(p)[i] = canon64(x);
}

// rule 1: the wavefront's observation rows into its tile by the flat index of the source (a row past E: zeros)
template <bool IO32>
__device__ inline void load_rows(const Args& a, float* tile, int64_t e0, int rows, int lane) {
  const int words = rows * a.D;
  int row = 0, col = lane;
  for (int f = lane; f < ROWS * a.D; f += 64) {
    while (col >= a.D) { col -= a.D; ++row; }
    float x = 0.0f;
    if (f < words) {
      const int64_t at = e0 * a.D + f;
      if constexpr (IO32) x = static_cast<const float*>(a.obs)[at];
      else x = float(static_cast<const double*>(a.obs)[at]);
    }
    tile[row * a.S + col] = x;
    col += 64;
  }
}

// words of `rows` rows of width W out of a tile of stride S, by the flat index of the destination
template <bool IO32>
__device__ inline void store_rows(void* dst, const float* tile, int S, int W, int64_t e0, int rows, int lane) {
  const int words = rows * W;
  int row = 0, col = lane;
  for (int f = lane; f < words; f += 64) {
    while (col >= W) { col -= W; ++row; }
    store<IO32>(dst, e0 * W + f, tile[row * S + col]);
    col += 64;
  }
}

// rule 2 (and 3 where `hidden`): one layer of one wavefront, from its tile `in` to its tile `out`
__device__ inline void layer(const float* Wt, const float* bias, int K, int N, const float* in, float* out, int S, int activation,
                             bool hidden, int lane) {
  const int env = lane & 31, h = lane >> 5;
  const float* x = in + env * S + h;
  const int Ke = K & ~1;
  for (int n0 = 0; n0 < N; n0 += 32) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      acc[r] = n < N ? bias[n] : 0.0f;
    }
    // a lane whose n = n0 + env is past N (a head) reads what follows in the staged vector -- parameters or the zero pad,
    // inside LDS -- into a row of the product that is never stored
    const float* wa = Wt + h * N + n0 + env;
    int k = 0;
    for (; k + 8 <= Ke; k += 8) {                              // four steps: their eight operands are read before the first
      float wv[4], xv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wv[j] = wa[(k + 2 * j) * N];
        xv[j] = x[k + 2 * j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[j], xv[j], acc, 0, 0, 0);
    }
    for (; k < Ke; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[k * N], x[k], acc, 0, 0, 0);
    if (K & 1) {
      const float xb = in[env * S + K - 1];
      const float* wrow = Wt + (K - 1) * N;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (n < N) acc[r] = __fmaf_rn(xb, wrow[n], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (n < N) out[env * S + n] = acc[r];
    }
  }
  wave_sync();
  if (!hidden) return;
  // rule 3, in place: lane (env, h) takes the outputs n = h, h + 2, .. of its environment (one copy of the function's code
  // in a rolled loop, where the accumulator registers would take sixteen)
  float* y = out + env * S;
  if (activation == ACT_TANH) {
#pragma unroll 4
    for (int n = h; n < N; n += 2) y[n] = tanh32(y[n]);
  } else {
#pragma unroll 4
    for (int n = h; n < N; n += 2) y[n] = relu32(y[n]);
  }
  wave_sync();
}

// the layers of a net from tile 0, alternating between the two tiles: the result is in the tile returned
__device__ inline float* run_net(const float* w, const Net& net, float* tile, int S, int activation, int lane) {
  float* in = tile;
  float* out = tile + ROWS * S;
  for (int i = 0; i < net.n_layers; ++i) {
    layer(w + net.w[i], w + net.b[i], net.K[i], net.N[i], in, out, S, activation, i + 1 < net.n_layers, lane);
    float* t = in;
    in = out;
    out = t;
  }
  return in;
}

// rule 5: the pairs p = h, h + 2, .. of environment row `env` into the noise tile
__device__ inline void draw_noise(const Args& a, float* eps, int64_t e, int env, int h) {
  const int pairs = (a.A + 1) >> 1;
  uint32_t kq[4];
  Philox::generate(a.seed, a.env_offset + uint64_t(e), uint32_t(a.reset_count[e]), KEY_DRAW, kq);
  const uint64_t key = uint64_t(kq[0]) | (uint64_t(kq[1]) << 32);
  const uint32_t t = uint32_t(a.timestep[e]);
  for (int p = h; p < pairs; p += 2) {
    uint32_t q[4];
    Philox::generate(key, uint64_t(t) | (uint64_t(uint32_t(p)) << 32), 0u, TAG, q);
    const double u1 = 1.0 - Philox::u01(q[0], q[1]);
    const double u2 = Philox::u01(q[2], q[3]);
    const double r = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    double sn, cs;
    sincos_medium(ang, sn, cs);
    const double zc = r * cs, zs = r * sn;
    eps[env * a.SA + 2 * p] = float(zc);
    if (2 * p + 1 < a.A) eps[env * a.SA + 2 * p + 1] = float(zs);
  }
}

// one tile of 32 rows of one wavefront: rules 1 to 7
template <bool IO32, bool V32>
__device__ inline void rows_of_wave(const Args& a, const float* w, const float* stdv, float* tile, float* eps, int64_t e0, int lane) {
  const int rows = a.E - e0 < ROWS ? int(a.E - e0) : ROWS;
  const int env = lane & 31, h = lane >> 5;
  const bool live = env < rows;

  if (!a.critic_only) {
    if (a.deterministic) {
      for (int j = h; j < a.A; j += 2) eps[env * a.SA + j] = 0.0f;
    } else if (live) {
      draw_noise(a, eps, e0 + env, env, h);
    }
  }

  load_rows<IO32>(a, tile, e0, rows, lane);
  wave_sync();
  const float* val = run_net(w, a.critic, tile, a.S, a.activation, lane);
  if (live && h == 0) store<V32>(a.values, e0 + env, val[env * a.S]);
  wave_sync();
  if (a.critic_only) return;

  load_rows<IO32>(a, tile, e0, rows, lane);
  wave_sync();
  float* head = run_net(w, a.actor, tile, a.S, a.activation, lane);
  if (live && h == 0) {                                // rule 6
    const float* ls = w + a.log_std;
    float lp = a.logp0;
    for (int j = 0; j < a.A; ++j) {
      const float mean = head[env * a.S + j], e = eps[env * a.SA + j];
      head[env * a.S + j] = __fmaf_rn(stdv[j], e, mean);
      const float he = -0.5f * e;
      lp = __fmaf_rn(he, e, lp);
      lp = __fsub_rn(lp, ls[j]);
    }
    store<V32>(a.logp, e0 + env, lp);
  }
  wave_sync();
  store_rows<IO32>(a.actions, head, a.S, a.A, e0, rows, lane);
  store_rows<true>(a.noise, eps, a.SA, a.A, e0, rows, lane);
  wave_sync();                                         // (the next tile of this wavefront writes the same LDS)
}

template <bool IO32, bool V32>
__global__ __launch_bounds__(MAX_WAVES * 64) void k_policy(Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* w = lds;                                      // [n_params + W_PAD]: the flat parameter vector
  float* stdv = lds + a.n_params + W_PAD;              // [STD_PAD]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  float* tile = stdv + STD_PAD + wave * ROWS * (2 * a.S + a.SA);   // two tiles [ROWS][S]
  float* eps = tile + 2 * ROWS * a.S;                  // [ROWS][SA]
  // the parameters, staged once per workgroup: 16-byte words where the vector is aligned (a.vec4), four loads of a lane in
  // flight; then the tail and the zero pad by single words
  const int n4 = a.vec4 ? a.n_params >> 2 : 0;
  {
    const float4* src = reinterpret_cast<const float4*>(a.params);
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
  for (int i = 4 * n4 + threadIdx.x; i < a.n_params + W_PAD; i += blockDim.x) w[i] = i < a.n_params ? a.params[i] : 0.0f;
  if (int(threadIdx.x) < a.A) {                        // rule 4
    const float sd = float(exp(double(a.params[a.log_std + threadIdx.x])));
    stdv[threadIdx.x] = sd;
    if (blockIdx.x == 0 && !a.critic_only) a.std[threadIdx.x] = canon32(sd);
  }
  __syncthreads();
  // the tiles of this workgroup: the grid is the number of workgroups the device holds at once, or fewer
  const int64_t per_tile = int64_t(waves) * ROWS;
  for (int64_t e0 = int64_t(blockIdx.x) * per_tile + int64_t(wave) * ROWS; e0 < a.E; e0 += int64_t(gridDim.x) * per_tile)
    rows_of_wave<IO32, V32>(a, w, stdv, tile, eps, e0, lane);
}

}  // namespace policy
}  // namespace anm
