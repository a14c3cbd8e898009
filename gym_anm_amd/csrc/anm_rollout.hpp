// anm_rollout.hpp -- the device rollout buffer of an on-policy loop (anm_rollout_begin / _add / _gae / _adv_norm;
// gym_anm_amd/rollout.py is the specification, rule numbers below are its).  No step, reset or MPC kernel knows of it: the
// kernels here read what a step call stored, in stream order behind it.
//
//   k_rollout_store  one launch per add / begin: the [E, D] observation block copied flat into its slot, and per row the
//                    reward copy, the classification of rule 2, the flags byte and t_seen
//   k_rollout_gae    one lane per environment, a reverse sweep over the slots (rule 3): the loads of BLK slots are issued a
//                    block ahead of the recurrence that consumes them
//   k_adv_partial    one workgroup of 256 lanes per aligned power-of-two range of the flat index k E + e: the leaves of
//                    rule 4 summed by its fixed tree, one slab [S1, S2, n] per workgroup
//   k_adv_finish     one workgroup: the slabs summed by the same tree (padded by +0.0 slabs), the statistics
//   k_adv_apply      adv_norm from the statistics
//
// The tree is that of anm_io_norm.hpp (node i = node 2i + node 2i+1 over the index padded by +0.0 to a power of two), walked by
// the same xor butterfly: the lanes of a wavefront are the low six bits of the flat index, the chunks of 64 leaves a wavefront
// takes the next bits (chunk c's sum is parked in lane c, then one more butterfly), the four wavefronts the next two, the slabs
// the rest.  A leaf is never -0.0, so padding further than the specification does adds +0.0 to a node that it leaves as it
// is.  Results pass between workgroups across the launch boundary alone: no tickets, no flags, no float atomics.
#pragma once

#include <cstdint>
#include <type_traits>

#include "anm_io_norm.hpp"

namespace anm {
namespace rollout {

using ionorm::butterfly;

constexpr int F_VALID = 1, F_TERMINATED = 2, F_TRUNCATED = 4;   // the flags byte (rule 2)
constexpr int STORE_LANES = 256;
constexpr int GAE_LANES = 64;   // one wavefront per workgroup: 65 536 environments are one wavefront per SIMD
constexpr int BLK = 16;         // slots whose loads are in flight while the block before them is consumed
constexpr int ADV_LANES = 256, ADV_WAVES = 4;
constexpr int64_t MIN_RANGE = 1024, MAX_RANGE = 16384;   // leaves of a slab: 256 lanes x (4 .. 64 chunks per wavefront) / 4
constexpr int MAX_SLABS = 4096;   // k_adv_finish: 64 lanes x an aligned run of at most 64 slabs each
constexpr int64_t MAX_LEAVES = MAX_SLABS * MAX_RANGE;
constexpr int SLAB = 3;           // S1, S2, n (an exact integer)
// the statistics block: six float64, then two int64
constexpr int ST_N = 0, ST_MEAN = 1, ST_VAR = 2, ST_STD = 3, ST_DEN = 4, ST_OK = 5, ST_NVALID = 6, ST_NSKIPPED = 7, ST_SIZE = 8;

// leaves of one slab: the smallest power of two from MIN_RANGE up that keeps the slab count within MAX_SLABS
constexpr ANM_HD int64_t slab_range(int64_t N) {
  int64_t r = MIN_RANGE;
  while (r < MAX_RANGE && (N + r - 1) / r > MAX_SLABS) r <<= 1;
  return r;
}

template <bool F32>
__device__ double load_f(const void* p, int64_t i) {
  if constexpr (F32) return double(static_cast<const float*>(p)[i]);
  else return static_cast<const double*>(p)[i];
}

// one rounding to the stored format; a NaN is stored as the canonical quiet NaN (sign 0, payload 0), chosen on the bits
template <bool F32>
__device__ void store_f(void* p, int64_t i, double x) {
  if constexpr (F32) {
    const uint32_t b = __float_as_uint(float(x));
    static_cast<uint32_t*>(p)[i] = (b & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : b;
  } else {
    const uint64_t b = uint64_t(__double_as_longlong(x));
    static_cast<uint64_t*>(p)[i] = (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull ? 0x7ff8000000000000ull : b;
  }
}

// ---- begin / add (rules 1 and 2) ----------------------------------------------------------------------------------------
struct StoreArgs {
  const void* src_obs;         // [E, D] what the step (or the reset) stored
  void* dst_obs;               // slot k + 1 (begin: slot 0) of obs
  int64_t n_obs;               // E D
  const void* reward;          // [E]
  void* dst_reward;            // slot k of rewards
  const uint8_t* terminated;   // [E]
  const uint8_t* truncated;    // [E] or null
  const int32_t* timestep;     // [E]
  uint8_t* flags;              // slot k of flags
  int32_t* t_seen;             // [E]
  int64_t E;
  int begin;                   // 1: obs and t_seen only
};

template <bool F32>
__global__ __launch_bounds__(STORE_LANES) void k_rollout_store(StoreArgs a) {
  using Word = typename std::conditional<F32, uint32_t, uint64_t>::type;   // (a copy of bits: no conversion, no canonicalisation)
  const int64_t i = int64_t(blockIdx.x) * STORE_LANES + threadIdx.x;
  if (i < a.n_obs) static_cast<Word*>(a.dst_obs)[i] = static_cast<const Word*>(a.src_obs)[i];
  if (i >= a.E) return;
  const int32_t t = a.timestep[i];
  if (a.begin == 0) {
    int f = (t != a.t_seen[i] && t != 0) ? F_VALID : 0;   // a real step; else: an autoreset, a failed draw, the absorbing no-op
    if (a.terminated[i] != 0) f |= F_TERMINATED;
    if (a.truncated && a.truncated[i] != 0) f |= F_TRUNCATED;
    a.flags[i] = uint8_t(f);
    static_cast<Word*>(a.dst_reward)[i] = static_cast<const Word*>(a.reward)[i];
  }
  a.t_seen[i] = t;
}

// ---- GAE (rule 3) -------------------------------------------------------------------------------------------------------------
struct GaeArgs {
  const void* rewards;    // [T, E]
  const void* values;     // [T + 1, E]
  const uint8_t* flags;   // [T, E]
  void* advantages;       // [T, E]
  void* returns;          // [T, E]
  int64_t T, E;
  double g, gl;           // gamma, gamma * gae_lambda
};

// a block of slots as loaded: the widening waits for the data, so it belongs to the consumer, a block later
template <bool RF32, bool VF32>
struct GaeBlock {
  using R = typename std::conditional<RF32, float, double>::type;
  using V = typename std::conditional<VF32, float, double>::type;
  R r[BLK];
  V v[BLK];
  uint8_t f[BLK];
};

// the slots top, top - 1, ... of environment e; below slot 0 the load repeats slot 0 (in bounds, never consumed)
template <bool RF32, bool VF32>
__device__ void gae_load(const GaeArgs& a, int64_t e, int64_t top, GaeBlock<RF32, VF32>& b) {
#pragma unroll
  for (int j = 0; j < BLK; ++j) {
    const int64_t k = top - j < 0 ? 0 : top - j;
    const int64_t i = k * a.E + e;
    b.r[j] = static_cast<const typename GaeBlock<RF32, VF32>::R*>(a.rewards)[i];
    b.v[j] = static_cast<const typename GaeBlock<RF32, VF32>::V*>(a.values)[i];
    b.f[j] = a.flags[i];
  }
}

template <bool RF32, bool VF32>
__device__ void gae_consume(const GaeArgs& a, int64_t e, int64_t top, const GaeBlock<RF32, VF32>& b, double& v_next, double& a_next) {
#pragma unroll
  for (int j = 0; j < BLK; ++j) {
    const int64_t k = top - j;
    if (k < 0) break;   // (uniform)
    const double r = double(b.r[j]), v = double(b.v[j]);
    const bool valid = (b.f[j] & F_VALID) != 0, term = (b.f[j] & F_TERMINATED) != 0, trunc = (b.f[j] & F_TRUNCATED) != 0;
    const double boot = fma(a.g, v_next, r);
    const double delta = (term ? r : boot) - v;
    const double start = valid ? delta : 0.0;          // what the slot holds when the trace does not run through it
    const double run = fma(a.gl, a_next, delta);
    const double adv = (!valid || term || trunc) ? start : run;
    const double sum = adv + v;
    const int64_t i = k * a.E + e;
    store_f<VF32>(a.advantages, i, adv);
    store_f<VF32>(a.returns, i, valid ? sum : 0.0);
    a_next = adv;
    v_next = v;
  }
}

template <bool RF32, bool VF32>
__global__ __launch_bounds__(GAE_LANES) void k_rollout_gae(GaeArgs a) {
  const int64_t e = int64_t(blockIdx.x) * GAE_LANES + threadIdx.x;
  if (e >= a.E) return;
  double v_next = load_f<VF32>(a.values, a.T * a.E + e), a_next = 0.0;
  GaeBlock<RF32, VF32> b0, b1;
  int64_t top = a.T - 1;
  gae_load(a, e, top, b0);
  while (true) {   // (uniform: every lane of the launch makes the same trips)
    if (top >= BLK) gae_load(a, e, top - BLK, b1);
    gae_consume(a, e, top, b0, v_next, a_next);
    top -= BLK;
    if (top < 0) break;
    if (top >= BLK) gae_load(a, e, top - BLK, b0);
    gae_consume(a, e, top, b1, v_next, a_next);
    top -= BLK;
    if (top < 0) break;
  }
}

// ---- advantage moments and normalisation (rule 4) ---------------------------------------------------------------------------------
struct AdvArgs {
  const void* advantages;   // [N] the flat index k E + e
  const uint8_t* flags;     // [N]
  void* adv_norm;           // [N]
  int64_t N;
  int64_t range;            // leaves of a slab: slab_range(N)
  double* slabs;            // [n_slabs][SLAB]
  int n_slabs;
  double* stats;            // [ST_SIZE]
  double eps;
};

template <bool VF32>
__global__ __launch_bounds__(ADV_LANES) void k_adv_partial(AdvArgs a) {
  __shared__ double part[ADV_WAVES][2];
  __shared__ int npart[ADV_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int chunks = int(a.range / (ADV_WAVES * 64));   // of this wavefront: 4 .. 64, a power of two
  const int64_t base = int64_t(blockIdx.x) * a.range + int64_t(w) * chunks * 64;
  double k1 = 0.0, k2 = 0.0;   // lane c keeps the sums of chunk c
  int n = 0;
  const int64_t left = a.N - base;   // (uniform: the chunks past the end are +0.0 leaves, and stay out of the loop)
  const int live = left <= 0 ? 0 : (left >= int64_t(chunks) * 64 ? chunks : int((left + 63) / 64));
  for (int c0 = 0; c0 < live; c0 += 4) {   // the loads of four chunks in flight
    double x[4];
    int f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t i = base + int64_t(c0 + j) * 64 + lane;
      const bool in = i < a.N;
      x[j] = in ? load_f<VF32>(a.advantages, i) : 0.0;
      f[j] = in ? int(a.flags[i]) : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = (f[j] & F_VALID) != 0;
      const double x0 = x[j] + 0.0, xx = x[j] * x[j];
      double l1 = valid ? x0 : 0.0, l2 = valid ? xx : 0.0;
      n += __popcll(__ballot(valid));
      l1 = butterfly<6>(l1);
      l2 = butterfly<6>(l2);
      if (lane == c0 + j) { k1 = l1; k2 = l2; }
    }
  }
  k1 = butterfly<6>(k1);   // the chunks of the wavefront (the lanes past them hold +0.0)
  k2 = butterfly<6>(k2);
  if (lane == 0) { part[w][0] = k1; part[w][1] = k2; npart[w] = n; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int v = threadIdx.x;
    double* slab = a.slabs + int64_t(blockIdx.x) * SLAB;
    slab[v] = (part[0][v] + part[1][v]) + (part[2][v] + part[3][v]);
    if (v == 0) slab[2] = double(npart[0] + npart[1] + npart[2] + npart[3]);
  }
}

__device__ inline double canonical(double x) {
  const uint64_t b = uint64_t(__double_as_longlong(x));
  return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull ? __longlong_as_double(0x7ff8000000000000ll) : x;
}

__global__ __launch_bounds__(ADV_LANES) void k_adv_finish(AdvArgs a) {
  __shared__ double tot[SLAB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int pow2 = 64;
  while (pow2 < a.n_slabs) pow2 <<= 1;
  const int run = pow2 / 64;
  if (w < SLAB) {   // one wavefront per entry: a lane's aligned run of slabs, then the butterfly
    const int first = lane * run;
    double x = ionorm::slab_tree(a.slabs + int64_t(first) * SLAB + w, SLAB, a.n_slabs - first, run);
    x = butterfly<6>(x);
    if (lane == 0) tot[w] = x;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = tot[2];
  double m = 0.0, var = 0.0, sd = 0.0, den = 1.0;
  bool ok = false;
  if (n >= 2.0) {
    m = tot[0] / n;
    const double q = tot[1] / n;
    const double t = fma(-m, m, q);
    const double vb = t < 0.0 ? 0.0 : t;   // (a NaN passes, and the normalisation is skipped)
    const double bessel = n / (n - 1.0);
    var = vb * bessel;
    sd = sqrt(var);
    den = sd + a.eps;
    ok = isfinite(m) && isfinite(sd);
  }
  a.stats[ST_N] = n;
  a.stats[ST_MEAN] = canonical(m);
  a.stats[ST_VAR] = canonical(var);
  a.stats[ST_STD] = canonical(sd);
  a.stats[ST_DEN] = canonical(den);
  a.stats[ST_OK] = ok ? 1.0 : 0.0;
  long long* counts = reinterpret_cast<long long*>(a.stats);
  counts[ST_NVALID] = (long long)n;
  if (!ok) counts[ST_NSKIPPED] += 1;
}

template <bool VF32>
__global__ __launch_bounds__(ADV_LANES) void k_adv_apply(AdvArgs a) {
  using Word = typename std::conditional<VF32, uint32_t, uint64_t>::type;
  const int64_t i = int64_t(blockIdx.x) * ADV_LANES + threadIdx.x;
  if (i >= a.N) return;
  if (a.stats[ST_OK] == 0.0) {   // skipped: a copy of the advantages, bit for bit
    static_cast<Word*>(a.adv_norm)[i] = static_cast<const Word*>(a.advantages)[i];
    return;
  }
  const double m = a.stats[ST_MEAN], den = a.stats[ST_DEN];
  const double x = load_f<VF32>(a.advantages, i);
  const double y = (x - m) / den;
  store_f<VF32>(a.adv_norm, i, (a.flags[i] & F_VALID) != 0 ? y : 0.0);
}

}  // namespace rollout
}  // namespace anm
