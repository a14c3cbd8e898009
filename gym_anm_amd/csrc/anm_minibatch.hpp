// anm_minibatch.hpp -- the minibatch sampler of the device rollout buffer (anm_minibatch_prepare / _gather;
// gym_anm_amd/minibatch.py is the specification, rule numbers below are its).  No step, reset, MPC or rollout kernel knows
// of it: the kernels here read what anm_rollout_gae / _adv_norm left, in stream order behind them.
//
//   k_mb_count    one workgroup of 256 lanes per aligned range of the flat index k E + e (rollout::slab_range): the number
//                 of valid slots of the range, by ballots and popcounts
//   k_mb_scan     one workgroup: the exclusive scan of the range counts, n, and one lane adds 1 to rollout_count
//   k_mb_scatter  one workgroup per range: a valid slot's rank within its range from the ballots (the chunks before it
//                 in its wavefront, the wavefronts before it through LDS), index[offset + rank] = s; lane s writes
//                 index[s] = -1 where s >= n (rule 1)
//   k_mb_gather   one launch per minibatch, one workgroup per tile of 64 rows: the first wavefront walks the permutation
//                 of rule 2 and loads `index` ONCE per row and parks the row's slot in LDS; then every lane copies words
//                 by the FLAT index of the destination tile (consecutive lanes write consecutive words, the lanes of a
//                 row read consecutive words of the source row), the row and word of a lane advanced by a host-computed
//                 quotient and remainder per trip -- no division per word; the loads of four trips are issued before the
//                 first store.  The six scalars of a row are one wavefront each.
//
// Everything is integers and copies of bits.  The counts are integer sums, so nothing depends on the grid; results pass
// between workgroups across the launch boundary alone: no atomics, no tickets, no flags.
#pragma once

#include <cstdint>
#include <type_traits>

#include "anm_device.hpp"
#include "anm_rollout.hpp"

namespace anm {
namespace minibatch {

constexpr int LANES = 256, WAVES = 4;
constexpr int SCAN_RUN = rollout::MAX_SLABS / LANES;   // range counts a lane of k_mb_scan takes: 16
constexpr int TILE = 64;                                // rows of one workgroup of k_mb_gather
constexpr int FLIGHT = 4;                               // trips whose loads are issued before the first store
constexpr uint32_t MB_TAG = 0x4D425348u;                // rule 2
constexpr int MIN_WIDTH = 8, ROUNDS = 4;
constexpr int ST_NVALID = 0, ST_COUNT = 1, ST_SIZE = 2; // the state block: int64 n_valid, rollout_count

// ---- prepare (rule 1) -----------------------------------------------------------------------------------------------------------
struct PrepArgs {
  const uint8_t* flags;   // [N]
  int32_t* index;         // [N]
  int32_t* counts;        // [n_ranges]
  int32_t* offsets;       // [n_ranges]
  long long* state;       // [ST_SIZE]
  int64_t N;
  int64_t range;          // slots of a range: rollout::slab_range(N)
  int n_ranges;
};

// valid slots of the chunk of 64 slots at `first`, as a ballot (a slot past N is not valid and is not read)
__device__ inline uint64_t chunk_ballot(const PrepArgs& a, int64_t first, int lane) {
  const int64_t i = first + lane;
  const bool valid = i < a.N && (a.flags[i] & rollout::F_VALID) != 0;
  return __ballot(valid);
}

// valid slots of this wavefront's quarter of the range of its workgroup; four chunks' loads in flight
__device__ inline int quarter_count(const PrepArgs& a, int64_t base, int live, int lane) {
  int n = 0;
  for (int c0 = 0; c0 < live; c0 += 4) {
    uint64_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = chunk_ballot(a, base + int64_t(c0 + j) * 64, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) n += __popcll(b[j]);
  }
  return n;
}

// chunks of a quarter that hold a slot below N (uniform over the wavefront)
__device__ inline int live_chunks(const PrepArgs& a, int64_t base, int chunks) {
  const int64_t left = a.N - base;
  return left <= 0 ? 0 : (left >= int64_t(chunks) * 64 ? chunks : int((left + 63) / 64));
}

__global__ __launch_bounds__(LANES) void k_mb_count(PrepArgs a) {
  __shared__ int part[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int chunks = int(a.range / (WAVES * 64));   // of this wavefront: 4 .. 64
  const int64_t base = int64_t(blockIdx.x) * a.range + int64_t(w) * chunks * 64;
  const int n = quarter_count(a, base, live_chunks(a, base, chunks), lane);
  if (lane == 0) part[w] = n;
  __syncthreads();
  if (threadIdx.x == 0) a.counts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(LANES) void k_mb_scan(PrepArgs a) {
  __shared__ int wave_sum[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int first = int(threadIdx.x) * SCAN_RUN;   // this lane's run of range counts
  int c[SCAN_RUN];
  int own = 0;
#pragma unroll
  for (int j = 0; j < SCAN_RUN; ++j) {
    c[j] = first + j < a.n_ranges ? a.counts[first + j] : 0;
    own += c[j];
  }
  int incl = own;   // inclusive scan over the wavefront
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_sum[w] = incl;
  __syncthreads();
  int before = incl - own;
  for (int v = 0; v < w; ++v) before += wave_sum[v];
#pragma unroll
  for (int j = 0; j < SCAN_RUN; ++j) {
    if (first + j < a.n_ranges) a.offsets[first + j] = before;
    before += c[j];
  }
  if (threadIdx.x == 0) {
    a.state[ST_NVALID] = (long long)((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]));
    a.state[ST_COUNT] += 1;
  }
}

__global__ __launch_bounds__(LANES) void k_mb_scatter(PrepArgs a) {
  __shared__ int part[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int chunks = int(a.range / (WAVES * 64));
  const int64_t base = int64_t(blockIdx.x) * a.range + int64_t(w) * chunks * 64;
  const int live = live_chunks(a, base, chunks);
  const int mine = quarter_count(a, base, live, lane);
  if (lane == 0) part[w] = mine;
  __syncthreads();
  int64_t at = a.offsets[blockIdx.x];   // where this wavefront's first valid slot goes
  for (int v = 0; v < w; ++v) at += part[v];
  const int64_t n = a.state[ST_NVALID];
  const uint64_t below = (uint64_t(1) << lane) - 1;
  for (int c0 = 0; c0 < live; c0 += 4) {
    uint64_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = chunk_ballot(a, base + int64_t(c0 + j) * 64, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t s = base + int64_t(c0 + j) * 64 + lane;
      const int64_t to = at + __popcll(b[j] & below);
      if (((b[j] >> lane) & 1) && to < a.N) a.index[to] = int32_t(s);   // (to < n <= N while the flags stand still)
      if (s < a.N && s >= n) a.index[s] = -1;
      at += __popcll(b[j]);
    }
  }
}

// ---- gather (rules 2 and 3) -----------------------------------------------------------------------------------------------------
struct GatherArgs {
  const void *obs, *actions, *logp, *values, *returns, *adv;   // the sources: [T, E, D], [T, E, A], [T, E] x 4
  const int32_t* index;                                        // [N]
  const long long* state;                                      // [ST_SIZE]
  void *mb_obs, *mb_actions, *mb_logp, *mb_values, *mb_returns, *mb_adv, *mb_weight;   // [B, D], [B, A], [B] x 5
  int32_t* mb_slot;                                            // [B]
  int64_t N;
  int64_t first;         // m B: the position of row 0
  int32_t B, D, A;
  int32_t dq, dr, dm;    // LANES / D, LANES % D: what a trip adds to a lane's row and word; ceil(2^16 / D): the first row
  int32_t aq, ar, am;    // the same for A
  uint32_t ep;
  uint64_t seed;
};

// F(r, v) of rule 2
__device__ inline uint32_t feistel_f(const GatherArgs& a, uint32_t count, int r, uint32_t v) {
  uint32_t q[4];
  Philox::generate(a.seed, uint64_t(v) | (uint64_t(a.ep) << 32), count, MB_TAG + uint32_t(r), q);
  return q[0];
}

// rule 2: the image of p < n under the permutation of [0, n) of (seed, rollout_count, ep).  The walk carries its bound,
// 2^b - n + 1 passes, as the trip limit.
__device__ inline uint32_t perm(const GatherArgs& a, uint32_t count, uint32_t n, uint32_t p) {
  const int bl = 32 - __clz(int(n - 1));
  const int b = bl < MIN_WIDTH ? MIN_WIDTH : bl;
  const int lo_bits = b / 2, hi_bits = b - lo_bits;
  const uint32_t lo_mask = (1u << lo_bits) - 1, hi_mask = (1u << hi_bits) - 1;
  uint32_t x = p;
  for (uint32_t left = (1u << b) - n + 1; left != 0; --left) {
    uint32_t lo = x & lo_mask, hi = x >> lo_bits;
#pragma unroll
    for (int r = 0; r < ROUNDS; r += 2) {
      hi ^= feistel_f(a, count, r, lo) & hi_mask;
      lo ^= feistel_f(a, count, r + 1, hi) & lo_mask;
    }
    x = (hi << lo_bits) | lo;
    if (x < n) break;
  }
  return x;
}

// The words of `rows` rows of width W copied into the destination tile by its flat index.  slot[]: the source row of each
// row of the tile, -1 for a padding row (all-zero words).  q, r: LANES / W and LANES % W; m = ceil(2^16 / W), which gives
// f / W = f m >> 16 for every f < 256 (the error f (m W - 2^16) stays below 2^16; above W = 256 both sides are 0).
template <class Word>
__device__ inline void copy_rows(const void* src_, void* dst_, const int* slot, int rows, int W, int q, int r, int m) {
  const Word* src = static_cast<const Word*>(src_);
  Word* dst = static_cast<Word*>(dst_);
  const int words = rows * W;
  int f = threadIdx.x;
  int row = (f * m) >> 16, word = f - row * W;
  while (f < words) {                    // (ends at the same trip for the lanes of a wavefront, up to the last one)
    Word x[FLIGHT];
    int at[FLIGHT], s[FLIGHT];
#pragma unroll
    for (int j = 0; j < FLIGHT; ++j) {
      at[j] = f;
      s[j] = slot[f < words ? row : 0];
      // no branch around the load, and nothing reads it before the stores: the four stay in flight.  A padding row and a
      // trip past the tile load from row 0 (in bounds; word < W always) and the select below drops what came
      x[j] = src[int64_t(s[j] < 0 ? 0 : s[j]) * W + word];
      f += LANES;
      row += q;
      word += r;
      if (word >= W) { word -= W; row += 1; }
    }
#pragma unroll
    for (int j = 0; j < FLIGHT; ++j)
      if (at[j] < words) dst[at[j]] = s[j] >= 0 ? x[j] : Word(0);
  }
}

template <bool IO32, bool V32>
__global__ __launch_bounds__(LANES) void k_mb_gather(GatherArgs a) {
  using IoWord = typename std::conditional<IO32, uint32_t, uint64_t>::type;
  using VWord = typename std::conditional<V32, uint32_t, uint64_t>::type;
  __shared__ int slot[TILE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row0 = int(blockIdx.x) * TILE;                       // of this tile, within the minibatch
  const int rows = a.B - row0 < TILE ? a.B - row0 : TILE;        // >= 1 by the grid
  if (w == 0) {
    long long n = a.state[ST_NVALID];
    n = n < 0 ? 0 : (n > a.N ? a.N : n);                          // (a state block nobody prepared reads no slot past the buffers)
    const int64_t p = a.first + row0 + lane;
    int s = -1;
    if (lane < rows && p < n) {
      s = a.index[perm(a, uint32_t(a.state[ST_COUNT]), uint32_t(n), uint32_t(p))];
      if (s < 0 || s >= a.N) s = -1;
    }
    slot[lane] = s;
  }
  __syncthreads();
  const size_t io = sizeof(IoWord), vw = sizeof(VWord);
  copy_rows<IoWord>(a.obs, static_cast<char*>(a.mb_obs) + size_t(row0) * a.D * io, slot, rows, a.D, a.dq, a.dr, a.dm);
  copy_rows<IoWord>(a.actions, static_cast<char*>(a.mb_actions) + size_t(row0) * a.A * io, slot, rows, a.A, a.aq, a.ar, a.am);
  if (lane >= rows) return;
  const int s = slot[lane];
  const int i = row0 + lane;
  const VWord one = V32 ? VWord(0x3f800000u) : VWord(0x3ff0000000000000ull);
  auto scalar = [&](const void* src, void* dst) {
    static_cast<VWord*>(dst)[i] = s >= 0 ? static_cast<const VWord*>(src)[s] : VWord(0);
  };
  if (w == 0) {   // (uniform over a wavefront: the six scalars of a row are spread over the four)
    scalar(a.logp, a.mb_logp);
    a.mb_slot[i] = s;
  } else if (w == 1) {
    scalar(a.values, a.mb_values);
    static_cast<VWord*>(a.mb_weight)[i] = s >= 0 ? one : VWord(0);
  } else if (w == 2) {
    scalar(a.returns, a.mb_returns);
  } else {
    scalar(a.adv, a.mb_adv);
  }
}

}  // namespace minibatch
}  // namespace anm
