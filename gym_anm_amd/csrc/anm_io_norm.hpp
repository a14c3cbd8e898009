// anm_io_norm.hpp -- running observation / return normalisation kept on the device (anm_model_io_norm_update;
// gym_anm_amd/io_norm.py is the specification, rule numbers below are its).  No step or reset kernel changes: they read the
// block behind EnvIO::iomap at launch, and the two kernels here rewrite `scale`, `bias` and `reward_scale` in that block,
// in stream order between steps, from statistics they keep in float64.
//
//   k_norm_partial   one workgroup of 256 lanes per aligned range of 256 rows (1024 above 262 144 environments, so that there
//                    are never more than 4096 slabs): the per-row return accumulator (rule 7) and the leaves (rule 3), summed
//                    by the fixed tree of rule 4; one slab per workgroup [n, nr, SG1, SG2 | S1[D] | S2[D]]
//   k_norm_finish    one workgroup of 256 lanes: the slabs summed by the same tree (padded by +0.0 slabs), then one lane per
//                    column for rules 5, 6 and 1, one lane for the return part and the counts
//
// The sum is ONE tree whatever the grid: node i = node 2i + node 2i+1 over the environment index padded by +0.0 to a power of
// two.  IEEE addition commutes, so an xor butterfly (both partners form the same sum) walks it; a leaf is never -0.0 (rule 3),
// so neither is a node, and padding further than the spec does -- to the rows of a workgroup, to 64 slabs -- adds +0.0 to a node that it
// leaves as it is.  Results pass between workgroups across the launch boundary alone: no tickets, no flags, no float atomics.
#pragma once

#include <cstdint>

namespace anm {
namespace ionorm {

constexpr int LANES = 256, WAVES = 4;   // lanes of a workgroup of k_norm_partial
constexpr int SUB = 64;      // rows of the tile a wavefront stages at a time; TILES (1 | 4) tiles: its 64 | 256 rows
constexpr int FINISH_LANES = 256, FINISH_WAVES = 4;   // (more lanes: a smaller register budget, and the long slab runs spill)
constexpr int64_t SMALL_BATCH = 262144;   // up to here a workgroup takes 256 rows (one tile per wavefront), above 1024
constexpr ANM_HD int rows_per_group(int64_t E) { return E <= SMALL_BATCH ? WAVES * SUB : 4 * WAVES * SUB; }
constexpr int CT = 24;       // columns of a tile: D <= CT is ONE tile, whose 64 rows are one contiguous stretch of obs
constexpr int MAX_SLABS = 4096;   // k_norm_finish: 64 lanes x an aligned run of at most 64 slabs each
// the statistics block (float64, device): a head, then mean, var and the tables they give (a mirror of what the block
// behind EnvIO::iomap holds, for the caller to read)
constexpr int ST_CNT = 0, ST_RCNT = 1, ST_RMEAN = 2, ST_RVAR = 3, ST_RSCALE = 4, ST_HEAD = 8;
// a slab (float64): counts (exact integers), the return sums, then S1[D], S2[D]
constexpr int SL_N = 0, SL_NR = 1, SL_G1 = 2, SL_G2 = 3, SL_HEAD = 4;
constexpr int CN_UPDATES = 0, CN_SKIPPED = 1;   // the int64 counters

constexpr ANM_HD int slab_doubles(int D) { return SL_HEAD + 2 * D; }
constexpr ANM_HD int stat_doubles(int D) { return ST_HEAD + 4 * D; }

struct Args {
  const void* obs;             // [E, D] float64 | float32: what the step stored
  const void* reward;          // [E]
  const uint8_t* terminated;   // [E]
  const uint8_t* truncated;    // [E] or null
  const int32_t* timestep;     // [E]
  double* iomap;               // the block the step kernels read (IoMap): reward_scale, ..., scale[D], bias[D]
  int off_scale;               // IoMap::obs(A): where scale starts in it; bias at off_scale + D
  int D;
  int64_t E;
  double* stats;               // [stat_doubles(D)]
  long long* counters;         // [2]
  double* slabs;               // [n_slabs][slab_doubles(D)]
  int n_slabs;
  double* G;                   // [E] discounted-return accumulator
  int32_t* t_seen;             // [E]
  double gamma, eps;
  int obs_on, reward_on;
};

// where entry (row, col) of a wavefront's tile sits: rows of CT doubles, and two doubles more every four rows, so that the
// lanes of a half-wave, which read rows 4q + j of columns p and p + 1 in one instruction, are 4 CT + 2 = 98 = 2 (mod 32)
// doubles apart and hit 32 different bank pairs; the staging writes are consecutive addresses
ANM_HD int tile_at(int row, int col) { return row * CT + col + 2 * (row >> 2); }
constexpr int TILE_DOUBLES = SUB * CT + 2 * (SUB / 4);

ANM_HD double rule1_scale(double var, double eps) { return 1.0 / sqrt(var + eps); }
ANM_HD double rule1_bias(double mean, double scale) {
  const double ms = mean * scale;   // (a statement of its own: no contraction into the subtraction)
  return 0.0 - ms;
}

template <bool F32>
__device__ double load_io(const void* p, int64_t i) {
  if constexpr (F32) return double(static_cast<const float*>(p)[i]);
  else return static_cast<const double*>(p)[i];
}

// both partners of every exchange form the same sum: the tree of rule 4 over the lanes of a group of 2^STEPS lanes
template <int STEPS>
__device__ double butterfly(double v) {
#pragma unroll
  for (int x = 1; x < (1 << STEPS); x <<= 1) v = v + __shfl_xor(v, x);
  return v;
}

// the TILES partial sums of a wavefront, in tree order
template <int TILES, class P>
__device__ double tiles_tree(P&& p) {
  if constexpr (TILES == 1) return p(0);
  else return (p(0) + p(1)) + (p(2) + p(3));
}

template <bool F32, int TILES>
__global__ __launch_bounds__(LANES) void k_norm_partial(Args a) {
  static_assert(TILES == 1 || TILES == 4);
  constexpr int ROWS = WAVES * SUB * TILES;
  __shared__ double tile[WAVES][TILE_DOUBLES];
  __shared__ double part[WAVES][TILES][2 * CT];   // [wave][tile of the wave]: S1 of the tile's columns, then S2
  __shared__ double gpart[WAVES][TILES][2];
  __shared__ int npart[WAVES][2];
  __shared__ uint8_t counted[WAVES][TILES][SUB];  // rule 3: the rows whose observation counts

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int D = a.D;
  const int64_t wave_row0 = int64_t(blockIdx.x) * ROWS + w * (ROWS / WAVES);
  double* slab = a.slabs + int64_t(blockIdx.x) * slab_doubles(D);

  // ---- the rows: one lane per row, tile after tile (rules 3 and 7) ----
  {
    const double rs = a.iomap[0];   // IoMap::REWARD: the reward_scale the step used
    int n_obs = 0, n_ret = 0;
#pragma unroll
    for (int s = 0; s < TILES; ++s) {
      const int64_t e = wave_row0 + s * SUB + lane;
      const bool in = e < a.E;
      const bool term = in && a.terminated[e] != 0;
      const bool c_obs = in && !term && a.obs_on != 0;
      counted[w][s][lane] = c_obs ? 1 : 0;
      n_obs += __popcll(__ballot(c_obs));
      double l1 = 0.0, l2 = 0.0;
      bool c_ret = false;
      if (in && a.reward_on != 0) {
        const int32_t t = a.timestep[e], seen = a.t_seen[e];
        if (t == seen) {
          // an absorbing no-op, a failed reset draw: nothing happened to this row
        } else if (t == 0) {   // an in-kernel autoreset
          a.G[e] = 0.0;
          a.t_seen[e] = 0;
        } else {
          const double r = load_io<F32>(a.reward, e) / rs;
          const double g = fma(a.gamma, a.G[e], r);
          l1 = g + 0.0;
          l2 = g * g;
          c_ret = true;
          const bool over = term || (a.truncated && a.truncated[e] != 0);
          a.G[e] = over ? 0.0 : g;
          a.t_seen[e] = t;
        }
      }
      n_ret += __popcll(__ballot(c_ret));
      l1 = butterfly<6>(l1);
      l2 = butterfly<6>(l2);
      if (lane == 0) { gpart[w][s][0] = l1; gpart[w][s][1] = l2; }
    }
    if (lane == 0) { npart[w][0] = n_obs; npart[w][1] = n_ret; }
  }
  __syncthreads();
  if (threadIdx.x < 2) {   // SG1, SG2: the tiles of a wavefront, then the four wavefronts
    const int v = threadIdx.x;
    double t[WAVES];
#pragma unroll
    for (int k = 0; k < WAVES; ++k) t[k] = tiles_tree<TILES>([&](int s) { return gpart[k][s][v]; });
    slab[SL_G1 + v] = (t[0] + t[1]) + (t[2] + t[3]);
    slab[SL_N + v] = double(npart[0][v] + npart[1][v] + npart[2][v] + npart[3][v]);
  }
  if (a.obs_on == 0) return;   // (uniform: the observation part is off, its slab entries are never read)

  // ---- the columns, CT at a time ----
  const int q = lane & 15, p = lane >> 4;   // the lane sums rows 4q .. 4q + 3 of the columns p, p + 4, ... of a tile
  for (int c0 = 0; c0 < D; c0 += CT) {
    const int ct = D - c0 < CT ? D - c0 : CT;
#pragma unroll 1
    for (int s = 0; s < TILES; ++s) {
      const int64_t row0 = wave_row0 + s * SUB;
      const int64_t left = a.E - row0;
      const int rows = left < 0 ? 0 : (left < SUB ? int(left) : SUB);
      // stage: consecutive lanes read consecutive addresses (ct == D: the whole tile is one stretch of obs)
      for (int i = lane; i < SUB * ct; i += 64) {
        const int row = i / ct, col = i - row * ct;
        tile[w][tile_at(row, col)] = row < rows ? load_io<F32>(a.obs, (row0 + row) * D + c0 + col) : 0.0;
      }
      __syncthreads();
      for (int col = p; col < ct; col += 4) {
        double l1[4], l2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = 4 * q + j;
          const double y = tile[w][tile_at(row, col)];
          const bool c = counted[w][s][row] != 0;
          const double y0 = y + 0.0, yy = y * y;
          l1[j] = c ? y0 : 0.0;
          l2[j] = c ? yy : 0.0;
        }
        double s1 = (l1[0] + l1[1]) + (l1[2] + l1[3]);
        double s2 = (l2[0] + l2[1]) + (l2[2] + l2[3]);
        s1 = butterfly<4>(s1);   // the 16 lanes of a DPP row: 64 rows
        s2 = butterfly<4>(s2);
        if (q == 0) { part[w][s][col] = s1; part[w][s][CT + col] = s2; }
      }
      __syncthreads();
    }
    // the tiles of a wavefront, then the four wavefronts
    for (int v = threadIdx.x; v < 2 * ct; v += LANES) {
      const int h = v >= ct ? 1 : 0, col = v - h * ct;
      double t[WAVES];
#pragma unroll
      for (int k = 0; k < WAVES; ++k) t[k] = tiles_tree<TILES>([&](int s) { return part[k][s][h * CT + col]; });
      slab[SL_HEAD + h * D + c0 + col] = (t[0] + t[1]) + (t[2] + t[3]);
    }
    __syncthreads();
  }
}

// the tree over an aligned run of N slabs (N a power of two), entry p[i * stride] of slab i; a slab that is not there is +0.0
template <int N>
__device__ double run_tree(const double* p, int64_t stride, int avail) {
  if constexpr (N == 1) {
    return avail > 0 ? p[0] : 0.0;
  } else {
    const double lo = run_tree<N / 2>(p, stride, avail);
    const double hi = run_tree<N / 2>(p + (N / 2) * stride, stride, avail - N / 2);
    return lo + hi;
  }
}

__device__ inline double slab_tree(const double* p, int64_t stride, int avail, int run) {
  switch (run) {
    case 1: return run_tree<1>(p, stride, avail);
    case 2: return run_tree<2>(p, stride, avail);
    case 4: return run_tree<4>(p, stride, avail);
    case 8: return run_tree<8>(p, stride, avail);
    case 16: return run_tree<16>(p, stride, avail);
    case 32: return run_tree<32>(p, stride, avail);
    default: return run_tree<64>(p, stride, avail);
  }
}

// rules 5 (already in raw space: mo, vo) and 6 on one set of statistics; false: not finite, nothing changes
__device__ inline bool merge(double mo, double vo, double n, double cnt, double& mean, double& var) {
  if (!(isfinite(mo) && isfinite(vo))) return false;
  const double tot = cnt + n, wgt = n / tot;
  const double d = mo - mean;
  const double dd = d * d, cw = cnt * wgt, vn = vo * n;
  const double m2 = fma(dd, cw, fma(var, cnt, vn));
  mean = fma(d, wgt, mean);
  var = m2 / tot;
  return true;
}

__global__ __launch_bounds__(FINISH_LANES) void k_norm_finish(Args a) {
  extern __shared__ double tot[];   // [slab_doubles(D)] the roots, then one int: the columns skipped
  const int D = a.D, V = slab_doubles(D);
  int* skipped = reinterpret_cast<int*>(tot + V);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int pow2 = 64;
  while (pow2 < a.n_slabs) pow2 <<= 1;
  const int run = pow2 / 64;
  if (threadIdx.x == 0) *skipped = 0;
  const int used = a.obs_on != 0 ? V : SL_HEAD;   // (observation part off: its slab entries were never written)
  for (int v = w; v < used; v += FINISH_WAVES) {   // one wavefront per entry: a lane's aligned run of slabs, then the butterfly
    const int first = lane * run;
    double x = slab_tree(a.slabs + int64_t(first) * V + v, V, a.n_slabs - first, run);
    x = butterfly<6>(x);
    if (lane == 0) tot[v] = x;
  }
  const double cnt = a.stats[ST_CNT];
  __syncthreads();
  const double n = tot[SL_N], nr = tot[SL_NR];
  double* mean = a.stats + ST_HEAD;
  double* var = mean + D;
  double* scale = var + D;
  double* bias = scale + D;
  if (a.obs_on != 0 && n > 0.0) {
    for (int k = threadIdx.x; k < D; k += FINISH_LANES) {
      const double s = a.iomap[a.off_scale + k], b = a.iomap[a.off_scale + D + k];   // the tables the step used
      const double my = tot[SL_HEAD + k] / n, qy = tot[SL_HEAD + D + k] / n;
      const double t = fma(-my, my, qy);
      const double vy = t < 0.0 ? 0.0 : t;   // (a NaN passes, and the column is skipped)
      const double ss = s * s;
      const double mo = (my - b) / s, vo = vy / ss;
      double m = mean[k], vr = var[k];
      if (!merge(mo, vo, n, cnt, m, vr)) {
        atomicAdd(skipped, 1);
        continue;
      }
      const double sc = rule1_scale(vr, a.eps), bi = rule1_bias(m, sc);
      mean[k] = m;
      var[k] = vr;
      scale[k] = sc;
      bias[k] = bi;
      a.iomap[a.off_scale + k] = sc;
      a.iomap[a.off_scale + D + k] = bi;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int skip = *skipped;
    if (a.obs_on != 0 && n > 0.0) a.stats[ST_CNT] = cnt + n;
    if (a.reward_on != 0 && nr > 0.0) {
      const double my = tot[SL_G1] / nr, qy = tot[SL_G2] / nr;
      const double t = fma(-my, my, qy);
      const double vy = t < 0.0 ? 0.0 : t;
      const double rcnt = a.stats[ST_RCNT];
      double m = a.stats[ST_RMEAN], vr = a.stats[ST_RVAR];
      if (merge(my, vy, nr, rcnt, m, vr)) {
        const double sc = rule1_scale(vr, a.eps);
        a.stats[ST_RMEAN] = m;
        a.stats[ST_RVAR] = vr;
        a.stats[ST_RCNT] = rcnt + nr;
        a.stats[ST_RSCALE] = sc;
        a.iomap[0] = sc;
      } else {
        skip += 1;
      }
    }
    a.counters[CN_UPDATES] += 1;
    a.counters[CN_SKIPPED] += skip;
  }
}

// rule 1 alone: the tables of a statistics block (construction, a loaded checkpoint)
__global__ __launch_bounds__(LANES) void k_norm_tables(Args a) {
  const int D = a.D;
  double* mean = a.stats + ST_HEAD;
  double* var = mean + D;
  double* scale = var + D;
  double* bias = scale + D;
  if (a.obs_on != 0) {
    for (int k = threadIdx.x; k < D; k += LANES) {
      const double sc = rule1_scale(var[k], a.eps), bi = rule1_bias(mean[k], sc);
      scale[k] = sc;
      bias[k] = bi;
      a.iomap[a.off_scale + k] = sc;
      a.iomap[a.off_scale + D + k] = bi;
    }
  }
  if (a.reward_on != 0 && threadIdx.x == 0) {
    const double sc = rule1_scale(a.stats[ST_RVAR], a.eps);
    a.stats[ST_RSCALE] = sc;
    a.iomap[0] = sc;
  }
}

}  // namespace ionorm
}  // namespace anm
