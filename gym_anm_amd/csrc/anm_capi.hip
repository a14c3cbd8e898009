// anm_capi.hip -- gfx950 kernels + the C ABI of include/anm_mi355x.h for ONE network topology
// (the descriptor header is injected with -DANM_TOPO_HEADER=...; see gym_anm_amd/codegen.py).
//
// Launch shapes: 64-thread workgroups = one wavefront each (the general family: up to 512 lanes per environment above 65
// buses), so that a diverging Newton-Raphson solve only ever holds back the other environments of its own wavefront and
// workgroups spread round-robin over the 8 XCDs; no inter-workgroup traffic.  Thread family: one thread per environment,
// LDS for the coalesced row transposes and the in-wave hand-over slots; lane-group families: one environment per group of
// lanes, hand-overs and Jacobian blocks in LDS.  HBM traffic per environment step is the action row in and the obs /
// reward rows out (~250 B for ANM6Easy); the network constants are wave-uniform scalar loads that stay in the scalar cache
// (thread family) or per-lane tables (lane groups).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include ANM_TOPO_HEADER
#include "anm_devbuf.hpp"
#include "anm_env_ops.hpp"
#include "anm_io_norm.hpp"
#include "anm_rollout.hpp"
#include "anm_minibatch.hpp"
#include "anm_policy.hpp"
#include "anm_policy_grad.hpp"
#include "anm_pack.hpp"
#include "anm_radial.hpp"
#include "anm_mesh.hpp"
#include "anm_mpc.hpp"

using namespace anm;

#include "anm_mpc_capi_types.inc"

namespace {

constexpr int BLOCK = 64;

thread_local std::string g_err;

int fail(const char* what) {
  g_err = what;
  return -1;
}
int fail_hip(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return -2;
}

// (in-wave hand-over point; end of round 6, with the lane-group trip at half a thread-mode trip: 5 / 6 / 7 -> 73.7 / 74.3 / 74.8 us
// per step at 65 536 environments, four rounds, profiles/r06_z_handoff.txt.  6 stays: it is also where the two-launch step of the
// larger batches hands over, and the two step modes are bit-identical under the automatic policy only at the same point --
// a batch's results must not depend on its size.)
#ifndef ANM_HANDOFF_DEFAULT
#define ANM_HANDOFF_DEFAULT 6
#endif
// (ANM_MID_CAP_DEFAULT, where the first straggler launch leaves the solves still running to the second: anm_group.hpp)
#ifndef ANM_ROWS_WAVES
#define ANM_ROWS_WAVES 1  // min. waves per SIMD the step kernel is compiled for (register budget 512 / waves)
#endif

// VIEW: the launch serves the environments a batch view names (anm_model_bind_view); without one the view is a compile-time
// identity and costs the kernels nothing
// START: the launch honours anm_model_bind_nr_start (an instantiation of its own, always with VIEW: see op_transition)
template <class JT, bool VIEW = false, bool START = false>
__global__ __launch_bounds__(BLOCK) void k_transition(cptr_t C0, TransitionIO io, SolverOpts so, int64_t n, ClassSel cs, View v) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[Topo::TREE != 0 ? group::Shape<Topo>::NG * group::Slot<Topo>::SIZE : 1];
  const int64_t e0 = int64_t(blockIdx.x) * BLOCK + threadIdx.x;
  const bool valid = e0 < n;
  const int64_t e = valid ? e0 : n - 1;
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  if constexpr (VIEW) op_transition<Topo, JT, START>(C, io, so, e, v, valid, lds);
  else op_transition<Topo, JT>(C, io, so, e, View{}, valid, lds);
#endif
}

template <class JT, bool VIEW = false>
__global__ __launch_bounds__(BLOCK) void k_reset(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs, View v) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[Topo::TREE != 0 ? group::Shape<Topo>::NG * group::Slot<Topo>::SIZE : 1];
  const int64_t e0 = int64_t(blockIdx.x) * BLOCK + threadIdx.x;
  const bool valid = e0 < n;
  const int64_t e = valid ? e0 : n - 1;
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  if constexpr (VIEW) op_reset<Topo, JT>(C, io, so, e, v, valid, lds);
  else op_reset<Topo, JT>(C, io, so, e, View{}, valid, lds);
#endif
}

// the step of the environments a batch view names (thread-per-environment family): see op_step_view.
// SW: wavefronts per SIMD the registers are budgeted for -- 1: 288 registers; 2: 256 + 80 bytes of scratch, the faster
// kernel once the batch gives every SIMD more than two wavefronts (two ANM6 models, 524 288 environments: 385 -> 315 us;
// 131 072: 219 -> 223; 16 384, where the step waits for one diverging solve: 124 -> 139.  profiles/r05_k_view_step.txt)
template <class JT, int SW>
__global__ __launch_bounds__(BLOCK, SW) void k_step_view(cptr_t C, EnvIO io, SolverOpts so, int64_t n, View v) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[Topo::TREE != 0 ? group::Shape<Topo>::NG * group::Slot<Topo>::SIZE : 1];
  op_step_view<Topo, JT>(C, io, so, n, v, lds);
#endif
}

// fast path of the step (series mode, K = 1, "state" observation): see op_step_rows
template <class JT, bool FULL>
__global__ __launch_bounds__(BLOCK, ANM_ROWS_WAVES) void k_step_rows(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[64 * (Topo::SDIM + 2)];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_rows<Topo, JT, FULL>(C, io, so, n, lds);
#endif
}

// the fast path with the episode time limit and statistics (anm_env_config.max_episode_steps / .episode): a kernel of its
// own, so that k_step_rows carries none of it
template <class JT>
__global__ __launch_bounds__(BLOCK, ANM_ROWS_WAVES) void k_step_rows_ep(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[64 * (Topo::SDIM + 2)];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_rows<Topo, JT, false, true>(C, io, so, n, lds);
#endif
}

// the fast path with float32 action, obs and reward I/O (anm_model_set_io, ANM_IO_F32), without and with the episode
// time limit and statistics: kernels of their own under their own names, so that k_step_rows / k_step_rows_ep carry none of it
template <class JT, bool EP>
__global__ __launch_bounds__(BLOCK, ANM_ROWS_WAVES) void k_step_rows_io32(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[64 * (Topo::SDIM + 2)];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_rows<Topo, JT, false, EP, true>(C, io, so, n, lds);
#endif
}

// the fast path through the affine I/O map (anm_model_set_io_map), float64 or float32 arrays: again kernels of their own,
// the four above carry none of it.  The episode settings are served at run time (io.ep.on, as in k_step_rows_ep): two
// instantiations per solve precision, not four
template <class JT, bool IO32>
__global__ __launch_bounds__(BLOCK, ANM_ROWS_WAVES) void k_step_rows_map(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[64 * (Topo::SDIM + 2)];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_rows<Topo, JT, false, true, IO32, true>(C, io, so, n, lds);
#endif
}

// general step (host next_vars, K != 1, list-form observations, `full` dump): see op_step_general
template <class JT>
__global__ __launch_bounds__(BLOCK) void k_step_general(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  extern __shared__ double lds_dyn[];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_general<Topo, JT>(C, io, so, n, lds_dyn);
#endif
}
// ... with the expected forecast written beside the state rows (io.forecast bound).  A kernel of its own: a task without
// the forecast keeps k_step_general's instruction stream
template <class JT>
__global__ __launch_bounds__(BLOCK) void k_step_general_fc(cptr_t C0, EnvIO io, SolverOpts so, int64_t n, ClassSel cs) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY
  extern __shared__ double lds_dyn[];
  const cptr_t C = class_constants(C0, cs, int64_t(blockIdx.x) * BLOCK);
  op_step_general<Topo, JT, true>(C, io, so, n, lds_dyn);
#endif
}

template <class JT, bool GROUPS>
__global__ __launch_bounds__(BLOCK) void k_step_stragglers(cptr_t C, EnvIO io, SolverOpts so, int level) {
#ifndef ANM_DEV_LANE_GROUPS_ONLY   // (tuning builds of the lane-group kernels alone: minutes less to compile)
  __shared__ double lds[GROUPS ? group::Shape<Topo>::NG * group::Slot<Topo>::SIZE : 1];
  op_step_stragglers<Topo, JT, GROUPS>(C, io, so, lds, level);
#endif
}

__global__ void k_step_scatter(EnvIO io) { op_step_scatter<Topo>(io); }

// anm_test_row_dpp: the row hand-over helpers of anm_group.hpp on one wavefront, each result a row of 64 doubles
__global__ __launch_bounds__(64) void k_test_row_dpp(const double* __restrict__ acc, const double* __restrict__ x,
                                                     double* __restrict__ out) {
  const int l = threadIdx.x;
  const double a = acc[l], v = x[l];
  double one = 1.0;
  asm volatile("" : "+v"(one));
  double s0 = a, s1 = a;
  group::row_wsum<5, 0x5>(s0, s1, v, v, one);
  double t0 = a, t1 = a;
  group::row_wsum<0, 0x1, 7, 0x2, 15, 0xC>(t0, t1, v, v, one);
  double m0 = a, m1 = a;
  group::row_mov<12, 0xA>(m0, m1, v, v);
  Blk<double> D{a, a, a, a};
  double r0 = a, r1 = a;
  group::row_fold<3, 0x8>(D, r0, r1, Blk<double>{v, v, v, v}, v, v, one);
  // (row_fma takes the two entries of a {ja, jb, -jb, ja} block: a0 = (a - ja v) - jb v of the first call, and of the
  // second a1 = (a + jb v) - ja v with jb = -16, ja = 8 -- the chain whose first product carries no negation)
  double b0 = a, b1 = a, u0 = a, u1 = a;
  group::row_fma<9, 0x3>(b0, u0, v, v, 2.0, 4.0);
  group::row_fma<9, 0x3>(u1, b1, v, v, 8.0, -16.0);
  out[l] = s0; out[64 + l] = s1; out[128 + l] = t1; out[192 + l] = m0; out[256 + l] = m1;
  out[320 + l] = D.a; out[384 + l] = D.d; out[448 + l] = r1; out[512 + l] = b0; out[576 + l] = b1;
}

// obs[e, k] = clip(src(e, index[k]) * scale[k], low[k], high[k]); src is the `full` row for
// index < full_dim and the aux tail of the state row beyond it; terminated environments observe 0
// (anm_env.py:365-367, 442-446)
__global__ void k_gather_obs(int64_t n, int full_dim, const double* __restrict__ full, int state_dim, int K,
                             const double* __restrict__ state, const uint8_t* __restrict__ terminated, int n_obs,
                             const int32_t* __restrict__ index, const double* __restrict__ scale,
                             const double* __restrict__ low, const double* __restrict__ high,
                             double* __restrict__ obs) {
  const int64_t total = n * n_obs;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t e = t / n_obs;
    const int k = int(t - e * n_obs);
    const int idx = index[k];
    const double src = (idx < full_dim) ? full[e * full_dim + idx] : state[e * state_dim + (state_dim - K) + (idx - full_dim)];
    const double v = fmin(fmax(src * scale[k], low[k]), high[k]);
    obs[t] = (terminated && terminated[e]) ? 0.0 : v;
  }
}

// ANM6Easy.init_state (anm6_easy.py:25-52) for any series-mode task, the draws alone: one thread per environment, table-driven
// (tab[d] = type, slot, q_min, q_max, soc_min, soc_max of device d), the very expressions of the samplers inside the reset /
// step kernels (sample_init_state, anm_lane_io.inc) -- tests/test_gpu_sampler.py holds them to it bit for
// bit.  raw (nullable): the Philox words behind the row, blocks 0 .. n_blocks - 1 of key (seed, env_offset + e, epoch).
__global__ void k_sample_init_state(int64_t n, int nd, int nload, int ngen, int ndes, const double* __restrict__ tab,
                                    const double* __restrict__ series, int period, uint64_t seed, uint64_t env_offset,
                                    const int32_t* __restrict__ reset_count, double* __restrict__ out, uint32_t* __restrict__ raw,
                                    int n_blocks, const double* __restrict__ exo_lo, const double* __restrict__ exo_noise) {
  // exo_lo != null: the uniform exogenous mode (low ends [nload + ngen], the high ends behind them) -- step index 0, loads
  // and generator P / P_max from the step stream at index 0 instead of the series, block 0 unused
  // exo_noise != null (with exo_lo, the clip ends): the noisy time series -- the time index from block 0 as in series mode,
  // loads and generator P / P_max by ExoNoise at that index and step index 0
  const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int W = 2 * nd + ndes + ngen + 1;
  const uint32_t epoch = reset_count ? uint32_t(reset_count[e]) : 0u;
  int aux = 0;
  uint64_t key = 0;
  const int nexo = nload + ngen;
  const bool noisy = exo_noise != nullptr, uni = exo_lo && !noisy;
  if (exo_lo) key = ExoUniform::episode_key(seed, env_offset + uint64_t(e), epoch);
  if (!uni) {
    uint32_t r[4];
    Philox::generate(seed, env_offset + uint64_t(e), epoch, 0u, r);
    aux = int((uint64_t(r[0]) * uint64_t(period)) >> 32);
  }
  auto drawn = [&](int unit) {   // unit `unit` of the mode's step stream at step index 0
    if (noisy) return ExoNoise::draw(key, 0u, unit, exo_noise[unit * period + aux], series[unit * period + aux], exo_lo[unit], exo_lo[nexo + unit]);
    return ExoUniform::draw(key, 0u, unit, exo_lo[unit], exo_lo[nexo + unit]);
  };
  double* s0 = out + e * W;
  for (int k = 0; k < W; ++k) s0[k] = 0.0;
  s0[W - 1] = double(aux);
  for (int d = 0; d < nd; ++d) {
    const double* t = tab + 6 * d;
    const int typ = int(t[0]), slot = int(t[1]);
    if (typ == DEV_LOAD) {
      s0[d] = exo_lo ? drawn(slot) : series[slot * period + aux];
    } else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE || typ == DEV_STORAGE) {
      const bool des = typ == DEV_STORAGE;
      const double uu = Philox::unit_u01(seed, env_offset + uint64_t(e), epoch, des ? ngen + slot : slot);
      if (des) {
        s0[2 * nd + slot] = t[4] + (t[5] - t[4]) * uu;
      } else {
        const double pm = exo_lo ? drawn(nload + slot) : series[(nload + slot) * period + aux];
        s0[d] = pm;
        s0[2 * nd + ndes + slot] = pm;
        s0[nd + d] = t[2] + (t[3] - t[2]) * uu;
      }
    }
  }
  if (raw)
    for (int b = 0; b < n_blocks; ++b) {
      uint32_t q[4];
      Philox::generate(seed, env_offset + uint64_t(e), epoch, uint32_t(b), q);
      for (int k = 0; k < 4; ++k) raw[(e * n_blocks + b) * 4 + k] = q[k];
    }
}

// The parameter tables of one kernel family: class 0 (the network the model was created from) on the host where the
// family's packer writes it, classes 1.. (anm_model_set_classes: same topology, other numbers), and the device buffer
// that holds all of them back to back, class k at k * h0.size() doubles
struct Tables {
  std::vector<double>& h0;      // h_const (Layout<Topo>) | plan.hd | mplan.hd
  const char* copy_what;        // error texts: of an upload, of the reallocation for more classes
  const char* alloc_what;
  bool ok = false;              // the family can serve this model
  int off_obs_lo = 0, off_obs_hi = 0;   // where the observation bounds [SDIM + K] sit in a class's table
  std::vector<std::vector<double>> extra;
  DevBuf<int> dev_int;          // lane-group families: the int tables of the plan (the topology: one copy for all classes)
  DevBuf<double> dev;
};

}  // namespace

struct anm_model {
  int impl = ANM_IMPL_THREAD;   // which kernel family serves this model
  int impl_unbound = -1;        // the family to go back to when a per-environment class binding is lifted (-1: none pending)
  radial::View view{};          // anm_model_bind_view: the launches serve a sub-batch of a larger, padded batch
  bool has_view = false;
  int view_waves = 0;   // k_step_view variant: 0 = by batch size; 1 | 2 (ANM_VIEW_WAVES, read at anm_model_create: tuning, tests)
  // the shape of the network, from the first family that took it: the compiled topology, else the radial plan, else the
  // general one (where two families have it they agree: all three derive it from the same description)
  anm_dims dims{};              // (action_dim = 2 n_set: the devices with set-points are the generators and the storage units)
  FullOffsets full{};           // rows of the `full` dump
  std::vector<double> h_const;  // constants of the compiled topology (Layout<Topo>)
  radial::Plan plan;            // per-lane tables of the lane-group kernel
  mesh::Plan mplan;             // ... of the general lane-group kernel
  mesh::Launch mlaunch{2, 1, true, 0, 0};
  // .ok: the network has the topology this library was compiled for | is a tree that fits one wavefront | is one the
  // general lane-group kernel can take
  Tables t_thread{h_const, "hipMemcpy(constants)", "hipMalloc(class constants)"};
  Tables t_radial{plan.hd, "hipMemcpy(radial tables)", "hipMalloc(class tables)"};
  Tables t_mesh{mplan.hd, "hipMemcpy(mesh tables)", "hipMalloc(class tables)"};
  DevBuf<double> d_series;      // device exogenous series [NEXO][period]
  int period = 0;
  int K = 0;
  bool env_set = false;
  // list-form observation (anm_model_set_obs)
  int n_obs = 0;
  unsigned obs_need = 0;
  int obs_row_stride = 0, obs_aux_off = 0;   // compact row layout (only the classes the list reads)
  short obs_cls_off[FC_COUNT] = {0};
  DevBuf<int32_t> d_obs_index;               // [2][n_obs]: compact-layout indices, identity-layout indices
  DevBuf<double> d_obs_tab;                  // [3][n_obs]: scale, low, high
  const int32_t* d_env_class = nullptr;       // caller's device array [num_envs] (anm_model_bind_env_classes)
  bool class_per_env = false;                 // the classes do not come in aligned blocks of 64 environments
  uint8_t* d_state_same = nullptr;            // caller's device array [num_envs] (anm_model_bind_state_same)
  double* d_nr_diff = nullptr;                // caller's device array [num_envs] (anm_model_bind_nr_diff)
  const double* d_nr_start = nullptr;         // caller's device array [num_envs, 2 (n_bus - 1)] (anm_model_bind_nr_start)
  DevBuf<int32_t> d_zero;                     // one zero: the class of every environment when no classes are bound
  DevBuf<double> d_samp;                      // [n_dev][6] sampler table (anm_sample_init_state_f64)
  int s_nd = 0, s_nload = 0, s_ngen = 0, s_ndes = 0;
  // uniform exogenous mode and noisy time series (anm_env_config.exo_mode)
  int exo_mode = ANM_EXO_HOST;
  std::vector<double> exo_default;            // [2][n_load + n_gen] MW: loads [p_min, 0], generators [0, p_max]
  DevBuf<double> d_exo;                       // [2][n_load + n_gen] MW: low, high of every unit
  DevBuf<double> d_noise;                     // noisy time series: [n_load + n_gen][period] MW amplitudes
  DevBuf<double> d_corr;                      // ... correlated (anm_env_config_corr): [2][n_load + n_gen] rho, then sqrt(1 - rho^2)
  double* exo_z = nullptr;                    // ... the caller's noise states [E][n_load + n_gen] (device; not owned)
  DevBuf<ExoForecastIO> d_forecast;           // ... the expected forecast (anm_env_config_forecast; null: off): the block the kernels
                                              // read -- the tables above, exo_z and the caller's rows [E][n_load + n_gen][H] (not owned)
  EpisodeIO ep{};                             // episode time limit and statistics (anm_env_config.max_episode_steps / .episode)
  int io_mode = ANM_IO_F64;                   // anm_model_set_io: float32 action / obs / reward arrays
  DevBuf<double> d_iomap;                     // anm_model_set_io_map (null: off): the block of IoMap the kernels read
  std::vector<cplx> ybus;

  std::array<Tables*, 3> tables() { return {&t_thread, &t_radial, &t_mesh}; }
  int n_classes() const { return 1 + int(std::max(std::max(t_thread.extra.size(), t_radial.extra.size()), t_mesh.extra.size())); }
};

// FullState<Topo> is full_offsets() at the counts of Topo, and the compiled topology counts action and state rows like
// the lane-group plans (build_plan): whichever family fills the shape of a model, it is the same shape
static_assert(full_offsets_match<Topo>());
static_assert(Dims<Topo>::ADIM == 2 * Topo::NSET && Topo::SDIM == 2 * Topo::ND + Topo::NDES + Topo::NGEN);

namespace {

// (const_doubles: Layout<Topo>::TOTAL | the plan's n_double)
void set_shape(anm_model* m, int NB, int ND, int NBR, int NLOAD, int NGEN, int NDES, int SDIM, int const_doubles) {
  m->full = full_offsets(NB, ND, NDES, NGEN, NBR);
  m->dims = anm_dims{NB, ND, NBR, NLOAD, NGEN, NDES, 2 * (NGEN + NDES), SDIM, m->full.base[FC_COUNT], const_doubles};
}

// device copies of a lane-group plan: its int tables and room for the doubles of class 0
bool alloc_plan(Tables& t, const std::vector<int>& hi) {
  return t.dev_int.assign(hi.data(), hi.size()) == hipSuccess && t.dev.alloc(t.h0.size()) == hipSuccess;
}

// an upload into a buffer of its own; the two error texts: of the allocation, of the copy
template <class T>
int stage(DevBuf<T>& b, const T* host, size_t count, size_t pad_bytes, const char* alloc_what, const char* copy_what) {
  const hipError_t e = b.assign(host, count, pad_bytes);
  return e == hipSuccess ? 0 : fail_hip(e, b.get() ? copy_what : alloc_what);
}

int upload(Tables& t) {
  if (!t.ok) return 0;
  const size_t n = t.h0.size();
  hipError_t e = hipMemcpy(t.dev.get(), t.h0.data(), n * sizeof(double), hipMemcpyHostToDevice);
  for (size_t k = 0; k < t.extra.size() && e == hipSuccess; ++k)
    e = hipMemcpy(t.dev.get() + (k + 1) * n, t.extra[k].data(), n * sizeof(double), hipMemcpyHostToDevice);
  return e == hipSuccess ? 0 : fail_hip(e, t.copy_what);
}

int upload_const(anm_model* m) {
  for (Tables* t : m->tables())
    if (int rc = upload(*t)) return rc;
  return 0;
}

// the device buffer for n_classes consecutive copies (the old one stays when there is no room for the new)
int reallocate(Tables& t, int n_classes) {
  if (!t.ok) return 0;
  DevBuf<double> p;
  hipError_t e = p.alloc(size_t(n_classes) * t.h0.size());
  if (e != hipSuccess) return fail_hip(e, t.alloc_what);
  t.dev = std::move(p);
  return 0;
}

void set_obs_bounds(Tables& t, int cls, int n, const double* low, const double* high) {
  if (!t.ok) return;
  std::vector<double>& h = cls == 0 ? t.h0 : t.extra[cls - 1];
  for (int k = 0; k < n; ++k) { h[t.off_obs_lo + k] = low[k]; h[t.off_obs_hi + k] = high[k]; }
}

// the task (anm_model_set_env) in the tables of a lane-group family: its scalars and the observation bounds are the
// task's, not the network's, and go into every class
void set_lane_group_task(Tables& t, const anm_env_config& cfg, int state_dim) {
  if (!t.ok) return;
  auto apply = [&](std::vector<double>& hd) {
    hd[radial::SF_C1] = cfg.clip_e_loss;
    hd[radial::SF_C2] = cfg.clip_penalty;
    hd[radial::SF_RTERM] = -cfg.clip_penalty / (1 - cfg.gamma);
    hd[radial::SF_PERIOD] = cfg.period;
    for (int k = 0; k < state_dim; ++k) {
      if (cfg.obs_low) hd[t.off_obs_lo + k] = cfg.obs_low[k];
      if (cfg.obs_high) hd[t.off_obs_hi + k] = cfg.obs_high[k];
    }
  };
  apply(t.h0);
  for (auto& x : t.extra) apply(x);
}

// The task of anm_model_set_env between its checks and its commit: what the checks resolve from cfg on the host, then
// (stage_task) the device tables and the episode settings -- all of it apart from the model
struct Task {
  int period = 0;
  const double* amp = nullptr;      // series-noise mode: the caller's amplitude table [nexo][period]
  std::vector<double> ends;         // drawn modes: [2][nexo] low, high
  std::vector<double> ar1;          // correlated noise: [2][nexo] rho, then sqrt(1 - rho^2)
  double* exo_z = nullptr;          // ... the caller's noise states
  void* exo_forecast = nullptr;     // expected forecast: the caller's rows
  int forecast_h = 0;               // ... and the horizon (0: off)
  DevBuf<double> series, exo, noise, corr;
  DevBuf<ExoForecastIO> forecast;
  EpisodeIO ep{};
};

// the ends of a drawn exogenous mode: the model's defaults overlaid by exo_low / exo_high.  finite: every end must be
// finite (uniform mode); else merely not NaN (series-noise mode: an infinite end is no clip on that side)
bool resolve_ends(const anm_model* m, const anm_env_config& cfg, bool finite, std::vector<double>& ends) {
  const int nexo = m->dims.n_load + m->dims.n_gen;
  ends = m->exo_default;
  for (int k = 0; k < nexo; ++k) {
    if (cfg.exo_low) ends[k] = cfg.exo_low[k];
    if (cfg.exo_high) ends[nexo + k] = cfg.exo_high[k];
    if (finite && !(std::isfinite(ends[k]) && std::isfinite(ends[nexo + k]))) return false;
    if (!(ends[k] <= ends[nexo + k])) return false;   // (NaN fails the comparison)
  }
  return true;
}

int check_episode(const anm_model* m, const anm_env_config& cfg) {
  if (cfg.tail < ANM_ENV_TAIL_EPISODE) return 0;   // (a struct that ends at exo_high: nothing behind it is read)
  if (cfg.max_episode_steps < 0) return fail("anm_model_set_env: max_episode_steps must not be negative (0 = no limit)");
  if (cfg.max_episode_steps == 0 && !cfg.episode) return 0;
  if (m->has_view)
    return fail("anm_model_set_env: an episode time limit or episode buffers do not go with a bound batch view (anm_model_bind_view)");
  if (const anm_episode_buffers* b = cfg.episode) {
    if ((b->ep_disc_return == nullptr) != (b->ep_discount == nullptr))
      return fail("anm_model_set_env: ep_disc_return and ep_discount go together");
    if ((b->last_return && !b->ep_return) || (b->last_disc_return && !b->ep_disc_return))
      return fail("anm_model_set_env: last_return needs ep_return and last_disc_return needs ep_disc_return");
  }
  return 0;
}

// anm_model_set_env, part 1: every rule that can refuse the task.  Reads cfg and the model, writes t alone
int check_task(const anm_model* m, const anm_env_config& cfg, Task& t) {
  if (cfg.K < 0 || cfg.K > radial::KMAX) return fail("K (number of aux variables) must be in [0, 8]");
  static_assert(int(Layout<Topo>::KMAX) == int(radial::KMAX));   // (the one bound pack_env checks itself)
  const bool has_series = cfg.series && cfg.period > 0;
  if (has_series && cfg.K != 1) return fail("series mode needs exactly K = 1 auxiliary variable (the time index)");
  t.period = has_series ? cfg.period : 0;
  // (0 ... 3 and ANM_ENV_TAIL_FORECAST = 5; 4 stays unknown, as it was before the forecast)
  if (cfg.tail < ANM_ENV_TAIL_NONE || (cfg.tail > ANM_ENV_TAIL_CORR && cfg.tail != ANM_ENV_TAIL_FORECAST))
    return fail("anm_model_set_env: unknown value of tail");
  if (cfg.tail == ANM_ENV_TAIL_CORR && cfg.exo_mode != ANM_EXO_SERIES_NOISE)
    return fail("anm_model_set_env: correlated noise (tail = ANM_ENV_TAIL_CORR, an anm_env_config_corr) needs exo_mode = ANM_EXO_SERIES_NOISE");
  if (cfg.tail == ANM_ENV_TAIL_FORECAST && cfg.exo_mode != ANM_EXO_SERIES_NOISE)
    return fail("anm_model_set_env: the expected forecast (tail = ANM_ENV_TAIL_FORECAST, an anm_env_config_forecast) needs exo_mode = ANM_EXO_SERIES_NOISE");
  const int nexo = m->dims.n_load + m->dims.n_gen;
  const bool classes = m->n_classes() > 1 || m->d_env_class, no_defaults = int(m->exo_default.size()) != 2 * nexo;
  if (cfg.exo_mode == ANM_EXO_SERIES_NOISE) {
    // noisy time series: the series of series mode, an amplitude table beside it and clip ends (gym_anm_amd/rng.py)
    if (cfg.K != 1) return fail("anm_model_set_env: the series-noise mode needs exactly K = 1 auxiliary variable (the time index)");
    if (t.period <= 0) return fail("anm_model_set_env: the series-noise mode needs a series (series, period)");
    t.amp = cfg.tail >= ANM_ENV_TAIL_NOISE ? reinterpret_cast<const anm_env_config_noise&>(cfg).exo_noise : nullptr;
    if (!t.amp)
      return fail("anm_model_set_env: the series-noise mode needs the amplitude table (an anm_env_config_noise: tail = ANM_ENV_TAIL_NOISE and exo_noise)");
    if (classes) return fail("anm_model_set_env: the series-noise mode does not take parameter classes");
    if (m->has_view) return fail("anm_model_set_env: the series-noise mode does not go with a bound batch view (anm_model_bind_view)");
    if (no_defaults) return fail("anm_model_set_env: no default ends for the series-noise mode");
    for (size_t k = 0, cells = size_t(nexo) * size_t(t.period); k < cells; ++k)
      if (!std::isfinite(t.amp[k]) || t.amp[k] < 0.0)
        return fail("anm_model_set_env: the amplitudes of the series-noise mode must be finite and >= 0");
    if (!resolve_ends(m, cfg, false, t.ends))
      return fail("anm_model_set_env: the clip ends of the series-noise mode must not be NaN, with exo_low <= exo_high");
    bool corr = cfg.tail == ANM_ENV_TAIL_CORR;
    if (cfg.tail == ANM_ENV_TAIL_FORECAST) {
      // expected forecast: the horizon and the caller's rows; the correlation trio before them is all set or all NULL
      const anm_env_config_forecast& fc = reinterpret_cast<const anm_env_config_forecast&>(cfg);
      if (fc.forecast_horizon < 1 || fc.forecast_horizon > 64)
        return fail("anm_model_set_env: forecast_horizon (anm_env_config_forecast) must be in [1, 64]");
      if (!fc.exo_forecast) return fail("anm_model_set_env: the expected forecast needs exo_forecast (a device array [num_envs][n_load + n_gen][forecast_horizon])");
      corr = fc.cfg.exo_rho || fc.cfg.exo_innov || fc.cfg.exo_z;
      t.forecast_h = fc.forecast_horizon;
      t.exo_forecast = fc.exo_forecast;
    }
    if (corr) {
      // correlated noise: the AR(1) tables, both from the host (the kernels take no square root), and the caller's states
      const anm_env_config_corr& cc = reinterpret_cast<const anm_env_config_corr&>(cfg);
      if (!cc.exo_rho || !cc.exo_innov || !cc.exo_z)
        return fail(cfg.tail == ANM_ENV_TAIL_FORECAST
                        ? "anm_model_set_env: exo_rho, exo_innov and exo_z of an anm_env_config_forecast go together: all set (correlated noise) or all NULL"
                        : "anm_model_set_env: correlated noise needs exo_rho, exo_innov and exo_z (anm_env_config_corr): none may be NULL");
      t.ar1.resize(size_t(2 * nexo));
      for (int k = 0; k < nexo; ++k) {
        const double r = cc.exo_rho[k], c = cc.exo_innov[k];
        if (!std::isfinite(r) || !(r >= 0.0 && r < 1.0)) return fail("anm_model_set_env: exo_rho must be finite and in [0, 1)");
        if (!std::isfinite(c) || !(c > 0.0 && c <= 1.0)) return fail("anm_model_set_env: exo_innov must be finite and in (0, 1]");
        t.ar1[k] = r;
        t.ar1[nexo + k] = c;
      }
      t.exo_z = cc.exo_z;
    }
  } else if (cfg.exo_mode != ANM_EXO_HOST) {
    if (cfg.exo_mode != ANM_EXO_UNIFORM) return fail("anm_model_set_env: unknown exo_mode");
    if (cfg.K != 1) return fail("anm_model_set_env: the uniform exogenous mode needs exactly K = 1 auxiliary variable (the step index)");
    if (t.period > 0) return fail("anm_model_set_env: the uniform exogenous mode and a series do not go together");
    if (classes) return fail("anm_model_set_env: the uniform exogenous mode does not take parameter classes");
    if (no_defaults) return fail("anm_model_set_env: no default ends for the uniform exogenous mode");
    if (!resolve_ends(m, cfg, true, t.ends))
      return fail("anm_model_set_env: the ends of the uniform exogenous mode must be finite with exo_low <= exo_high");
  }
  return check_episode(m, cfg);
}

// anm_model_set_env, part 2: the device tables of a task that passed, and its episode settings, all into t
int stage_task(const anm_model* m, const anm_env_config& cfg, Task& t) {
  const size_t cells = size_t(m->dims.n_load + m->dims.n_gen) * size_t(t.period);
  int rc = 0;
  if (t.period > 0 && (rc = stage(t.series, cfg.series, cells, 0, "hipMalloc(series)", "hipMemcpy(series)"))) return rc;
  if (!t.ends.empty() && (rc = stage(t.exo, t.ends.data(), t.ends.size(), 8, "hipMalloc(exo ends)", "hipMemcpy(exo ends)"))) return rc;
  if (t.amp && (rc = stage(t.noise, t.amp, cells, 0, "hipMalloc(exo noise)", "hipMemcpy(exo noise)"))) return rc;
  if (!t.ar1.empty() && (rc = stage(t.corr, t.ar1.data(), t.ar1.size(), 8, "hipMalloc(exo corr)", "hipMemcpy(exo corr)"))) return rc;
  if (t.forecast_h > 0) {   // the block of the expected forecast: the tables just staged (a move keeps their addresses)
    const int nexo = m->dims.n_load + m->dims.n_gen;
    const ExoForecastIO f{t.corr.get(), t.corr.get() ? t.exo_z : nullptr, t.noise.get(), t.series.get(), t.exo.get(), t.exo.get() + nexo,
                          t.exo_forecast, t.period, t.forecast_h};
    if ((rc = stage(t.forecast, &f, 1, 0, "hipMalloc(exo forecast)", "hipMemcpy(exo forecast)"))) return rc;
  }
  if (cfg.tail >= ANM_ENV_TAIL_EPISODE && (cfg.max_episode_steps > 0 || cfg.episode)) {
    EpisodeIO& ep = t.ep;
    if (const anm_episode_buffers* b = cfg.episode)
      ep = EpisodeIO{0, 0, 0.0, b->truncated, b->ep_return, b->ep_disc_return, b->ep_discount, b->last_return, b->last_disc_return,
                     b->last_length, b->episodes_done};
    ep.max_steps = cfg.max_episode_steps;
    ep.gamma = cfg.gamma;
    ep.on = (ep.max_steps > 0 || ep.truncated || ep.ret || ep.disc_ret || ep.last_len || ep.n_done) ? 1 : 0;
  }
  return 0;
}

// the tables of parameter class k for a lane-group family: its plan is the model's own but for the numbers
template <class Plan, class Build>
bool class_tables(const Plan& own, Build build, const anm_network_desc& desc, int k, std::vector<std::vector<double>>& out) {
  Plan P;
  std::string err;
  if (!build(desc, P, err) || P.hi != own.hi || P.hd.size() != own.hd.size()) {
    g_err = "class " + std::to_string(k) + ": not the topology of the model" + (err.empty() ? "" : " (" + err + ")");
    return false;
  }
  out.push_back(std::move(P.hd));
  return true;
}

// One launch: the kernel, its shape, its arguments; `what` is "launch <kernel>", the text of a failure.
template <class Kernel, class... Args>
int launch(const char* what, Kernel kernel, unsigned grid, unsigned threads, size_t lds, hipStream_t s, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, args...);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail_hip(e, what);
}

// anm_solver_opts.precision -> the arithmetic type of the Newton solve, as a tag: f(float{}) | f(double{})
template <class F>
int by_precision(int precision, F&& f) {
  return precision == ANM_SOLVE_F32 ? f(float{}) : f(double{});
}

ClassSel class_sel(const anm_model* m, const Tables& t) {
  if (!m->d_env_class) return ClassSel{m->d_zero.get(), 0, 0, 0};
  return ClassSel{m->d_env_class, int(t.h0.size()), 1, m->class_per_env ? 1 : 0};
}

// the variants of k_mesh a launch may pick (mesh::Launch), as function pointers: for hipFuncSetAttribute
template <bool WG, int SW, bool TL>
void mesh_variants(std::vector<const void*>& out) {
  out.push_back((const void*)mesh::k_mesh<float, false, WG, SW, TL>);
  out.push_back((const void*)mesh::k_mesh<double, false, WG, SW, TL>);
  out.push_back((const void*)mesh::k_mesh<float, true, WG, SW, TL>);
  out.push_back((const void*)mesh::k_mesh<double, true, WG, SW, TL>);
  out.push_back((const void*)mesh::k_mesh<IoMapped<float>, false, WG, SW, TL>);   // (the affine I/O map: no parameter classes)
  out.push_back((const void*)mesh::k_mesh<IoMapped<double>, false, WG, SW, TL>);
}

// the variant of k_mesh for a plan (mesh::Launch: WG, SW, TL) and for how the classes are bound
template <class JT, bool WG, int SW = 2, bool TL = !WG>
auto mesh_kernel(bool class_per_group, bool mapped) {
  if (mapped) return mesh::k_mesh<IoMapped<JT>, false, WG, SW, TL>;   // (anm_model_set_io_map refuses parameter classes)
  return class_per_group ? mesh::k_mesh<JT, true, WG, SW, TL> : mesh::k_mesh<JT, false, WG, SW, TL>;
}

int launch_mesh(anm_model* m, int precision, int64_t n, hipStream_t s, const radial::IO& io, SolverOpts so) {
  const mesh::Dims& d = m->mplan.d;
  const mesh::Launch& L = m->mlaunch;   // (decided once, at anm_model_create)
  const int per_block = mesh::envs_per_block(d, L);
  const unsigned grid = unsigned((n + per_block - 1) / per_block), threads = unsigned(64 * L.waves);
  const ClassSel cs = class_sel(m, m->t_mesh);
  const bool pg = cs.per_group != 0, mp = io.mode != 0 && io.e.iomap != nullptr;
  return by_precision(precision, [&](auto jt) {
    using JT = decltype(jt);
    auto kern = mesh::is_workgroup(d) ? mesh_kernel<JT, true>(pg, mp)
                : !L.tables_in_lds    ? mesh_kernel<JT, false, 2, false>(pg, mp)
                : L.simd_waves == 3   ? mesh_kernel<JT, false, 3>(pg, mp)
                                      : mesh_kernel<JT, false>(pg, mp);
    return launch("launch k_mesh", kern, grid, threads, L.lds, s, d, m->t_mesh.dev_int.get(), m->t_mesh.dev.get(), io, so, n, cs);
  });
}

// the lane-group families gather a list-form observation from one LDS row of the electrical state per environment
// (FS + KMAX doubles): the radial kernel in dynamic LDS next to its static 6 KB, the general kernel where its Jacobian
// blocks were
size_t radial_obs_lds_bytes(const anm_model* m) {
  return size_t(64 / m->plan.d.G) * size_t(m->plan.d.FS + radial::KMAX) * sizeof(double);
}

int launch_radial(anm_model* m, int precision, int64_t n, hipStream_t s, const radial::IO& io, SolverOpts so) {
  const int per_wave = 64 / m->plan.d.G;
  const unsigned grid = unsigned((n + per_wave - 1) / per_wave);
  // the model is the compiled tree: the specialised Newton loop; else (generic mode) the table-driven one
  bool spec = false;
  if constexpr (Topo::TREE != 0) spec = m->t_thread.ok && m->plan.d.G == Topo::GRP && !getenv("ANM_RADIAL_GENERIC");
  const ClassSel cs = class_sel(m, m->t_radial);
  const size_t obs_lds = (io.mode == 2 && io.e.n_obs > 0) ? radial_obs_lds_bytes(m) : 0;   // rows of a list-form observation
  auto go = [&](auto kern) {
    return launch("launch k_radial", kern, grid, 64, obs_lds, s, m->plan.d, m->t_radial.dev_int.get(), m->t_radial.dev.get(), io, so, n, cs);
  };
  return by_precision(precision, [&](auto jt) {
    using JT = decltype(jt);
    const bool mp = io.mode != 0 && io.e.iomap != nullptr;   // the affine I/O map (it refuses parameter classes)
    if constexpr (Topo::TREE != 0)
      if (spec) return mp ? go(radial::k_radial<IoMapped<JT>, Topo>) : cs.per_group ? go(radial::k_radial<JT, Topo, true>) : go(radial::k_radial<JT, Topo>);
    if (mp) return go(radial::k_radial<IoMapped<JT>, void>);
    return cs.per_group ? go(radial::k_radial<JT, void, true>) : go(radial::k_radial<JT, void>);
  });
}

// The lane-group families serve every entry point with one kernel, told apart by radial::IO::mode: 0 transition (t),
// 1 reset, 2 step (e)
bool on_lane_groups(const anm_model* m) { return m->impl == ANM_IMPL_RADIAL || m->impl == ANM_IMPL_MESH; }
int launch_lane_groups(anm_model* m, int mode, const TransitionIO* t, const EnvIO* e, int precision, int64_t n, hipStream_t s,
                       SolverOpts so) {
  radial::IO io{};
  io.mode = mode;
  if (t) io.t = *t;
  if (e) io.e = *e;
  io.v = m->view;
  return m->impl == ANM_IMPL_MESH ? launch_mesh(m, precision, n, s, io, so) : launch_radial(m, precision, n, s, io, so);
}

SolverOpts solver(const anm_solver_opts* o, int& precision) {
  SolverOpts s{1e-5, 100, ANM_HANDOFF_AUTO, 0};
  precision = ANM_SOLVE_F64;
  if (o) {
    s.tol = o->tol;
    s.max_iter = o->max_iter;
    precision = o->precision;
    s.handoff = o->handoff_after;
    s.rowc = o->row_continuation;
  }
  // default hand-over point: every converging solve seen so far needs <= 9 iterations at tol 1e-6, so after
  // ANM_HANDOFF_DEFAULT trips the lanes still iterating are (almost only) diverging solves
  if (s.handoff == ANM_HANDOFF_AUTO) s.handoff = Topo::TREE ? ANM_HANDOFF_DEFAULT : ANM_HANDOFF_NEVER;
  return s;
}

// the dense Y_bus of a generic model (the compiled topology has it from pack_constants)
void dense_ybus(const anm_network_desc& desc, std::vector<cplx>& ybus) {
  const int NB = desc.n_bus;
  ybus.assign(size_t(NB) * NB, cplx(0, 0));
  for (int b = 0; b < desc.n_branch; ++b) {
    const int f = desc.br_from[b], t = desc.br_to[b];
    const cplx ys(desc.br_series[2 * b], desc.br_series[2 * b + 1]), sh(desc.br_shunt[2 * b], desc.br_shunt[2 * b + 1]);
    const cplx tap(desc.br_tap[2 * b], desc.br_tap[2 * b + 1]);
    ybus[f * NB + t] = -ys / std::conj(tap);
    ybus[t * NB + f] = -ys / tap;
    ybus[f * NB + f] += (ys + sh) / (std::abs(tap) * std::abs(tap));
    ybus[t * NB + t] += ys + sh;
  }
}

// the table of the stand-alone sampler (class 0) and the default ends of the drawn exogenous modes
int set_sampler_tables(anm_model* m, const anm_network_desc& desc) {
  std::vector<double> tab(size_t(6) * desc.n_dev, 0.0);
  m->s_nd = desc.n_dev;
  for (int k = 0; k < desc.n_dev; ++k) {
    const int t = desc.dev_type[k];
    int slot = -1;
    if (t == DEV_LOAD) slot = m->s_nload++;
    else if (t == DEV_CLASSICAL || t == DEV_RENEWABLE) slot = m->s_ngen++;
    else if (t == DEV_STORAGE) slot = m->s_ndes++;
    double* o = &tab[6 * size_t(k)];
    o[0] = t; o[1] = slot; o[2] = desc.dev_qmin[k]; o[3] = desc.dev_qmax[k];
    o[4] = t == DEV_STORAGE ? desc.dev_soc_min[k] : 0.0; o[5] = t == DEV_STORAGE ? desc.dev_soc_max[k] : 0.0;
  }
  // default ends of the uniform exogenous mode, in MW, by unit (loads by device id, then non-slack generators)
  const int nexo = m->s_nload + m->s_ngen;
  m->exo_default.assign(2 * size_t(nexo), 0.0);
  for (int k = 0; k < desc.n_dev; ++k) {
    const int t = desc.dev_type[k], slot = int(tab[6 * size_t(k) + 1]);
    if (t == DEV_LOAD) m->exo_default[slot] = desc.dev_pmin[k] * desc.base_mva;
    else if (t == DEV_CLASSICAL || t == DEV_RENEWABLE) m->exo_default[nexo + m->s_nload + slot] = desc.dev_pmax[k] * desc.base_mva;
  }
  return m->d_samp.assign(tab.data(), tab.size(), 8) == hipSuccess ? 0 : fail("hipMalloc(sampler table)");
}

inline unsigned grid_for(int64_t n) { return unsigned((n + BLOCK - 1) / BLOCK); }

}  // namespace

extern "C" {

const char* anm_last_error(void) { return g_err.c_str(); }
const char* anm_topology_name(void) { return Topo::NAME; }
const char* anm_topology_signature(void) { return Topo::SIGNATURE; }

int anm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int anm_model_create(const anm_network_desc* desc, anm_model** out) {
  if (!desc || !out) return fail("anm_model_create: null argument");
  anm_model* m = new (std::nothrow) anm_model();
  if (!m) return fail("out of host memory");
  auto give_up = [&](int rc) {   // (every way out but the last: what was allocated so far goes with the model)
    delete m;
    return rc;
  };
  std::string err, err_topo;
  m->t_thread.ok = pack_constants<Topo>(*desc, m->h_const, m->ybus, err_topo);
  if (m->t_thread.ok) {
    m->t_thread.off_obs_lo = Layout<Topo>::OBS_LO;
    m->t_thread.off_obs_hi = Layout<Topo>::OBS_HI;
    // k_step_general's dynamic LDS: the electrical-state rows (at most 60 KB, GenLds::FULL_OK) plus the state rows can
    // exceed the default 64 KB per workgroup (an 8-bus tree with 9 devices: 68 KB).  The attribute is set here, once,
    // not in a launch path that may be under stream capture
    typedef GenLds<Topo> GL;
    constexpr size_t worst = (size_t(GL::FULL_OK ? (64 * GL::FSP > GL::B_DOUBLES ? 64 * GL::FSP : GL::B_DOUBLES) : GL::B_DOUBLES) +
                              size_t(64) * size_t(GL::SP)) * sizeof(double);
    if (worst > 64 * 1024) {
      for (const void* k : {(const void*)k_step_general<float>, (const void*)k_step_general<double>, (const void*)k_step_general_fc<float>,
                            (const void*)k_step_general_fc<double>}) {
        hipError_t a = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (a != hipSuccess) return give_up(fail_hip(a, "k_step_general: LDS size attribute"));
      }
    }
    hipError_t e = m->t_thread.dev.alloc(m->h_const.size());
    if (e != hipSuccess) return give_up(fail_hip(e, "hipMalloc(constants)"));
  }
  if (radial::is_radial(*desc) && radial::build_plan(*desc, m->plan, err) && alloc_plan(m->t_radial, m->plan.hi)) {
    m->t_radial.ok = true;
    m->t_radial.off_obs_lo = m->plan.d.off_obs_lo;
    m->t_radial.off_obs_hi = m->plan.d.off_obs_hi;
    // default: the lane-group kernel once the thread-per-environment working set no longer fits
    // in registers (measured: a 30-bus feeder spills 4.7 KB/lane); ANM_IMPL=thread|radial overrides
    m->impl = (!m->t_thread.ok || desc->n_bus > 12) ? ANM_IMPL_RADIAL : ANM_IMPL_THREAD;
    const char* ev = getenv("ANM_IMPL");
    if (ev && std::string(ev) == "thread" && m->t_thread.ok) m->impl = ANM_IMPL_THREAD;
    if (ev && std::string(ev) == "radial") m->impl = ANM_IMPL_RADIAL;
  }
  std::string err_mesh;
  if (mesh::build_plan(*desc, m->mplan, err_mesh) && alloc_plan(m->t_mesh, m->mplan.hi)) {
    // the general lane-group kernel: any topology that fits a wavefront
    m->t_mesh.ok = true;
    m->t_mesh.off_obs_lo = m->mplan.d.off_obs_lo;
    m->t_mesh.off_obs_hi = m->mplan.d.off_obs_hi;
    m->mlaunch = mesh::launch_of(m->mplan.d);
    if (m->mlaunch.lds > 64 * 1024) {
      // above the default per-workgroup limit: ask for the compute unit's whole LDS (once, here: an
      // attribute call has no place in a launch path that may be under stream capture)
      std::vector<const void*> fns;
      mesh_variants<false, 2, true>(fns); mesh_variants<false, 3, true>(fns); mesh_variants<false, 2, false>(fns); mesh_variants<true, 2, false>(fns);
      for (const void* fn : fns)
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) m->t_mesh.ok = false;
    }
    if (m->t_mesh.ok) {
      // default for what neither of the other families serves well: not a tree, and either not the compiled
      // topology or too large for one thread's registers
      if (!m->t_radial.ok && (!m->t_thread.ok || desc->n_bus > 12)) m->impl = ANM_IMPL_MESH;
      const char* ev = getenv("ANM_IMPL");
      if (ev && std::string(ev) == "mesh") m->impl = ANM_IMPL_MESH;
    }
  }
  if (const char* ev = getenv("ANM_VIEW_WAVES")) {
    const int v = atoi(ev);
    if (v == 1 || v == 2) m->view_waves = v;
  }
  if (m->t_thread.ok) {
    set_shape(m, Topo::NB, Topo::ND, Topo::NBR, Topo::NLOAD, Topo::NGEN, Topo::NDES, Topo::SDIM, Layout<Topo>::TOTAL);
  } else if (m->t_radial.ok || m->t_mesh.ok) {
    auto of_plan = [&](const auto& d) { set_shape(m, d.NB, d.ND, d.NBR, d.NLOAD, d.NGEN, d.NDES, d.SDIM, d.n_double); };
    if (m->t_radial.ok) of_plan(m->plan.d);
    else of_plan(m->mplan.d);
  } else {
    // neither the compiled topology nor a network the generic lane-group kernels can take
    g_err = err_topo;
    return give_up(-3);
  }
  if (!m->t_thread.ok) dense_ybus(*desc, m->ybus);   // generic model: for diagnostics
  int rc = upload_const(m);
  const int32_t zero = 0;
  if (rc == 0 && m->d_zero.assign(&zero, 1) != hipSuccess) rc = fail("hipMalloc(class selector)");
  if (rc == 0) rc = set_sampler_tables(m, *desc);
  if (rc) return give_up(rc);
  *out = m;
  return 0;
}

void anm_model_destroy(anm_model* m) { delete m; }

int anm_model_dims(const anm_model* m, anm_dims* out) {
  if (!m || !out) return fail("anm_model_dims: null argument");
  *out = m->dims;
  return 0;
}

int anm_model_full_layout(const anm_model* m, anm_full_layout* o) {
  if (!m || !o) return fail("anm_model_full_layout: null argument");
  const int* b = m->full.base;
  o->bus_p = b[FC_BUS_P]; o->bus_q = b[FC_BUS_Q]; o->bus_v_magn = b[FC_BUS_VM]; o->bus_v_ang = b[FC_BUS_VA];
  o->bus_i_magn = b[FC_BUS_IM]; o->bus_i_ang = b[FC_BUS_IA]; o->dev_p = b[FC_DEV_P]; o->dev_q = b[FC_DEV_Q];
  o->des_soc = b[FC_DES_SOC]; o->gen_p_max = b[FC_GEN_PMAX]; o->branch_p = b[FC_BR_P]; o->branch_q = b[FC_BR_Q];
  o->branch_s = b[FC_BR_S]; o->branch_i_magn = b[FC_BR_IM]; o->branch_i_ang = b[FC_BR_IA]; o->size = b[FC_COUNT];
  return 0;
}

int anm_model_set_env(anm_model* m, const anm_env_config* cfg) {
  if (!m || !cfg) return fail("anm_model_set_env: null argument");
  if (m->d_iomap.get())
    return fail("anm_model_set_env: an affine I/O map is set (anm_model_set_io_map), whose tables have the lengths of the task that was "
                "set: clear it first (NULL) and set it again afterwards");
  // 1. whatever can refuse the task, 2. its device tables, in buffers of their own: the model is untouched so far
  Task t;
  if (int rc = check_task(m, *cfg, t)) return rc;
  if (int rc = stage_task(m, *cfg, t)) return rc;
  // 3. commit
  if (m->t_thread.ok) {
    std::string err;   // (pack_env refuses nothing but the K that check_task has passed)
    pack_env<Topo>(*cfg, m->h_const, err);
    for (auto& xc : m->t_thread.extra) pack_env<Topo>(*cfg, xc, err);
  }
  // (a known difference: where obs_low / obs_high are NULL the lane-group tables keep their old observation bounds,
  // the thread tables fall back to -inf / +inf)
  set_lane_group_task(m->t_radial, *cfg, m->dims.state_base_dim + cfg->K);
  set_lane_group_task(m->t_mesh, *cfg, m->dims.state_base_dim + cfg->K);
  m->d_series = std::move(t.series);
  m->d_exo = std::move(t.exo);
  m->d_noise = std::move(t.noise);
  m->d_corr = std::move(t.corr);
  m->K = cfg->K;
  m->period = t.period;
  m->exo_mode = cfg->exo_mode;
  m->exo_z = t.exo_z;
  m->d_forecast = std::move(t.forecast);
  m->ep = t.ep;
  m->env_set = true;
  return upload_const(m);
}

int anm_model_set_classes(anm_model* m, int32_t n_classes, const anm_network_desc* const* descs) {
  if (!m) return fail("anm_model_set_classes: null model");
  if (n_classes > 1 && m->has_view)
    return fail("anm_model_set_classes: not while a batch view is bound (anm_model_bind_view)");
  if (n_classes < 1 || n_classes > 65536) return fail("anm_model_set_classes: n_classes must be in [1, 65536]");
  if (n_classes > 1 && m->exo_mode != ANM_EXO_HOST) return fail("anm_model_set_classes: the uniform and series-noise exogenous modes do not take parameter classes");
  if (n_classes > 1 && m->io_mode == ANM_IO_F32) return fail("anm_model_set_classes: the float32 I/O mode (anm_model_set_io) does not take parameter classes");
  if (n_classes > 1 && m->d_iomap.get()) return fail("anm_model_set_classes: the affine I/O map (anm_model_set_io_map) does not take parameter classes");
  if (n_classes > 1 && !descs) return fail("anm_model_set_classes: null descriptions");
  std::vector<std::vector<double>> xc, xh, xm;
  for (int k = 1; k < n_classes; ++k) {
    if (!descs[k]) return fail("anm_model_set_classes: null description");
    if (m->t_thread.ok) {
      std::string err;
      std::vector<double> cbuf;
      std::vector<cplx> y;
      if (!pack_constants<Topo>(*descs[k], cbuf, y, err)) {
        g_err = "class " + std::to_string(k) + ": " + err;
        return -3;
      }
      xc.push_back(std::move(cbuf));
    }
    if (m->t_radial.ok && !class_tables(m->plan, radial::build_plan, *descs[k], k, xh)) return -3;
    if (m->t_mesh.ok && !class_tables(m->mplan, mesh::build_plan, *descs[k], k, xm)) return -3;
  }
  for (Tables* t : m->tables())
    if (int rc = reallocate(*t, n_classes)) return rc;
  m->t_thread.extra = std::move(xc);
  m->t_radial.extra = std::move(xh);
  m->t_mesh.extra = std::move(xm);
  m->d_env_class = nullptr;
  m->class_per_env = false;
  if (m->impl_unbound >= 0) { m->impl = m->impl_unbound; m->impl_unbound = -1; }
  m->env_set = false;   // the task constants (anm_model_set_env) must be set again: they live in every class
  return upload_const(m);
}

int anm_model_set_class_obs_bounds(anm_model* m, int32_t cls, const double* low, const double* high) {
  if (!m || !low || !high) return fail("anm_model_set_class_obs_bounds: null argument");
  if (!m->env_set) return fail("anm_model_set_class_obs_bounds: call anm_model_set_env first (it writes every class)");
  if (cls < 0 || cls >= m->n_classes()) return fail("anm_model_set_class_obs_bounds: no such class");
  for (Tables* t : m->tables()) set_obs_bounds(*t, cls, m->dims.state_base_dim + m->K, low, high);
  return upload_const(m);
}

int anm_model_bind_env_classes(anm_model* m, const int32_t* env_class, int64_t num_envs) {
  if (!m) return fail("anm_model_bind_env_classes: null model");
  auto restore_impl = [&]() {   // a binding that forced a lane-group family is gone: back to the family it displaced
    if (m->impl_unbound >= 0) m->impl = m->impl_unbound;
    m->impl_unbound = -1;
  };
  // Lifting a binding (or rebinding in aligned blocks) takes the model back to the family the binding displaced.  A
  // list-form observation set meanwhile has the tables of the lane-group family it was set in (identity layout, no row
  // stride): the thread-per-environment kernels would gather from overlapping LDS rows.  Refused, like the forward
  // direction below and anm_model_set_impl.
  auto restore_refused = [&]() {
    return m->n_obs > 0 && m->impl_unbound >= 0 && m->impl_unbound != m->impl;
  };
  const char* const restore_msg =
      "anm_model_bind_env_classes: lifting this binding moves the model back to the kernel family it displaced, and the "
      "list-form observation that is set (anm_model_set_obs) has the tables of the current family: clear it first "
      "(n_obs = 0) and set it again afterwards";
  if (!env_class) {
    if (restore_refused()) return fail(restore_msg);
    m->d_env_class = nullptr;
    m->class_per_env = false;
    restore_impl();
    return 0;
  }
  if (m->has_view)   // (the same rule as anm_model_bind_view, from the other side: k_mesh looks a block's
    // class up by launch slot and an environment's by its index in the batch)
    return fail("anm_model_bind_env_classes: not while a batch view is bound (anm_model_bind_view)");
  if (m->exo_mode == ANM_EXO_SERIES_NOISE) return fail("anm_model_bind_env_classes: the series-noise mode does not take parameter classes");
  if (m->io_mode == ANM_IO_F32) return fail("anm_model_bind_env_classes: the float32 I/O mode (anm_model_set_io) does not take parameter classes");
  if (m->d_iomap.get()) return fail("anm_model_bind_env_classes: the affine I/O map (anm_model_set_io_map) does not take parameter classes");
  if (num_envs <= 0) return fail("anm_model_bind_env_classes: num_envs must be positive");
  const int n_classes = m->n_classes();
  std::vector<int32_t> h(static_cast<size_t>(num_envs));
  hipError_t e = hipMemcpy(h.data(), env_class, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail_hip(e, "anm_model_bind_env_classes");
  bool blocks = true;
  for (int64_t i = 0; i < num_envs; ++i) {
    if (h[i] < 0 || h[i] >= n_classes) return fail("anm_model_bind_env_classes: class index out of range");
    blocks = blocks && h[i] == h[i - i % 64];
  }
  // One class per aligned block of 64 environments: the constants of a wavefront stay wave-uniform (scalar loads) in
  // every kernel family.  Any other assignment -- a different network in every environment -- is served by the
  // lane-group families (one environment per lane group, its constants read by vector loads); the
  // thread-per-environment kernels cannot (64 environments share a wavefront's scalar constants).
  if (!blocks && !(m->t_radial.ok || m->t_mesh.ok))
    return fail("anm_model_bind_env_classes: a class must cover whole aligned blocks of 64 environments (this network has no lane-group kernel)");
  // (the same guard as anm_model_set_impl: the lane-group kernels do not gather a list-form observation -- moving a
  // model with one to them would silently turn its observation into clip(state))
  if (!blocks && m->impl == ANM_IMPL_THREAD && m->n_obs > 0)
    return fail("anm_model_bind_env_classes: classes that change inside blocks of 64 environments move the model to a lane-group "
                "kernel, and the list-form observation that is set (anm_model_set_obs) has the tables of the thread-per-environment "
                "kernel: clear it first (n_obs = 0) and set it again after binding, or bind the classes in aligned blocks of 64");
  if (blocks && restore_refused()) return fail(restore_msg);
  m->class_per_env = !blocks;
  m->d_env_class = env_class;
  if (blocks) restore_impl();
  else if (m->impl == ANM_IMPL_THREAD) {
    m->impl_unbound = ANM_IMPL_THREAD;
    m->impl = m->t_radial.ok ? ANM_IMPL_RADIAL : ANM_IMPL_MESH;
  }
  return 0;
}

int anm_model_bind_state_same(anm_model* m, uint8_t* state_same) {
  if (!m) return fail("anm_model_bind_state_same: null model");
  if (state_same && m->has_view) return fail("anm_model_bind_state_same: not while a batch view is bound");
  if (state_same && m->io_mode == ANM_IO_F32)
    return fail("anm_model_bind_state_same: not in the float32 I/O mode (anm_model_set_io): the state row has no float64 twin in obs and is always written");
  if (state_same && m->d_iomap.get())
    return fail("anm_model_bind_state_same: not while an affine I/O map is set (anm_model_set_io_map): obs is no copy of the state row, which is always written");
  m->d_state_same = state_same;
  return 0;
}

int anm_model_bind_nr_diff(anm_model* m, double* nr_diff) {
  if (!m) return fail("anm_model_bind_nr_diff: null model");
  m->d_nr_diff = nr_diff;
  return 0;
}

int anm_model_bind_nr_start(anm_model* m, const double* x0) {
  if (!m) return fail("anm_model_bind_nr_start: null model");
  m->d_nr_start = x0;
  return 0;
}

int anm_model_set_io(anm_model* m, int32_t io) {
  if (!m) return fail("anm_model_set_io: null model");
  if (io != ANM_IO_F64 && io != ANM_IO_F32) return fail("anm_model_set_io: unknown value (ANM_IO_F64 | ANM_IO_F32)");
  if (io == ANM_IO_F32) {
    if (m->has_view) return fail("anm_model_set_io: the float32 I/O mode does not go with a batch view (anm_model_bind_view)");
    if (m->n_classes() > 1 || m->d_env_class)
      return fail("anm_model_set_io: the float32 I/O mode does not take parameter classes (anm_model_set_classes / anm_model_bind_env_classes)");
    if (m->d_state_same)
      return fail("anm_model_set_io: the float32 I/O mode does not go with anm_model_bind_state_same (the state row has no float64 twin in obs)");
  }
  m->io_mode = io;
  return 0;
}

int anm_model_set_io_map(anm_model* m, const anm_io_map* map) {
  if (!m) return fail("anm_model_set_io_map: null model");
  if (!map) {   // back to the plain arrays
    m->d_iomap.reset();
    return 0;
  }
  if (!m->env_set) return fail("anm_model_set_io_map: call anm_model_set_env first (and anm_model_set_obs, where a list is gathered in the kernel)");
  if (m->has_view) return fail("anm_model_set_io_map: the affine I/O map does not go with a batch view (anm_model_bind_view)");
  if (m->n_classes() > 1 || m->d_env_class)
    return fail("anm_model_set_io_map: the affine I/O map does not take parameter classes (anm_model_set_classes / anm_model_bind_env_classes)");
  if (m->d_state_same)
    return fail("anm_model_set_io_map: the affine I/O map does not go with anm_model_bind_state_same (obs is no copy of the state row)");
  const int n_act = (map->act_mid ? 1 : 0) + (map->act_half ? 1 : 0) + (map->act_low ? 1 : 0) + (map->act_high ? 1 : 0);
  if (n_act != 0 && n_act != 4) return fail("anm_model_set_io_map: act_mid, act_half, act_low and act_high are all NULL (actions not mapped) or all set");
  if ((map->obs_scale == nullptr) != (map->obs_bias == nullptr))
    return fail("anm_model_set_io_map: obs_scale and obs_bias are both NULL (observations not mapped) or both set");
  if (!(std::isfinite(map->reward_scale) && map->reward_scale > 0.0)) return fail("anm_model_set_io_map: reward_scale must be finite and > 0");
  const int A = m->dims.action_dim, N = m->n_obs > 0 ? m->n_obs : m->dims.state_base_dim + m->K;
  const double inf = std::numeric_limits<double>::infinity();
  // a part that is not mapped gets the exact identity (IoMap, anm_env_ops.hpp): the kernels test one pointer, no table
  std::vector<double> h(size_t(IoMap::obs(A)) + 2 * size_t(N));
  h[IoMap::REWARD] = map->reward_scale;
  for (int j = 0; j < A; ++j) {
    double* a = &h[IoMap::ACT + j];
    a[0] = -0.0; a[A] = 1.0; a[2 * A] = -inf; a[3 * A] = inf;
    if (!n_act) continue;
    const double mid = map->act_mid[j], half = map->act_half[j], lo = map->act_low[j], hi = map->act_high[j];
    if (!(std::isfinite(half) && half > 0.0)) return fail("anm_model_set_io_map: act_half must be finite and > 0");
    if (!std::isfinite(mid)) return fail("anm_model_set_io_map: act_mid must be finite");
    if (!(lo <= hi)) return fail("anm_model_set_io_map: act_low > act_high (or NaN)");
    a[0] = mid; a[A] = half; a[2 * A] = lo; a[3 * A] = hi;
  }
  for (int k = 0; k < N; ++k) {
    double* o = &h[IoMap::obs(A) + k];
    o[0] = 1.0; o[N] = -0.0;
    if (!map->obs_scale) continue;
    if (!(std::isfinite(map->obs_scale[k]) && map->obs_scale[k] > 0.0)) return fail("anm_model_set_io_map: obs_scale must be finite and > 0");
    if (!std::isfinite(map->obs_bias[k])) return fail("anm_model_set_io_map: obs_bias must be finite");
    o[0] = map->obs_scale[k]; o[N] = map->obs_bias[k];
  }
  DevBuf<double> d;   // (a refused or failed call leaves the map that is set as it was)
  const hipError_t e = d.assign(h.data(), h.size());
  if (e != hipSuccess) return fail_hip(e, "anm_model_set_io_map");
  m->d_iomap = std::move(d);
  return 0;
}

namespace {

// what both entry points of the running normalisation check, and the arguments of its kernels
int io_norm_args(const char* who, anm_model* m, const anm_io_norm* nm, ionorm::Args& a) {
  const std::string w = who;
  if (!m) return fail((w + ": null model").c_str());
  if (!nm) return fail((w + ": null anm_io_norm").c_str());
  if (!m->d_iomap.get())
    return fail((w + ": no affine I/O map is set (anm_model_set_io_map): the running normalisation rewrites the tables of that map").c_str());
  if (m->has_view) return fail((w + ": the running normalisation does not go with a batch view (anm_model_bind_view)").c_str());
  if (m->n_classes() > 1 || m->d_env_class)
    return fail((w + ": the running normalisation does not take parameter classes (anm_model_set_classes / anm_model_bind_env_classes)").c_str());
  if (!nm->stats || !nm->counters) return fail((w + ": stats and counters must be set").c_str());
  if (!(std::isfinite(nm->eps) && nm->eps > 0.0)) return fail((w + ": eps must be finite and > 0").c_str());
  if (!(nm->gamma >= 0.0 && nm->gamma <= 1.0)) return fail((w + ": gamma must be in [0, 1]").c_str());
  a = ionorm::Args{};
  a.iomap = m->d_iomap.get();
  a.off_scale = IoMap::obs(m->dims.action_dim);
  a.D = m->n_obs > 0 ? m->n_obs : m->dims.state_base_dim + m->K;
  a.stats = nm->stats;
  a.counters = reinterpret_cast<long long*>(nm->counters);
  a.slabs = nm->slabs;
  a.G = nm->ret_acc;
  a.t_seen = nm->t_seen;
  a.gamma = nm->gamma;
  a.eps = nm->eps;
  a.obs_on = nm->obs_on ? 1 : 0;
  a.reward_on = nm->reward_on ? 1 : 0;
  return 0;
}

}  // namespace

int anm_model_io_norm_update(anm_model* m, int64_t num_envs, const double* obs, const double* reward, const uint8_t* terminated,
                             const uint8_t* truncated, const int32_t* timestep, const anm_io_norm* nm, void* stream) {
  const char* who = "anm_model_io_norm_update";
  ionorm::Args a;
  if (int rc = io_norm_args(who, m, nm, a)) return rc;
  if (num_envs < 1) return fail("anm_model_io_norm_update: num_envs < 1");
  if (!a.obs_on && !a.reward_on) return 0;
  if (!obs || !reward || !terminated || !timestep) return fail("anm_model_io_norm_update: obs, reward, terminated and timestep must be set");
  if (a.reward_on && (!a.G || !a.t_seen)) return fail("anm_model_io_norm_update: ret_acc and t_seen must be set while reward_on is");
  const int rows = ionorm::rows_per_group(num_envs);
  const int64_t groups = (num_envs + rows - 1) / rows;
  if (groups > ionorm::MAX_SLABS) return fail("anm_model_io_norm_update: more than 4 194 304 environments (4096 slabs of 1024 rows)");
  if (!nm->slabs || nm->n_slab_doubles < groups * ionorm::slab_doubles(a.D))
    return fail("anm_model_io_norm_update: the slab buffer is too short: ceil(num_envs / rows) slabs of 4 + 2 obs_dim doubles each, "
                "rows = 256 up to 262 144 environments and 1024 above");
  a.obs = obs;
  a.reward = reward;
  a.terminated = terminated;
  a.truncated = truncated;
  a.timestep = timestep;
  a.E = num_envs;
  a.n_slabs = int(groups);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool f32 = m->io_mode == ANM_IO_F32;
  auto partial = [&](auto kernel) { return launch("launch k_norm_partial", kernel, unsigned(groups), ionorm::LANES, 0, s, a); };
  if (int rc = rows == ionorm::WAVES * ionorm::SUB
                   ? (f32 ? partial(ionorm::k_norm_partial<true, 1>) : partial(ionorm::k_norm_partial<false, 1>))
                   : (f32 ? partial(ionorm::k_norm_partial<true, 4>) : partial(ionorm::k_norm_partial<false, 4>)))
    return rc;
  return launch("launch k_norm_finish", ionorm::k_norm_finish, 1, ionorm::FINISH_LANES, (size_t(ionorm::slab_doubles(a.D)) + 1) * sizeof(double), s, a);
}

int anm_model_io_norm_tables(anm_model* m, const anm_io_norm* nm, void* stream) {
  ionorm::Args a;
  if (int rc = io_norm_args("anm_model_io_norm_tables", m, nm, a)) return rc;
  return launch("launch k_norm_tables", ionorm::k_norm_tables, 1, ionorm::LANES, 0, static_cast<hipStream_t>(stream), a);
}

namespace {

// what every entry point of the rollout buffer checks
int rollout_args(const char* who, const anm_rollout* rb) {
  const std::string w = who;
  if (!rb) return fail((w + ": null anm_rollout").c_str());
  if (rb->T < 1 || rb->E < 1 || rb->D < 1) return fail((w + ": T, E and D must be at least 1").c_str());
  if (rb->T > (int64_t(1) << 30) || rb->E > (int64_t(1) << 30) || rb->E * int64_t(rb->D) > (int64_t(1) << 38))
    return fail((w + ": T or E above 2^30, or E D above 2^38").c_str());
  for (int32_t code : {rb->io_dtype, rb->value_dtype})
    if (code != ANM_IO_F64 && code != ANM_IO_F32) return fail((w + ": io_dtype and value_dtype must be ANM_IO_F64 or ANM_IO_F32").c_str());
  if (!(rb->gamma >= 0.0 && rb->gamma <= 1.0)) return fail((w + ": gamma must be in [0, 1]").c_str());
  if (!(rb->gae_lambda >= 0.0 && rb->gae_lambda <= 1.0)) return fail((w + ": gae_lambda must be in [0, 1]").c_str());
  if (!(std::isfinite(rb->eps) && rb->eps > 0.0)) return fail((w + ": eps must be finite and > 0").c_str());
  return 0;
}

int rollout_store(const char* what, const anm_rollout* rb, const rollout::StoreArgs& a, void* stream) {
  const unsigned grid = unsigned((a.n_obs + rollout::STORE_LANES - 1) / rollout::STORE_LANES);   // (E D >= E)
  hipStream_t s = static_cast<hipStream_t>(stream);
  return rb->io_dtype == ANM_IO_F32 ? launch(what, rollout::k_rollout_store<true>, grid, rollout::STORE_LANES, 0, s, a)
                                    : launch(what, rollout::k_rollout_store<false>, grid, rollout::STORE_LANES, 0, s, a);
}

}  // namespace

int anm_rollout_begin(const anm_rollout* rb, const void* obs, const int32_t* timestep, void* stream) {
  if (int rc = rollout_args("anm_rollout_begin", rb)) return rc;
  if (!rb->obs || !rb->t_seen || !obs || !timestep) return fail("anm_rollout_begin: the buffers obs and t_seen and the arrays obs and timestep must be set");
  rollout::StoreArgs a{};
  a.src_obs = obs;
  a.dst_obs = rb->obs;
  a.n_obs = rb->E * int64_t(rb->D);
  a.timestep = timestep;
  a.t_seen = rb->t_seen;
  a.E = rb->E;
  a.begin = 1;
  return rollout_store("launch k_rollout_store (begin)", rb, a, stream);
}

int anm_rollout_add(const anm_rollout* rb, int64_t k, const void* obs, const void* reward, const uint8_t* terminated,
                    const uint8_t* truncated, const int32_t* timestep, void* stream) {
  if (int rc = rollout_args("anm_rollout_add", rb)) return rc;
  if (k < 0 || k >= rb->T) return fail("anm_rollout_add: k is outside [0, T)");
  if (!rb->obs || !rb->rewards || !rb->flags || !rb->t_seen) return fail("anm_rollout_add: the buffers obs, rewards, flags and t_seen must be set");
  if (!obs || !reward || !terminated || !timestep) return fail("anm_rollout_add: obs, reward, terminated and timestep must be set");
  const size_t io = rb->io_dtype == ANM_IO_F32 ? 4 : 8;
  rollout::StoreArgs a{};
  a.src_obs = obs;
  a.n_obs = rb->E * int64_t(rb->D);
  a.dst_obs = static_cast<char*>(rb->obs) + size_t(k + 1) * size_t(a.n_obs) * io;
  a.reward = reward;
  a.dst_reward = static_cast<char*>(rb->rewards) + size_t(k) * size_t(rb->E) * io;
  a.terminated = terminated;
  a.truncated = truncated;
  a.timestep = timestep;
  a.flags = rb->flags + k * rb->E;
  a.t_seen = rb->t_seen;
  a.E = rb->E;
  a.begin = 0;
  return rollout_store("launch k_rollout_store", rb, a, stream);
}

int anm_rollout_gae(const anm_rollout* rb, void* stream) {
  if (int rc = rollout_args("anm_rollout_gae", rb)) return rc;
  if (!rb->rewards || !rb->values || !rb->flags || !rb->advantages || !rb->returns)
    return fail("anm_rollout_gae: the buffers rewards, values, flags, advantages and returns must be set");
  rollout::GaeArgs a{};
  a.rewards = rb->rewards;
  a.values = rb->values;
  a.flags = rb->flags;
  a.advantages = rb->advantages;
  a.returns = rb->returns;
  a.T = rb->T;
  a.E = rb->E;
  a.g = rb->gamma;
  const double gl = rb->gamma * rb->gae_lambda;   // (one double product, formed once: rule 3)
  a.gl = gl;
  const unsigned grid = unsigned((rb->E + rollout::GAE_LANES - 1) / rollout::GAE_LANES);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool r32 = rb->io_dtype == ANM_IO_F32, v32 = rb->value_dtype == ANM_IO_F32;
  auto go = [&](auto kernel) { return launch("launch k_rollout_gae", kernel, grid, rollout::GAE_LANES, 0, s, a); };
  return r32 ? (v32 ? go(rollout::k_rollout_gae<true, true>) : go(rollout::k_rollout_gae<true, false>))
             : (v32 ? go(rollout::k_rollout_gae<false, true>) : go(rollout::k_rollout_gae<false, false>));
}

int anm_rollout_adv_norm(const anm_rollout* rb, void* stream) {
  if (int rc = rollout_args("anm_rollout_adv_norm", rb)) return rc;
  if (!rb->advantages || !rb->flags || !rb->adv_norm || !rb->stats)
    return fail("anm_rollout_adv_norm: the buffers advantages, flags, adv_norm and stats must be set");
  if (rb->T > rollout::MAX_LEAVES / rb->E) return fail("anm_rollout_adv_norm: T E is above 67 108 864 (4096 slabs of 16 384 slots)");
  rollout::AdvArgs a{};
  a.advantages = rb->advantages;
  a.flags = rb->flags;
  a.adv_norm = rb->adv_norm;
  a.N = rb->T * rb->E;
  a.range = rollout::slab_range(a.N);
  const int64_t n_slabs = (a.N + a.range - 1) / a.range;
  if (!rb->slabs || rb->n_slab_doubles < n_slabs * rollout::SLAB)
    return fail("anm_rollout_adv_norm: the slab buffer is too short: 3 ceil(T E / range) doubles, range = 1024 doubled while that "
                "leaves more than 4096 slabs");
  a.slabs = rb->slabs;
  a.n_slabs = int(n_slabs);
  a.stats = rb->stats;
  a.eps = rb->eps;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool v32 = rb->value_dtype == ANM_IO_F32;
  if (int rc = v32 ? launch("launch k_adv_partial", rollout::k_adv_partial<true>, unsigned(n_slabs), rollout::ADV_LANES, 0, s, a)
                   : launch("launch k_adv_partial", rollout::k_adv_partial<false>, unsigned(n_slabs), rollout::ADV_LANES, 0, s, a))
    return rc;
  if (int rc = launch("launch k_adv_finish", rollout::k_adv_finish, 1, rollout::ADV_LANES, 0, s, a)) return rc;
  const unsigned grid = unsigned((a.N + rollout::ADV_LANES - 1) / rollout::ADV_LANES);
  return v32 ? launch("launch k_adv_apply", rollout::k_adv_apply<true>, grid, rollout::ADV_LANES, 0, s, a)
             : launch("launch k_adv_apply", rollout::k_adv_apply<false>, grid, rollout::ADV_LANES, 0, s, a);
}

namespace {

// what both entry points of the minibatch sampler check; n_ranges: the ranges of the plan
int minibatch_args(const char* who, const anm_minibatch* mb, int64_t& n_ranges) {
  const std::string w = who;
  if (!mb) return fail((w + ": null anm_minibatch").c_str());
  if (mb->T < 1 || mb->E < 1 || mb->D < 1 || mb->A < 1 || mb->B < 1) return fail((w + ": T, E, D, A and B must be at least 1").c_str());
  if (mb->T > rollout::MAX_LEAVES || mb->E > rollout::MAX_LEAVES || mb->T > rollout::MAX_LEAVES / mb->E)
    return fail((w + ": T E is above 67 108 864 (4096 ranges of 16 384 slots)").c_str());
  if (mb->D > (1 << 20) || mb->A > (1 << 20) || mb->B > (int64_t(1) << 30)) return fail((w + ": D or A above 2^20, or B above 2^30").c_str());
  for (int32_t code : {mb->io_dtype, mb->value_dtype})
    if (code != ANM_IO_F64 && code != ANM_IO_F32) return fail((w + ": io_dtype and value_dtype must be ANM_IO_F64 or ANM_IO_F32").c_str());
  if (!mb->index || !mb->state) return fail((w + ": index and state must be set").c_str());
  const int64_t N = mb->T * mb->E, range = rollout::slab_range(N);
  n_ranges = (N + range - 1) / range;
  if (!mb->counts || !mb->offsets || mb->n_counts < n_ranges)
    return fail((w + ": the counts buffer is too short: counts and offsets take ceil(T E / range) int32 each, range = 1024 doubled "
                     "while that leaves more than 4096 ranges").c_str());
  return 0;
}

}  // namespace

int anm_minibatch_prepare(const anm_minibatch* mb, void* stream) {
  int64_t n_ranges = 0;
  if (int rc = minibatch_args("anm_minibatch_prepare", mb, n_ranges)) return rc;
  if (!mb->flags) return fail("anm_minibatch_prepare: flags must be set");
  minibatch::PrepArgs a{};
  a.flags = mb->flags;
  a.index = mb->index;
  a.counts = mb->counts;
  a.offsets = mb->offsets;
  a.state = reinterpret_cast<long long*>(mb->state);
  a.N = mb->T * mb->E;
  a.range = rollout::slab_range(a.N);
  a.n_ranges = int(n_ranges);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = launch("launch k_mb_count", minibatch::k_mb_count, unsigned(n_ranges), minibatch::LANES, 0, s, a)) return rc;
  if (int rc = launch("launch k_mb_scan", minibatch::k_mb_scan, 1, minibatch::LANES, 0, s, a)) return rc;
  return launch("launch k_mb_scatter", minibatch::k_mb_scatter, unsigned(n_ranges), minibatch::LANES, 0, s, a);
}

int anm_minibatch_gather(const anm_minibatch* mb, int64_t m, int64_t ep, void* stream) {
  int64_t n_ranges = 0;
  if (int rc = minibatch_args("anm_minibatch_gather", mb, n_ranges)) return rc;
  if (!mb->obs || !mb->actions || !mb->logp || !mb->values || !mb->returns || !mb->adv)
    return fail("anm_minibatch_gather: the sources obs, actions, logp, values, returns and adv must be set");
  if (!mb->mb_obs || !mb->mb_actions || !mb->mb_logp || !mb->mb_values || !mb->mb_returns || !mb->mb_adv || !mb->mb_weight || !mb->mb_slot)
    return fail("anm_minibatch_gather: the eight destinations must be set");
  const int64_t N = mb->T * mb->E;
  if (m < 0 || m > (N - 1) / mb->B) return fail("anm_minibatch_gather: m is outside [0, ceil(T E / B))");   // (m B >= T E)
  if (ep < 0 || ep > int64_t(0xFFFFFFFFll)) return fail("anm_minibatch_gather: ep is outside [0, 2^32)");
  minibatch::GatherArgs a{};
  a.obs = mb->obs;
  a.actions = mb->actions;
  a.logp = mb->logp;
  a.values = mb->values;
  a.returns = mb->returns;
  a.adv = mb->adv;
  a.index = mb->index;
  a.state = reinterpret_cast<const long long*>(mb->state);
  a.mb_obs = mb->mb_obs;
  a.mb_actions = mb->mb_actions;
  a.mb_logp = mb->mb_logp;
  a.mb_values = mb->mb_values;
  a.mb_returns = mb->mb_returns;
  a.mb_adv = mb->mb_adv;
  a.mb_weight = mb->mb_weight;
  a.mb_slot = mb->mb_slot;
  a.N = N;
  a.first = m * mb->B;
  a.B = int32_t(mb->B);
  a.D = mb->D;
  a.A = mb->A;
  a.dq = minibatch::LANES / mb->D;
  a.dr = minibatch::LANES % mb->D;
  a.dm = (65536 + mb->D - 1) / mb->D;
  a.aq = minibatch::LANES / mb->A;
  a.ar = minibatch::LANES % mb->A;
  a.am = (65536 + mb->A - 1) / mb->A;
  a.ep = uint32_t(ep);
  a.seed = mb->seed;
  const unsigned grid = unsigned((mb->B + minibatch::TILE - 1) / minibatch::TILE);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool i32 = mb->io_dtype == ANM_IO_F32, v32 = mb->value_dtype == ANM_IO_F32;
  auto go = [&](auto kernel) { return launch("launch k_mb_gather", kernel, grid, minibatch::LANES, 0, s, a); };
  return i32 ? (v32 ? go(minibatch::k_mb_gather<true, true>) : go(minibatch::k_mb_gather<true, false>))
             : (v32 ? go(minibatch::k_mb_gather<false, true>) : go(minibatch::k_mb_gather<false, false>));
}

namespace {

// the layers of one net of the flat parameter vector from offset `at` on (policy.layout): W [K, N] then b [N] per layer
void policy_net(policy::Net& net, const anm_policy* pi, int n_out, int32_t& at) {
  net.n_layers = pi->n_hidden + 1;
  int K = pi->D;
  for (int i = 0; i < net.n_layers; ++i) {
    const int N = i < pi->n_hidden ? pi->hidden[i] : n_out;
    net.K[i] = K;
    net.N[i] = N;
    net.w[i] = at;
    at += K * N;
    net.b[i] = at;
    at += N;
    K = N;
  }
}

}  // namespace

int anm_policy_act(const anm_policy* pi, const void* obs, void* actions, void* values, void* logp, void* stream) {
  if (!pi) return fail("anm_policy_act: null anm_policy");
  if (pi->D < 1 || pi->D > policy::MAX_D) return fail("anm_policy_act: D is outside [1, 256]");
  if (pi->A < 1 || pi->A > policy::MAX_A) return fail("anm_policy_act: A is outside [1, 64]");
  if (pi->n_hidden < 1 || pi->n_hidden > policy::MAX_HIDDEN) return fail("anm_policy_act: n_hidden is outside [1, 3]");
  int H = 0;
  for (int i = 0; i < pi->n_hidden; ++i) {
    const int32_t h = pi->hidden[i];
    if (h < policy::MIN_WIDTH || h > policy::MAX_WIDTH || h % 32 != 0)
      return fail("anm_policy_act: a hidden width is not a multiple of 32 in [32, 256]");
    H = h > H ? h : H;
  }
  if (pi->activation != policy::ACT_TANH && pi->activation != policy::ACT_RELU) return fail("anm_policy_act: activation must be ANM_POLICY_TANH or ANM_POLICY_RELU");
  for (int32_t code : {pi->io_dtype, pi->value_dtype})
    if (code != ANM_IO_F64 && code != ANM_IO_F32) return fail("anm_policy_act: io_dtype and value_dtype must be ANM_IO_F64 or ANM_IO_F32");
  if (pi->E < 1 || pi->E > (int64_t(1) << 30)) return fail("anm_policy_act: E is outside [1, 2^30]");
  policy::Args a{};
  int32_t at = 0;
  policy_net(a.actor, pi, pi->A, at);
  policy_net(a.critic, pi, 1, at);
  a.log_std = at;
  at += pi->A;
  if (pi->n_params != at) return fail("anm_policy_act: n_params is not the size of the layout (actor, critic, log_std)");
  const bool critic_only = !actions && !logp;
  if (!pi->params || !obs || !values) return fail("anm_policy_act: params, obs and values must be set");
  if (!critic_only) {
    if (!actions || !logp) return fail("anm_policy_act: actions and logp must both be set (or both NULL: the critic alone)");
    if (!pi->noise || !pi->std) return fail("anm_policy_act: noise and std must be set");
    if (!pi->deterministic && (!pi->reset_count || !pi->timestep)) return fail("anm_policy_act: reset_count and timestep must be set");
  }
  const int wide = H > pi->A ? H : pi->A;
  a.S = (pi->D > wide ? pi->D : wide) | 1;
  a.SA = pi->A | 1;
  int waves = policy::MAX_WAVES;
  while (waves >= 1 && policy::lds_floats(at, a.S, a.SA, waves) * 4 > policy::LDS_BYTES) waves >>= 1;
  if (waves < 1) return fail("anm_policy_act: the network does not fit the LDS plan (P + 96 + 32 (2 (max(D, H, A)|1) + (A|1)) floats above 40 960)");
  a.params = pi->params;
  a.n_params = at;
  a.D = pi->D;
  a.A = pi->A;
  a.activation = pi->activation;
  a.deterministic = pi->deterministic ? 1 : 0;
  a.critic_only = critic_only ? 1 : 0;
  a.logp0 = float(-0.5 * double(pi->A) * std::log(2.0 * 3.141592653589793));   // (formed in double, rounded once: rule 6)
  a.seed = pi->seed;
  a.env_offset = pi->env_offset;
  a.reset_count = pi->reset_count;
  a.timestep = pi->timestep;
  a.obs = obs;
  a.actions = actions;
  a.values = values;
  a.logp = logp;
  a.noise = pi->noise;
  a.std = pi->std;
  a.E = pi->E;
  const int tile = waves * policy::ROWS;
  const size_t lds = size_t(policy::lds_floats(at, a.S, a.SA, waves)) * 4;
  a.vec4 = reinterpret_cast<uintptr_t>(pi->params) % 16 == 0 ? 1 : 0;
  // a workgroup stages the parameters once and then takes tiles in a loop: no more workgroups than the device holds at once
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, n = 0;
    n_cu = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : -1;
  }
  const int64_t n_tiles = (pi->E + tile - 1) / tile;
  const int64_t resident = n_cu > 0 ? int64_t(n_cu) * int64_t(policy::LDS_BYTES / lds) : n_tiles;
  const unsigned grid = unsigned(n_tiles < resident ? n_tiles : resident);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool i32 = pi->io_dtype == ANM_IO_F32, v32 = pi->value_dtype == ANM_IO_F32;
  static bool raised[4] = {false, false, false, false};   // (the default limit of dynamic LDS is 64 KiB; raised once per kernel)
  auto go = [&](auto kernel, int which) {
    if (!raised[which]) {
      hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, policy::LDS_BYTES);
      if (e != hipSuccess) return fail_hip(e, "anm_policy_act: hipFuncSetAttribute");
      raised[which] = true;
    }
    return launch("launch k_policy", kernel, grid, unsigned(waves * 64), lds, s, a);
  };
  return i32 ? (v32 ? go(policy::k_policy<true, true>, 0) : go(policy::k_policy<true, false>, 1))
             : (v32 ? go(policy::k_policy<false, true>, 2) : go(policy::k_policy<false, false>, 3));
}

int anm_policy_ppo_grad(const anm_policy* pi, const anm_ppo* job, void* stream) {
  if (!pi) return fail("anm_policy_ppo_grad: null anm_policy");
  if (!job) return fail("anm_policy_ppo_grad: null anm_ppo");
  if (pi->D < 1 || pi->D > policy::MAX_D) return fail("anm_policy_ppo_grad: D is outside [1, 256]");
  if (pi->A < 1 || pi->A > policy::MAX_A) return fail("anm_policy_ppo_grad: A is outside [1, 64]");
  if (pi->n_hidden < 1 || pi->n_hidden > policy::MAX_HIDDEN) return fail("anm_policy_ppo_grad: n_hidden is outside [1, 3]");
  int H = 0;
  for (int i = 0; i < pi->n_hidden; ++i) {
    const int32_t h = pi->hidden[i];
    if (h < policy::MIN_WIDTH || h > policy::MAX_WIDTH || h % 32 != 0)
      return fail("anm_policy_ppo_grad: a hidden width is not a multiple of 32 in [32, 256]");
    H = h > H ? h : H;
  }
  if (pi->activation != policy::ACT_TANH && pi->activation != policy::ACT_RELU) return fail("anm_policy_ppo_grad: activation must be ANM_POLICY_TANH or ANM_POLICY_RELU");
  for (int32_t code : {job->io_dtype, job->value_dtype})
    if (code != ANM_IO_F64 && code != ANM_IO_F32) return fail("anm_policy_ppo_grad: io_dtype and value_dtype must be ANM_IO_F64 or ANM_IO_F32");
  if (job->B < 1 || job->B > (int64_t(1) << 24)) return fail("anm_policy_ppo_grad: B is outside [1, 2^24]");
  if (job->rows_per_partial < policy::ROWS || job->rows_per_partial % policy::ROWS != 0)
    return fail("anm_policy_ppo_grad: rows_per_partial is not a positive multiple of 32");
  if (!(job->clip > 0.0f) || !std::isfinite(job->clip)) return fail("anm_policy_ppo_grad: clip is not a positive finite number");
  if (!std::isfinite(job->vf_coef) || !std::isfinite(job->ent_coef) || !std::isfinite(job->vf_clip))
    return fail("anm_policy_ppo_grad: vf_coef, ent_coef and vf_clip must be finite (vf_clip < 0: off)");
  ppo::Args a{};
  int32_t at = 0;
  policy_net(a.p.actor, pi, pi->A, at);
  policy_net(a.p.critic, pi, 1, at);
  a.p.log_std = at;
  at += pi->A;
  if (pi->n_params != at) return fail("anm_policy_ppo_grad: n_params is not the size of the layout (actor, critic, log_std)");
  if (!pi->params || !job->obs || !job->actions || !job->logp_old || !job->returns || !job->adv || !job->weight)
    return fail("anm_policy_ppo_grad: params and the minibatch's obs, actions, logp_old, returns, adv and weight must be set");
  if (job->vf_clip >= 0.0f && !job->values_old) return fail("anm_policy_ppo_grad: values_old must be set when vf_clip is on");
  if (!job->grad || !job->partials || !job->ratio || !job->logp || !job->values || !job->inv_std || !job->stats)
    return fail("anm_policy_ppo_grad: grad, partials, ratio, logp, values, inv_std and stats must be set");
  const int wide = H > pi->A ? H : pi->A;
  a.p.S = ((pi->D > wide ? pi->D : wide) + 1) | 1;       // (one column more than the widest layer: the 1.0 of the bias)
  a.SE = (pi->A + ppo::STATS) | 1;
  a.n_tiles = pi->n_hidden + 2;
  for (int net = 0; net < 2; ++net) {
    const policy::Net& nn = net ? a.p.critic : a.p.actor;
    int32_t* off = net ? a.wt_critic : a.wt_actor;
    for (int i = 1; i < nn.n_layers; ++i) {
      off[i] = a.wt_floats;
      a.wt_floats += ((nn.N[i] + 1) & ~1) * nn.K[i];
    }
  }
  int waves = ppo::MAX_WAVES;
  while (waves >= 1 && ppo::lds_floats(at, a.wt_floats, a.n_tiles, a.p.S, a.SE, waves) * 4 > policy::LDS_BYTES) waves >>= 1;
  if (waves < 1) return fail("anm_policy_ppo_grad: the network does not fit the backward LDS plan (policy_grad.grad_lds_floats above 40 960)");
  a.p.params = pi->params;
  a.p.n_params = at;
  a.p.D = pi->D;
  a.p.A = pi->A;
  a.p.activation = pi->activation;
  a.p.logp0 = float(-0.5 * double(pi->A) * std::log(2.0 * 3.141592653589793));
  a.p.obs = job->obs;
  a.p.vec4 = reinterpret_cast<uintptr_t>(pi->params) % 16 == 0 ? 1 : 0;
  a.actions = job->actions;
  a.logp_old = job->logp_old;
  a.v_old = job->values_old;
  a.returns = job->returns;
  a.adv = job->adv;
  a.weight = job->weight;
  a.partials = job->partials;
  a.ratio = job->ratio;
  a.logp = job->logp;
  a.values = job->values;
  a.inv_std = job->inv_std;
  a.B = job->B;
  a.R = job->rows_per_partial;
  a.clip_lo = 1.0f - job->clip;
  a.clip_hi = 1.0f + job->clip;
  a.vf_coef = job->vf_coef;
  a.vf_clip = job->vf_clip < 0.0f ? -1.0f : job->vf_clip;
  const size_t lds = size_t(ppo::lds_floats(at, a.wt_floats, a.n_tiles, a.p.S, a.SE, waves)) * 4;
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, n = 0;
    n_cu = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : -1;
  }
  // a wavefront takes whole groups of rows_per_partial rows, a workgroup `waves` of them at a time; the grid decides only
  // which wavefront computes a group, never what it computes
  const int64_t G = (job->B + a.R - 1) / a.R;
  const int64_t n_wg = (G + waves - 1) / waves;
  const int64_t resident = n_cu > 0 ? int64_t(n_cu) * int64_t(policy::LDS_BYTES / lds) : n_wg;
  const unsigned grid = unsigned(n_wg < resident ? n_wg : resident);
  ppo::ReduceArgs r{};
  r.partials = job->partials;
  r.params = pi->params;
  r.grad = job->grad;
  r.stats = job->stats;
  r.P = at;
  r.A = pi->A;
  r.log_std = a.p.log_std;
  r.G = G;
  r.vf_coef = job->vf_coef;
  r.ent_coef = job->ent_coef;
  r.ent_const = float(0.5 + 0.5 * std::log(2.0 * 3.141592653589793));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool i32 = job->io_dtype == ANM_IO_F32, v32 = job->value_dtype == ANM_IO_F32;
  static bool raised[4] = {false, false, false, false};
  auto go = [&](auto kernel, int which) {
    if (!raised[which]) {
      hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, policy::LDS_BYTES);
      if (e != hipSuccess) return fail_hip(e, "anm_policy_ppo_grad: hipFuncSetAttribute");
      raised[which] = true;
    }
    return launch("launch k_ppo_grad", kernel, grid, unsigned(waves * 64), lds, s, a);
  };
  const int rc = i32 ? (v32 ? go(ppo::k_ppo_grad<true, true>, 0) : go(ppo::k_ppo_grad<true, false>, 1))
                     : (v32 ? go(ppo::k_ppo_grad<false, true>, 2) : go(ppo::k_ppo_grad<false, false>, 3));
  if (rc != 0) return rc;
  const unsigned rgrid = unsigned((at + ppo::REDUCE_THREADS - 1) / ppo::REDUCE_THREADS) + 1;
  return launch("launch k_ppo_reduce", ppo::k_ppo_reduce, rgrid, ppo::REDUCE_THREADS, 0, s, r);
}

int anm_model_bind_view(anm_model* m, const anm_batch_view* v) {
  if (!m) return fail("anm_model_bind_view: null model");
  if (!v) {
    m->view = radial::View{};
    m->has_view = false;
    return 0;
  }
  if (m->d_env_class) return fail("anm_model_bind_view: not together with parameter classes (anm_model_bind_env_classes)");
  if (m->exo_mode == ANM_EXO_SERIES_NOISE) return fail("anm_model_bind_view: a batch view does not go with the series-noise mode");
  if (m->io_mode == ANM_IO_F32) return fail("anm_model_bind_view: a batch view does not go with the float32 I/O mode (anm_model_set_io)");
  if (m->d_iomap.get()) return fail("anm_model_bind_view: a batch view does not go with the affine I/O map (anm_model_set_io_map)");
  if (m->n_obs > 0 && m->impl == ANM_IMPL_THREAD)
    return fail("anm_model_bind_view: the thread-per-environment family gathers no list-form observation through a view "
                "(anm_model_set_obs): clear it, or move the model to a lane-group family first (anm_model_set_impl)");
  if (m->n_obs > 0 && v->w_obs != 0 && v->w_obs < m->n_obs) return fail("anm_model_bind_view: w_obs is narrower than the observation list");
  if (m->d_state_same) return fail("anm_model_bind_view: not together with anm_model_bind_state_same (the flags are indexed by launch slot)");
  if (m->ep.on)
    return fail("anm_model_bind_view: a batch view does not go with an episode time limit or episode buffers (anm_env_config.max_episode_steps / .episode)");
  const anm_dims& d = m->dims;
  const int K = m->K;
  const int n_set = d.n_gen + d.n_des;
  struct { int given, own; const char* what; } w[] = {
      {v->w_load, d.n_load, "w_load"}, {v->w_gen, d.n_gen, "w_gen"}, {v->w_set, n_set, "w_set"}, {v->w_des, d.n_des, "w_des"},
      {v->w_action, 2 * n_set, "w_action"}, {v->w_state, d.state_base_dim + K, "w_state"}, {v->w_exo, d.n_load + d.n_gen, "w_exo"},
      {v->w_aux, K, "w_aux"}, {v->w_full, d.full_dim, "w_full"}};
  for (auto& x : w)
    if (x.given != 0 && x.given < x.own) {
      g_err = std::string("anm_model_bind_view: ") + x.what + " is narrower than this network's own rows";
      return -1;
    }
  m->view = radial::View{v->env_index, v->w_load, v->w_gen, v->w_set, v->w_des, v->w_action, v->w_state, v->w_exo, v->w_aux, v->w_full, v->w_obs};
  m->has_view = true;
  return 0;   // (every kernel family serves a view: the model stays in the family it is in)
}

int anm_step_ws_record_doubles(void) { return Rec<Topo>::SIZE; }

static unsigned magic_div(int d) { return d > 0 ? unsigned((0x100000000ull + uint64_t(d) - 1) / uint64_t(d)) : 0u; }

int anm_model_obs_fusable(const anm_model* m) {
  if (!m) return 0;
  if (m->has_view && m->impl == ANM_IMPL_THREAD) return 0;   // (its step through a view moves rows per lane: no LDS rows to gather from)
  if (m->impl == ANM_IMPL_THREAD) return (m->t_thread.ok && GenLds<Topo>::FULL_OK) ? 1 : 0;
  if (m->impl == ANM_IMPL_RADIAL) return (m->t_radial.ok && radial_obs_lds_bytes(m) <= 48 * 1024) ? 1 : 0;
  if (m->impl == ANM_IMPL_MESH) return (m->t_mesh.ok && m->mplan.d.l_bw - m->mplan.d.l_blk >= m->mplan.d.FS + radial::KMAX) ? 1 : 0;
  return 0;
}
int anm_model_set_obs(anm_model* m, int32_t n_obs, const int32_t* index, const double* scale, const double* low,
                      const double* high) {
  if (!m) return fail("anm_model_set_obs: null model");
  if (m->d_iomap.get())
    return fail("anm_model_set_obs: an affine I/O map is set (anm_model_set_io_map), whose observation tables have the length of the "
                "observation that was set: clear it first (NULL) and set it again afterwards");
  if (n_obs <= 0) {   // back to the "state" observation
    m->d_obs_index.reset(); m->d_obs_tab.reset(); m->n_obs = 0;
    return 0;
  }
  // (a refused list leaves the one that is set as it was: checks and uploads first, the model last)
  if (!anm_model_obs_fusable(m))
    return fail("anm_model_set_obs: this model cannot gather inside the step kernel (use anm_gather_obs_f64)");
  if (!index || !scale || !low || !high) return fail("anm_model_set_obs: null argument");
  if (n_obs > 4096) return fail("anm_model_set_obs: more than 4096 observation entries");
  if (m->has_view && m->view.w_obs != 0 && m->view.w_obs < n_obs) return fail("anm_model_set_obs: the bound view's w_obs is narrower than the list");
  // the family in use: the offsets of `full` (the same in all three, full_offsets), the aux slots a row has behind them
  const bool thread = m->impl == ANM_IMPL_THREAD;
  const int* base = m->full.base;
  const int FS = base[FC_COUNT], aux_slots = thread ? int(Layout<Topo>::KMAX) : int(radial::KMAX);
  auto class_of = [&](int i) {
    unsigned c = 0;
    while (c + 1 < FC_COUNT && base[c + 1] <= i) ++c;
    return c;
  };
  unsigned need = 0;   // the classes the list reads
  std::vector<int32_t> idx(2 * size_t(n_obs));
  for (int k = 0; k < n_obs; ++k) {
    const int i = index[k];
    // (the aux slots behind the electrical state: only the K of the task are written, anm_model_set_env)
    if (i < 0 || i >= FS + (m->env_set ? m->K : aux_slots)) return fail("anm_model_set_obs: index out of range");
    if (i < FS) need |= 1u << class_of(i);
    idx[k] = idx[n_obs + k] = i;   // (both halves: the identity layout -- `full` offsets, aux behind them)
  }
  short cls_off[FC_COUNT] = {0};
  int aux_off = 0;
  if (thread) {
    // thread family: rows of the compact layout (only the classes the list reads) unless the dump is asked for; the
    // first half of the indices points into those.  The lane-group families gather from the identity layout alone
    for (unsigned c = 0; c < FC_COUNT; ++c) {
      cls_off[c] = short(aux_off);
      if ((need >> c) & 1u) aux_off += base[c + 1] - base[c];
    }
    for (int k = 0; k < n_obs; ++k) {
      const int i = index[k];
      idx[k] = i >= FS ? aux_off + (i - FS) : cls_off[class_of(i)] + (i - base[class_of(i)]);
    }
  }
  std::vector<double> tab(3 * size_t(n_obs));
  for (int k = 0; k < n_obs; ++k) { tab[k] = scale[k]; tab[n_obs + k] = low[k]; tab[2 * n_obs + k] = high[k]; }
  DevBuf<int32_t> d_index;
  DevBuf<double> d_tab;
  hipError_t e = d_index.assign(idx.data(), idx.size());
  if (e == hipSuccess) e = d_tab.assign(tab.data(), tab.size());
  if (e != hipSuccess) return fail_hip(e, "anm_model_set_obs");
  if (thread) {
    std::copy(cls_off, cls_off + FC_COUNT, m->obs_cls_off);
    m->obs_aux_off = aux_off;
    m->obs_row_stride = (aux_off + Layout<Topo>::KMAX) | 1;
  }
  m->d_obs_index = std::move(d_index);
  m->d_obs_tab = std::move(d_tab);
  m->obs_need = need;
  m->n_obs = n_obs;
  return 0;
}

int anm_model_set_impl(anm_model* m, int32_t impl) {
  if (!m) return fail("anm_model_set_impl: null model");
  if (impl == ANM_IMPL_RADIAL && !m->t_radial.ok)
    return fail("the lane-group kernel needs a radial (tree) network with at most 64 buses and devices");
  if (impl == ANM_IMPL_MESH && !m->t_mesh.ok)
    return fail("the general lane-group kernel needs a network of at most 65 buses, 128 branches, 64 devices");
  if (impl != ANM_IMPL_THREAD && impl != ANM_IMPL_RADIAL && impl != ANM_IMPL_MESH)
    return fail("anm_model_set_impl: unknown implementation");
  if (impl == ANM_IMPL_THREAD && !m->t_thread.ok)
    return fail("this library was compiled for another topology: only the generic lane-group kernel is available");
  if (impl == ANM_IMPL_THREAD && m->class_per_env)
    return fail("anm_model_set_impl: the bound parameter classes change inside blocks of 64 environments: only a "
                "lane-group kernel can serve them");
  if (impl != m->impl && m->n_obs > 0)
    return fail("anm_model_set_impl: a list-form observation is set (anm_model_set_obs), whose tables belong to the current "
                "kernel family; clear it before switching and set it again afterwards");
  m->impl = impl;
  m->impl_unbound = -1;   // an explicit choice is not undone by a later unbind
  return 0;
}

int anm_model_get_impl(const anm_model* m) { return m ? m->impl : -1; }
int anm_model_lanes_per_env(const anm_model* m) {
  if (!m) return -1;
  return m->impl == ANM_IMPL_MESH ? m->mplan.d.G : (m->impl == ANM_IMPL_RADIAL ? m->plan.d.G : 1);
}

int anm_model_get_ybus(const anm_model* m, double* y) {
  if (!m || !y) return fail("anm_model_get_ybus: null argument");
  for (size_t k = 0; k < m->ybus.size(); ++k) {
    y[2 * k] = m->ybus[k].real();
    y[2 * k + 1] = m->ybus[k].imag();
  }
  return 0;
}

int anm_transition_f64(anm_model* m, int64_t n, const double* p_load, const double* p_pot, const double* p_set,
                       const double* q_set, double* soc, double* full, double* reward, double* e_loss,
                       double* penalty, uint8_t* converged, int32_t* nr_iters, const anm_solver_opts* opts,
                       void* stream) {
  if (!m) return fail("anm_transition_f64: null model");
  if (n <= 0) return 0;
  if (!reward || !e_loss || !penalty || !converged) return fail("anm_transition_f64: null output");
  TransitionIO io{p_load, p_pot, p_set, q_set, soc, full, reward, e_loss, penalty, converged, nr_iters, m->d_nr_diff, m->d_nr_start};
  int prec;
  SolverOpts so = solver(opts, prec);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (on_lane_groups(m)) return launch_lane_groups(m, 0, &io, nullptr, prec, n, s, so);
  return by_precision(prec, [&](auto jt) {
    using JT = decltype(jt);
    auto kern = io.nr_start ? k_transition<JT, true, true> : m->has_view ? k_transition<JT, true> : k_transition<JT, false>;
    return launch("launch k_transition", kern, grid_for(n), BLOCK, 0, s, (cptr_t)m->t_thread.dev.get(), io, so, n, class_sel(m, m->t_thread), m->view);
  });
}

// What a reset and a step take from the model alike: the task's exogenous mode and tables, the episode settings and the
// I/O mode -- and what of these a bound batch view does not go with.  `who`: the entry point, for the error texts.
static int env_io_of_model(const anm_model* m, const char* who, EnvIO& io) {
  io = EnvIO{};
  io.K = m->K;
  io.exo_mode = m->exo_mode;
  io.exo_lo = m->d_exo.get();
  io.exo_hi = m->exo_mode != ANM_EXO_HOST ? m->d_exo.get() + (m->dims.n_load + m->dims.n_gen) : nullptr;
  io.exo_noise = m->exo_mode == ANM_EXO_SERIES_NOISE ? m->d_noise.get() : nullptr;
  if (m->exo_mode == ANM_EXO_SERIES_NOISE && m->d_corr.get()) {
    io.exo_rho = m->d_corr.get();
    io.exo_innov = m->d_corr.get() + (m->dims.n_load + m->dims.n_gen);
    io.exo_z = m->exo_z;
  }
  io.forecast = m->exo_mode == ANM_EXO_SERIES_NOISE ? m->d_forecast.get() : nullptr;   // expected forecast (null: off)
  io.series = m->d_series.get();
  io.period = m->period;
  io.ep = m->ep;
  io.io32 = m->io_mode == ANM_IO_F32 ? 1 : 0;
  io.iomap = m->d_iomap.get();
  if (m->has_view) {
    const std::string w(who);
    if (io.iomap) return fail((w + ": the affine I/O map (anm_model_set_io_map) does not go with a batch view (anm_model_bind_view)").c_str());
    if (io.io32) return fail((w + ": the float32 I/O mode (anm_model_set_io) does not go with a batch view (anm_model_bind_view)").c_str());
    if (io.ep.on) return fail((w + ": an episode time limit or episode buffers do not go with a batch view (anm_model_bind_view)").c_str());
  }
  return 0;
}

int anm_reset_f64(anm_model* m, int64_t n, const double* init_state, const uint8_t* mask, uint64_t rng_seed,
                  uint64_t env_offset, int32_t* reset_count, double* soc, double* state,
                  double* obs, uint8_t* converged, uint8_t* terminated, int32_t* timestep, int32_t* nr_iters,
                  double* full, int32_t* aux_index, const anm_solver_opts* opts, void* stream) {
  if (!m) return fail("anm_reset_f64: null model");
  if (!m->env_set) return fail("anm_reset_f64: call anm_model_set_env first");
  if (n <= 0) return 0;
  if (!state || !obs || !converged || !terminated) return fail("anm_reset_f64: null argument");
  const bool uniform = m->exo_mode == ANM_EXO_UNIFORM;
  if (!init_state && ((m->period <= 0 && !uniform) || m->K != 1 || !reset_count))
    return fail("anm_reset_f64: drawing initial states on the device needs a series-mode or uniform-mode model and reset_count");
  if (uniform && (m->has_view || m->d_env_class))
    return fail("anm_reset_f64: the uniform exogenous mode goes with neither a batch view nor parameter classes");
  if (m->exo_mode == ANM_EXO_SERIES_NOISE && (m->has_view || m->d_env_class))
    return fail("anm_reset_f64: the series-noise mode goes with neither a batch view nor parameter classes");
  if (m->exo_mode == ANM_EXO_SERIES_NOISE && m->d_corr.get() && !reset_count)
    return fail("anm_reset_f64: correlated noise needs reset_count (the epoch keys the noise state every reset stores)");
  EnvIO io;
  if (int rc = env_io_of_model(m, "anm_reset_f64", io)) return rc;
  // (a list-form observation is set: this launch writes the "state" form, whose rows are not the length of the map's tables --
  // left raw, and the caller maps the list it gathers afterwards: io_affine.py, reset)
  if (m->n_obs > 0) io.iomap = nullptr;
  io.init_state = init_state;
  io.rng_seed = rng_seed;
  io.env_offset = env_offset;
  io.reset_count = reset_count;
  io.mask = mask;
  io.soc = soc;
  io.state = state;
  io.obs = obs;
  io.converged = converged;
  io.terminated = terminated;
  io.timestep = timestep;
  io.nr_iters = nr_iters;
  io.full = full;
  io.aux_index = aux_index;
  io.nr_diff = m->d_nr_diff;
  int prec;
  SolverOpts so = solver(opts, prec);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (on_lane_groups(m)) return launch_lane_groups(m, 1, nullptr, &io, prec, n, s, so);
  return by_precision(prec, [&](auto jt) {
    using JT = decltype(jt);
    return launch("launch k_reset", m->has_view ? k_reset<JT, true> : k_reset<JT, false>, grid_for(n), BLOCK, 0, s, (cptr_t)m->t_thread.dev.get(), io,
                  so, n, class_sel(m, m->t_thread), m->view);
  });
}

int anm_sample_init_state_f64(anm_model* m, int64_t n, uint64_t rng_seed, uint64_t env_offset, const int32_t* reset_count,
                              double* init_state, uint32_t* raw, void* stream) {
  if (!m || !init_state) return fail("anm_sample_init_state_f64: null argument");
  const bool uniform = m->env_set && m->exo_mode == ANM_EXO_UNIFORM;
  if (!uniform && (!m->env_set || m->period <= 0 || m->K != 1 || !m->d_series.get()))
    return fail("anm_sample_init_state_f64: the model needs a series-mode or uniform-mode task (anm_model_set_env with series or exo_mode, K = 1)");
  if (m->d_env_class) return fail("anm_sample_init_state_f64: not while parameter classes are bound (the table is class 0's)");
  if (n <= 0) return 0;
  const int n_blocks = 1 + (m->s_ngen + m->s_ndes + 1) / 2;
  const bool noisy = m->exo_mode == ANM_EXO_SERIES_NOISE;
  const double* exo_lo = (uniform || noisy) ? m->d_exo.get() : nullptr;
  return launch("launch k_sample_init_state", k_sample_init_state, unsigned((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), n,
                m->s_nd, m->s_nload, m->s_ngen, m->s_ndes, m->d_samp.get(), (const double*)m->d_series.get(), m->period, rng_seed, env_offset,
                (const int32_t*)reset_count, init_state, raw, n_blocks, exo_lo, (const double*)(noisy ? m->d_noise.get() : nullptr));
}

static int make_step_io(anm_model* m, const double* action, const double* exo, const double* aux_next, double* soc,
                        double* state, uint8_t* terminated, int32_t* timestep, double* obs, double* reward,
                        double* e_loss, double* penalty, int32_t* nr_iters, double* full, int32_t autoreset,
                        uint64_t rng_seed, uint64_t env_offset, int32_t* reset_count, int32_t* aux_index, const anm_step_ws* ws,
                        EnvIO& io) {
  if (!m) return fail("anm_step_f64: null model");
  if (!m->env_set) return fail("anm_step_f64: call anm_model_set_env first");
  // (a network without set-point devices has an empty action vector: examples/simple_env.py of the reference)
  if ((!action && m->dims.action_dim > 0) || !state || !terminated || !obs || !reward || !e_loss || !penalty)
    return fail("anm_step_f64: null argument");
  if (m->dims.n_des > 0 && !soc) return fail("anm_step_f64: null soc");
  const bool series = exo == nullptr;
  const bool uniform = m->exo_mode == ANM_EXO_UNIFORM;
  if (uniform) {
    if (exo || aux_next) return fail("anm_step_f64: the uniform exogenous mode draws P_load / P_pot in the kernel: exo and aux_next must be NULL");
    if (!reset_count) return fail("anm_step_f64: the uniform exogenous mode needs reset_count (the epoch is part of the key of every draw)");
    if (m->has_view) return fail("anm_step_f64: the uniform exogenous mode does not go with a batch view (anm_model_bind_view)");
    if (m->d_env_class) return fail("anm_step_f64: the uniform exogenous mode does not go with parameter classes (anm_model_bind_env_classes)");
  }
  if (m->exo_mode == ANM_EXO_SERIES_NOISE) {
    if (exo || aux_next) return fail("anm_step_f64: the series-noise mode draws P_load / P_pot in the kernel: exo and aux_next must be NULL");
    if (!timestep) return fail("anm_step_f64: the series-noise mode needs the timestep buffer (the step index of the episode keys every draw)");
    if (!reset_count) return fail("anm_step_f64: the series-noise mode needs reset_count (the epoch is part of the key of every draw)");
    if (m->has_view) return fail("anm_step_f64: the series-noise mode does not go with a batch view (anm_model_bind_view)");
    if (m->d_env_class) return fail("anm_step_f64: the series-noise mode does not go with parameter classes (anm_model_bind_env_classes)");
  }
  if (series && !uniform && m->period <= 0) return fail("anm_step_f64: no exo given and the model has no series (set_env)");
  if (!series && m->K > 0 && !aux_next) return fail("anm_step_f64: exo given without aux_next");
  if (autoreset && (!series || !reset_count)) return fail("anm_step_f64: autoreset needs series mode and reset_count");
  if (int rc = env_io_of_model(m, "anm_step_f64", io)) return rc;
  io.action = action;
  io.exo = exo;
  io.aux_next = aux_next;
  io.soc = soc;
  io.state = state;
  io.terminated = terminated;
  io.timestep = timestep;
  io.obs = obs;
  io.reward = reward;
  io.e_loss = e_loss;
  io.penalty = penalty;
  io.nr_iters = nr_iters;
  io.full = full;
  io.autoreset = autoreset;
  io.rng_seed = rng_seed;
  io.env_offset = env_offset;
  io.reset_count = reset_count;
  io.aux_index = aux_index;
  io.state_same = m->d_state_same;
  if (io.ep.on && !timestep) return fail("anm_step_f64: an episode time limit or episode buffers need the timestep buffer");
  if (io.io32 && full && m->n_obs == 0)
    return fail("anm_step_f64: the float32 I/O mode (anm_model_set_io) has no unfused observation gather: `full` + anm_gather_obs_f64 "
                "writes float64 observations; set the list in the kernel (anm_model_set_obs) or leave `full` NULL");
  if (io.iomap && full && m->n_obs == 0)
    return fail("anm_step_f64: the affine I/O map (anm_model_set_io_map) has no unfused observation gather: `full` + anm_gather_obs_f64 "
                "writes unmapped observations; set the list in the kernel (anm_model_set_obs) or leave `full` NULL");
  io.n_obs = 0;
  io.state_magic = magic_div(m->dims.state_base_dim + m->K);
  if (m->t_thread.ok && m->impl == ANM_IMPL_THREAD && (m->n_obs > 0 || full)) {
    // rows of the electrical state in LDS: identity layout when the dump is asked for, else only the classes
    // the observation list reads
    const bool ident = full != nullptr;
    io.n_obs = m->n_obs;
    io.obs_magic = magic_div(m->n_obs);
    io.obs_need = ident ? ~0u : m->obs_need;
    io.row_stride = ident ? GenLds<Topo>::FSP : m->obs_row_stride;
    io.aux_off = ident ? FullState<Topo>::SIZE : m->obs_aux_off;
    for (unsigned cc = 0; cc < FC_COUNT; ++cc)
      io.cls_off[cc] = ident ? short(full_class_base<Topo>(cc)) : m->obs_cls_off[cc];
    if (m->n_obs > 0) {
      io.obs_index = m->d_obs_index.get() + (ident ? m->n_obs : 0);
      io.obs_scale = m->d_obs_tab.get();
      io.obs_lo = m->d_obs_tab.get() + m->n_obs;
      io.obs_hi = m->d_obs_tab.get() + 2 * m->n_obs;
    }
  }
  if (m->impl != ANM_IMPL_THREAD && m->n_obs > 0) {   // lane-group families: identity layout (see anm_model_set_obs)
    io.n_obs = m->n_obs;
    io.obs_need = m->obs_need;
    io.obs_index = m->d_obs_index.get();
    io.obs_scale = m->d_obs_tab.get();
    io.obs_lo = m->d_obs_tab.get() + m->n_obs;
    io.obs_hi = m->d_obs_tab.get() + 2 * m->n_obs;
  }
  io.ws = nullptr;
  if (ws && ws->buf && m->t_thread.ok && !m->d_env_class) {  // (the straggler launch packs records of all blocks together)
    // records, then the int32 list of the records the first straggler launch leaves to the second
    const int64_t cap = 2 * (ws->n_doubles - Rec<Topo>::HEADER) / (2 * Rec<Topo>::SIZE + 1);
    if (cap < 1 || ws->iter_cap < 1) return fail("anm_step_f64: step workspace too small or iter_cap < 1");
    io.ws = ws->buf;
    io.ws_cap = cap;
    io.iter_cap = ws->iter_cap;
    io.ws_list2 = reinterpret_cast<int32_t*>(ws->buf + Rec<Topo>::HEADER + cap * Rec<Topo>::SIZE);
    io.mid_cap = ws->mid_cap == 0 ? ANM_MID_CAP_DEFAULT : (ws->mid_cap < 0 ? 0 : ws->mid_cap);
    if (io.mid_cap > 0 && io.mid_cap <= io.iter_cap) io.mid_cap = 0;
  }
  return 0;
}

static int launch_step(anm_model* m, const EnvIO& io_in, int64_t n, const anm_solver_opts* opts, hipStream_t s) {
  EnvIO io = io_in;
  int prec;
  SolverOpts so = solver(opts, prec);
  auto clear_state_same = [&]() {   // a kernel that writes every state row: no row is "the same as obs and left out"
    hipError_t em = io.state_same ? hipMemsetAsync(io.state_same, 0, size_t(n), s) : hipSuccess;
    return em == hipSuccess ? 0 : fail_hip(em, "hipMemsetAsync(state_same)");
  };
  if (on_lane_groups(m)) {
    if (int rc = clear_state_same()) return rc;
    return launch_lane_groups(m, 2, nullptr, &io, prec, n, s, so);
  }
  const cptr_t C = (cptr_t)m->t_thread.dev.get();
  const unsigned grid = grid_for(n);
  if (m->has_view) {
    // a batch view: per-lane rows (the coalesced-row kernels need 64 consecutive environments)
    if (io.K > 1) return fail("anm_step_f64: a batch view in the thread-per-environment family takes K <= 1 auxiliary variables (use the general lane-group family)");
    if (io.n_obs > 0) return fail("anm_step_f64: a batch view and a list-form observation do not go together");
    io.ws = nullptr;
    io.state_same = nullptr;
    io.aux_stride = m->view.w_aux;
    const bool dense = m->view_waves ? m->view_waves == 2 : n > int64_t(2) * 64 * 4 * 256;   // more than two wavefronts per SIMD of the chip
    return by_precision(prec, [&](auto jt) {
      using JT = decltype(jt);
      return launch("launch k_step_view", dense ? k_step_view<JT, 2> : k_step_view<JT, 1>, grid, BLOCK, 0, s, C, io, so, n, m->view);
    });
  }
  const ClassSel cs = class_sel(m, m->t_thread);
  if (io.aux_index && io.exo == nullptr && io.exo_mode == ANM_EXO_HOST && io.K == 1 && !io.full && io.n_obs == 0) {
    // fast path: series mode, "state" observation, nothing but the batch tensors
    int rc = by_precision(prec, [&](auto jt) {
      if (io.iomap) {
        if (io.io32) return launch("launch k_step_rows_map", k_step_rows_map<decltype(jt), true>, grid, BLOCK, 0, s, C, io, so, n, cs);
        return launch("launch k_step_rows_map", k_step_rows_map<decltype(jt), false>, grid, BLOCK, 0, s, C, io, so, n, cs);
      }
      if (io.io32) {
        if (io.ep.on) return launch("launch k_step_rows_io32", k_step_rows_io32<decltype(jt), true>, grid, BLOCK, 0, s, C, io, so, n, cs);
        return launch("launch k_step_rows_io32", k_step_rows_io32<decltype(jt), false>, grid, BLOCK, 0, s, C, io, so, n, cs);
      }
      if (io.ep.on) return launch("launch k_step_rows_ep", k_step_rows_ep<decltype(jt)>, grid, BLOCK, 0, s, C, io, so, n, cs);
      return launch("launch k_step_rows", k_step_rows<decltype(jt), false>, grid, BLOCK, 0, s, C, io, so, n, cs);
    });
    if (rc || !(io.ws && io.iter_cap < so.max_iter)) return rc;
    // second launch: the handed-over solves, grid-stride over the records (count lives on the device)
    // (a tree topology continues them on lane groups, 8 records per wavefront, unless that was switched off)
    const bool groups = Topo::TREE != 0 && so.handoff >= 0;
    const int per_block = groups ? group::Shape<Topo>::NG : BLOCK;
    const unsigned g2 = unsigned((io.ws_cap + per_block - 1) / per_block);  // covers every record
    const bool two_level = groups && io.mid_cap > 0 && io.mid_cap < so.max_iter;
    for (int level = 1; level <= (two_level ? 2 : 1) && rc == 0; ++level)   // (level 2: most wavefronts find nothing and leave)
      rc = by_precision(prec, [&](auto jt) {
        using JT = decltype(jt);
        if constexpr (Topo::TREE != 0)
          if (groups) return launch("launch k_step_stragglers", k_step_stragglers<JT, true>, g2, BLOCK, 0, s, C, io, so, level);
        return launch("launch k_step_stragglers", k_step_stragglers<JT, false>, g2, BLOCK, 0, s, C, io, so, level);
      });
    if (rc) return rc;
    const unsigned g3 = unsigned((int64_t(io.ws_cap) * SCATTER_LANES + 255) / 256);
    return launch("launch k_step_scatter", k_step_scatter, g3, 256, 0, s, io);
  }
  io.ws = nullptr;
  if (int rc = clear_state_same()) return rc;
  if (io.full && !GenLds<Topo>::FULL_OK) {  // rows too wide for LDS: plain per-lane dump, no fused list
    io.n_obs = 0;
  }
  // dynamic LDS: the widest of the buffers op_step_general overlays
  const int S = Topo::SDIM + io.K;
  size_t doubles = size_t(GenLds<Topo>::G_MIN);
  doubles = std::max(doubles, size_t(64) * size_t(Dims<Topo>::ADIM + 1));
  if (GenLds<Topo>::FULL_OK && (io.n_obs > 0 || io.full)) doubles = std::max(doubles, size_t(64) * size_t(io.row_stride));
  io.state_row_off = int(doubles);               // the state rows follow the buffer the other uses overlay
  const size_t lds_bytes = (doubles + size_t(64) * size_t(S | 1)) * sizeof(double);
  return by_precision(prec, [&](auto jt) {
    if (io.forecast) return launch("launch k_step_general_fc", k_step_general_fc<decltype(jt)>, grid, BLOCK, lds_bytes, s, C, io, so, n, cs);
    return launch("launch k_step_general", k_step_general<decltype(jt)>, grid, BLOCK, lds_bytes, s, C, io, so, n, cs);
  });
}

int anm_step_f64(anm_model* m, int64_t n, const double* action, const double* exo, const double* aux_next,
                 double* soc, double* state, uint8_t* terminated, int32_t* timestep, double* obs, double* reward,
                 double* e_loss, double* penalty, int32_t* nr_iters, double* full, int32_t autoreset,
                 uint64_t rng_seed, uint64_t env_offset, int32_t* reset_count, int32_t* aux_index, const anm_step_ws* ws,
                 const anm_solver_opts* opts, void* stream) {
  EnvIO io;
  int rc = make_step_io(m, action, exo, aux_next, soc, state, terminated, timestep, obs, reward, e_loss, penalty,
                        nr_iters, full, autoreset, rng_seed, env_offset, reset_count, aux_index, ws, io);
  if (rc) return rc;
  if (n <= 0) return 0;
  return launch_step(m, io, n, opts, static_cast<hipStream_t>(stream));
}

int anm_time_step_launches(anm_model* m, int64_t n, const double* action, double* soc, double* state,
                           uint8_t* terminated, int32_t* timestep, double* obs, double* reward, double* e_loss,
                           double* penalty, int32_t autoreset, uint64_t rng_seed, uint64_t env_offset, int32_t* reset_count,
                           int32_t* aux_index, anm_step_ws* ws, const anm_solver_opts* opts, void* stream, int32_t n_launch,
                           float* ms_per_launch) {
  EnvIO io;
  int rc = make_step_io(m, action, nullptr, nullptr, soc, state, terminated, timestep, obs, reward, e_loss, penalty,
                        nullptr, nullptr, autoreset, rng_seed, env_offset, reset_count, aux_index, ws, io);
  if (rc) return rc;
  if (n <= 0 || n_launch <= 0 || !ms_per_launch) return fail("anm_time_step_launches: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipEvent_t t0, t1;
  hipError_t e;
  if ((e = hipEventCreate(&t0)) != hipSuccess) return fail_hip(e, "hipEventCreate");
  if ((e = hipEventCreate(&t1)) != hipSuccess) return fail_hip(e, "hipEventCreate");
  hipEventRecord(t0, s);
  for (int k = 0; k < n_launch && rc == 0; ++k) {
    rc = launch_step(m, io, n, opts, s);
  }
  hipEventRecord(t1, s);
  e = hipEventSynchronize(t1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
  hipEventDestroy(t0);
  hipEventDestroy(t1);
  if (rc) return rc;
  if (e != hipSuccess) return fail_hip(e, "event timing");
  *ms_per_launch = ms / float(n_launch);
  return 0;
}

#include "anm_mpc_capi.inc"

int anm_gather_obs_f64(int64_t n, int32_t full_dim, const double* full, int32_t state_dim, int32_t K,
                       const double* state, const uint8_t* terminated, int32_t n_obs, const int32_t* index,
                       const double* scale, const double* low, const double* high, double* obs, void* stream) {
  if (!full || !index || !scale || !low || !high || !obs) return fail("anm_gather_obs_f64: null argument");
  if (K > 0 && !state) return fail("anm_gather_obs_f64: aux variables need the state array");
  if (n <= 0 || n_obs <= 0) return 0;
  const int64_t total = n * n_obs;
  unsigned grid = unsigned(std::min<int64_t>((total + 255) / 256, 2048));
  return launch("launch k_gather_obs", k_gather_obs, grid, 256, 0, static_cast<hipStream_t>(stream), n, int(full_dim), full, int(state_dim),
                int(K), state, terminated, int(n_obs), index, scale, low, high, obs);
}

int anm_test_row_dpp(const double* acc, const double* x, double* out, void* stream) {
  if (!acc || !x || !out) return fail("anm_test_row_dpp: null argument");
  return launch("launch k_test_row_dpp", k_test_row_dpp, 1, 64, 0, static_cast<hipStream_t>(stream), acc, x, out);
}

#ifdef ANM_PHASE_TIMING
// tuning builds only: copy the per-wave phase timestamps of the last launches to the host
__attribute__((visibility("default"))) int anm_debug_phase_times(unsigned long long* out, int n_waves) {
  std::vector<unsigned long long> tmp(size_t(ANM_N_PHASES) * ANM_MAX_WAVES);
  if (hipMemcpyFromSymbol(tmp.data(), HIP_SYMBOL(g_anm_phase), tmp.size() * 8) != hipSuccess) return -1;
  for (int k = 0; k < ANM_N_PHASES; ++k)
    for (int w = 0; w < n_waves && w < ANM_MAX_WAVES; ++w) out[k * n_waves + w] = tmp[size_t(k) * ANM_MAX_WAVES + w];
  return 0;
}
#endif

}  // extern "C"
