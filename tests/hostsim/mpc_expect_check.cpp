// mpc_expect_check.cpp -- a stand-alone program (tests/test_mpc_expect_spec.py): the expected forecast of the MPC kernel,
// mpc::act_expect_value over mpc::chain_sweep (gym_anm_amd/csrc/anm_mpc.hpp, Act mode ANM_MPC_FORECAST_EXPECT), compiled for
// the host and run the way k_mpc runs it: a wavefront of 64 lanes, one host thread each, groups of G = 2^k >= N lanes, one
// environment per group, lane = stage -- idle lanes (stage >= N, environment >= E) and neighbouring groups included.  The
// bit patterns it prints are compared with gym_anm_amd/rng.py (exo_forecast_expected).  Built once per topology header
// (-DANM_TOPO_HEADER=...): a generated topology, and an MPC size class (is_padded).
//
// stdin (whitespace separated; floating-point values as the decimal value of their 64 bit patterns):
//   kind E N nl ng period base          kind 0: uniform mode; 1: series-noise mode without noise states; 2: with them
//   E x aux
//   low[n]  high[n]  rho[n]  z[E n]  series[n period]  noise[n period]        (n = nl + ng; all read, whatever the kind)
// stdout: one line per (environment, stage, unit), the value's bit pattern in hex.
#include <pthread.h>

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include ANM_TOPO_HEADER
#include "../../gym_anm_amd/csrc/anm_mpc.hpp"

using namespace anm;

// the part of mpc::WaveGroup the sweep uses: up() is the value of the lane before this one in the WAVEFRONT (row_shr:1 /
// wave_shr:1), 0 at stage 0 -- every lane of the wavefront takes part in every exchange
struct HostWave {
  double slot[64];
  pthread_barrier_t bar;
  HostWave() { pthread_barrier_init(&bar, nullptr, 64); }
  ~HostWave() { pthread_barrier_destroy(&bar); }
};
struct HostLane {
  HostWave* w;
  int lane, st;
  int stage() const { return st; }
  double up(double v) const {
    w->slot[lane] = v;
    pthread_barrier_wait(&w->bar);
    const double r = (st == 0 || lane == 0) ? 0.0 : w->slot[lane - 1];
    pthread_barrier_wait(&w->bar);
    return r;
  }
};

static bool read_u64(uint64_t& v) { return std::scanf("%" SCNu64, &v) == 1; }
static bool read_f64(double& d) {
  uint64_t v;
  if (!read_u64(v)) return false;
  std::memcpy(&d, &v, sizeof d);
  return true;
}
static bool read_all(std::vector<double>& a) {
  for (double& d : a)
    if (!read_f64(d)) return false;
  return true;
}

int main() {
  uint64_t kind, E, N, nl, ng, period;
  double base;
  if (!(read_u64(kind) && read_u64(E) && read_u64(N) && read_u64(nl) && read_u64(ng) && read_u64(period) && read_f64(base))) return 2;
  constexpr bool PAD = mpc::is_padded<Topo>::value;
  if (nl > uint64_t(Topo::NLOAD) || ng > uint64_t(Topo::NGEN) || (!PAD && (nl != uint64_t(Topo::NLOAD) || ng != uint64_t(Topo::NGEN)))) return 3;
  if (kind > 2 || E == 0 || E > 4096 || N == 0 || N > 64 || period == 0 || period > 4096) return 3;
  const int n = int(nl + ng), state_dim = 2 * Topo::ND + Topo::NDES + Topo::NGEN + 1;
  std::vector<double> state(E * state_dim, 0.0);
  for (uint64_t e = 0; e < E; ++e) {
    uint64_t a;
    if (!read_u64(a)) return 2;
    state[e * state_dim + state_dim - 1] = double(a);
  }
  std::vector<double> low(n), high(n), rho(n), z(E * n), series(size_t(n) * period), noise(size_t(n) * period);
  if (!(read_all(low) && read_all(high) && read_all(rho) && read_all(z) && read_all(series) && read_all(noise))) return 2;

  // what the mode does not read stays null: a dereference of it is a fault here, and an error under the sanitizers
  mpc::Act a{};
  a.mode = ANM_MPC_FORECAST_EXPECT;
  a.base = base;
  a.exo_mode = kind == 0 ? ANM_EXO_UNIFORM : ANM_EXO_SERIES_NOISE;
  a.exo_low = low.data();
  a.exo_high = high.data();
  if (kind >= 1) {
    a.state = state.data();
    a.state_dim = state_dim;
    a.series = series.data();
    a.period = int(period);
    a.exo_noise = noise.data();
  }
  if (kind == 2) {
    a.exo_rho = rho.data();
    a.exo_z = z.data();
  }

  int G = 1;
  while (G < int(N)) G *= 2;
  const int per_wave = 64 / G;
  const int64_t waves = (int64_t(E) + per_wave - 1) / per_wave;
  std::vector<double> out(E * N * n, 0.0);
  HostWave wave;
  std::vector<std::thread> th;
  for (int lane = 0; lane < 64; ++lane)
    th.emplace_back([&, lane]() {
      const HostLane x{&wave, lane, lane % G};
      for (int64_t b = 0; b < waves; ++b) {     // (k_mpc: env = block * (64 / G) + lane / G, on = env < n_envs && stage < N)
        const int64_t env = b * per_wave + lane / G;
        const bool on = env < int64_t(E) && x.st < int(N);
        const int aux = (on && a.exo_mode == ANM_EXO_SERIES_NOISE) ? mpc::act_table_at(a, env, x.st) : 0;   // (as solve<T, 3> does)
        for (int u = 0; u < n; ++u) {
          const double v = mpc::act_expect_value(a, aux, on, env, u, n, int(N), x);
          if (on) out[(env * N + x.st) * n + u] = v;
        }
      }
    });
  for (auto& t : th) t.join();
  for (double v : out) {
    uint64_t bits;
    std::memcpy(&bits, &v, sizeof bits);
    std::printf("%016" PRIx64 "\n", bits);
  }
  return 0;
}
