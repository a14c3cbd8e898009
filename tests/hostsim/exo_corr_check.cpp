// exo_corr_check.cpp -- a stand-alone program (tests/test_exo_corr_spec.py): the correlated noise of the series-noise mode,
// ExoNoise::advance and ExoNoise::map_state (gym_anm_amd/csrc/anm_device.hpp, unchanged), compiled for the host and run over
// the episodes of a few keys; the bit patterns it prints are compared with gym_anm_amd/rng.py (exo_series_corr,
// series_corr_init_z).
//
// stdin (whitespace separated; floating-point values as the decimal value of their 64 bit patterns):
//   seed n_exo period steps E
//   E x (env epoch aux0)
//   rho[n_exo] innov[n_exo] low[n_exo] high[n_exo] series[n_exo period] noise[n_exo period]
// stdout, per episode: n_exo lines with the initial z, then per step and unit one line "z P" -- bit patterns in hex.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../gym_anm_amd/csrc/anm_device.hpp"

using namespace anm;

static bool read_u64(uint64_t& v) { return std::scanf("%" SCNu64, &v) == 1; }
static bool read_all(std::vector<double>& a) {
  for (double& d : a) {
    uint64_t v;
    if (!read_u64(v)) return false;
    std::memcpy(&d, &v, sizeof d);
  }
  return true;
}
static uint64_t bits(double d) {
  uint64_t v;
  std::memcpy(&v, &d, sizeof v);
  return v;
}

int main() {
  uint64_t seed, n, period, steps, E;
  if (!(read_u64(seed) && read_u64(n) && read_u64(period) && read_u64(steps) && read_u64(E))) return 2;
  if (n == 0 || n > 64 || period == 0 || period > 4096 || steps > 4096 || E == 0 || E > 64) return 3;
  std::vector<uint64_t> env(E), epoch(E), aux0(E);
  for (uint64_t e = 0; e < E; ++e)
    if (!(read_u64(env[e]) && read_u64(epoch[e]) && read_u64(aux0[e])) || aux0[e] >= period) return 2;
  std::vector<double> rho(n), innov(n), low(n), high(n), series(n * period), noise(n * period);
  if (!(read_all(rho) && read_all(innov) && read_all(low) && read_all(high) && read_all(series) && read_all(noise))) return 2;
  std::vector<double> z(n);
  for (uint64_t e = 0; e < E; ++e) {
    const uint64_t key = ExoUniform::episode_key(seed, env[e], uint32_t(epoch[e]));
    uint32_t q[4];
    for (uint64_t i = 0; i < n; ++i) {   // an episode starts at the factors of step index 0
      ExoUniform::block(key, 0u, uint32_t(i) >> 1, q);
      z[i] = ExoNoise::factor(q, int(i));
      std::printf("%016" PRIx64 "\n", bits(z[i]));
    }
    uint64_t aux = aux0[e];
    for (uint64_t t = 1; t <= steps; ++t) {
      aux = (aux + 1) % period;
      for (uint64_t i = 0; i < n; ++i) {
        ExoUniform::block(key, uint32_t(t), uint32_t(i) >> 1, q);
        z[i] = ExoNoise::advance(rho[i], innov[i], z[i], ExoNoise::factor(q, int(i)));
        const double P = ExoNoise::map_state(noise[i * period + aux], z[i], series[i * period + aux], low[i], high[i]);
        std::printf("%016" PRIx64 " %016" PRIx64 "\n", bits(z[i]), bits(P));
      }
    }
  }
  return 0;
}
