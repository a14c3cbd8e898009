// anm_lane_io.inc -- what a lane-group kernel does for the ENVIRONMENT around its Newton solve, as program text that
// radial::k_radial (anm_radial.hpp) and mesh::k_mesh (anm_mesh.hpp) include into their bodies: a device lane's inputs for
// transition, reset or step, and the stores of state, observation, reward, flags, counters and episode statistics after
// the solve.  The semantics are the bit-exact specifications of rng.py, episode.py and io_dtype.py; they are stated here
// once.  Text and not function templates, because k_mesh's schedule does not survive them: through functions with these
// bodies it computed the same bits from no more registers and ran 0.7 ... 2.5 % slower in every form tried (DESIGN 3.7);
// included, both kernels compile to the machine code they had with the text written out.
//
//   #define ANM_LANE_IO_PART n
//   #include "anm_lane_io.inc"
//
// Names the including kernel has in scope (all parts): d (its Dims), io, mode, K = io.e.K, typ / slot / sset (the device
// lane l plays), l, G, C (the constants of the environment's parameter class), rd, base, the row strides W_LOAD, W_GEN,
// W_SET, W_DES, W_ACT, W_ST, W_EXO, W_AUX (the network's widths or those of a bound view).
//   1  inputs: ee (the environment index, valid for an idle lane too) and env_ok (the lane's slot is inside the batch: ee
//      is its OWN environment).  Declares skip, resetting, sampled, aux, in_p, in_q, in_pot, soc, s0_q, soc_req.  Stores the
//      noise states of the correlated series-noise mode (io.e.exo_z), the one output that is read, advanced and written
//      at the draw site, under env_ok.
//   2  the stores of mode 0; inside the kernel's do { } while (false), which it leaves with `dump` set.  Needs e, reward,
//      e_loss, penalty, converged, it, nr_diff, fdiff, dump.
//   3  declares state, list, ON, OW and the sinks put_obs / put_reward / put; inside a generic lambda whose
//      `constexpr bool f32` chooses float32 or float64 obs rows and reward (EnvIO::io32, a wave-uniform flag; the float64
//      values rounded once as they are stored: ONE branch chooses between the two instantiations, nothing of it is inside
//      the Newton trips, and the float64 path is the code it was without the mode).  MAP, the kernel's template flag: the
//      affine I/O map (EnvIO::iomap, never null there; io_affine.py) -- ONE instance of the output section, which maps what
//      it stores and takes the number format at run time.  A kernel instantiation of its own, not a third arm: with the arm
//      in it, k_radial<double, Topo> took 169 VGPRs instead of 168 -- two wavefronts per SIMD instead of three -- for every
//      task (profiles/io_map_kernels.txt); the plain instantiations are the code they were.
//   4  the skeleton of modes 1 and 2, after part 3 and inside a do { } while (false).  Needs dev_p, dev_q, p_pot and what
//      part 2 needs; writes `soc` on a reset (the requested one, which the kernel's dump and list observation then show)
//      and sets `dump`.  ANM_LIST_OBS_DUE(zero) is the kernel's: a list observation is due -- zeros (terminal / absorbing:
//      anm_env.py:365-367, 442-446) or gathered from the electrical state -- on a path all lanes of the environment take
//      together (every condition around it is uniform over the lane group).  k_radial writes it on the spot, k_mesh notes
//      it and writes it at its single site (DESIGN 3.6, 3.7).  Sets fc_due / fc_at (the kernel's: `bool fc_due = false; int
//      fc_at = 0;` beside `dump`) wherever it writes the state row.
//   5  after the dump, outside every do { } while: the expected forecast of the lane's unit (io.e.forecast) where part 4
//      said it is due.
#if ANM_LANE_IO_PART == 1   // ---- inputs per device lane
  bool skip = false;        // env in the absorbing terminal state (step mode, no autoreset), or masked out of a reset
  bool resetting = false;
  bool sampled = false;     // initial state drawn by the in-kernel RNG (autoreset, or reset without init_state)
  int aux = 0;
  double in_p = 0.0, in_q = 0.0, in_pot = 0.0, soc = 0.0, s0_q = 0.0;
  double soc_req = 0.0;     // reset: requested SoC (MWh slot)
  if (mode == 0) {
    if (typ == DEV_LOAD) in_p = io.t.p_load[ee * W_LOAD + slot];
    else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) {
      in_pot = io.t.p_pot[ee * W_GEN + slot];
      in_p = io.t.p_set[ee * W_SET + sset];
      in_q = io.t.q_set[ee * W_SET + sset];
    } else if (typ == DEV_STORAGE) {
      in_p = io.t.p_set[ee * W_SET + sset];
      in_q = io.t.q_set[ee * W_SET + sset];
      soc = io.t.soc[ee * W_DES + slot];
    }
  } else {
    bool was_term = (mode == 2) && io.e.terminated[ee] != 0;
    // episode time limit (io.e.ep, wave-uniform): with autoreset an environment past it is re-initialised like a terminated one
    if (mode == 2 && io.e.ep.on && io.e.autoreset) was_term = was_term || episode_timed_out(io.e.ep, io.e.timestep[ee]);
    const bool series = io.e.exo == nullptr;
    resetting = (mode == 1) || (was_term && io.e.autoreset && series);
    skip = (mode == 2) && was_term && !resetting;
    if (mode == 1 && io.e.mask && !io.e.mask[ee]) skip = true;
    double s0_p = 0.0, s0_pm = 0.0;
    sampled = resetting && !(mode == 1 && io.e.init_state);
    // uniform exogenous mode (io.e.exo_mode, wave-uniform): every load / generator lane draws its own unit from the step
    // stream of its environment's episode -- the episode key plus one block (ExoUniform, anm_device.hpp)
    // noisy time series (the third value of io.e.exo_mode): the table index moves as in series mode, the draws are keyed by
    // the step index of the episode (io.e.timestep) and shaped by the two table entries at the NEW index (ExoNoise)
    const bool uni = io.e.exo_mode == 1;
    const bool noisy = io.e.exo_mode == 2;
    const bool exo_unit = typ == DEV_LOAD || typ == DEV_CLASSICAL || typ == DEV_RENEWABLE;
    // (one site draws for both modes -- the Philox blocks are the bulk of the code -- and the mode only chooses the map;
    // `at`: the table index of the noisy series)
    // correlated noise (io.e.exo_z bound, wave-uniform; rng.py: exo_series_corr): the factor drives the unit's noise state
    // and the state is mapped.  `first`: step index 0 of an episode, z = w.  `keep`: rows the caller brings -- only the
    // state is stored.  The read-modify-write is the lane's own unit of its OWN environment: an idle lane (ee clamped to
    // a valid index) touches nothing, or that environment would be advanced twice; nor does a lane masked out of a reset.
    const bool corr = noisy && io.e.exo_z != nullptr;
    const bool own = env_ok && !skip;
    auto exo_draw = [&](uint32_t epoch, uint32_t step, int at, bool first, bool keep = false) {
      const int unit = typ == DEV_LOAD ? slot : d.NLOAD + slot;
      const uint64_t key = ExoUniform::episode_key(io.e.rng_seed, io.e.env_offset + uint64_t(ee), epoch);
      uint32_t q[4];
      ExoUniform::block(key, step, uint32_t(unit) >> 1, q);
      if (noisy) {
        double v = ExoNoise::factor(q, unit);
        if (corr) {
          double* z = io.e.exo_z + ee * (d.NLOAD + d.NGEN) + unit;
          if (!first) v = ExoNoise::advance(io.e.exo_rho[unit], io.e.exo_innov[unit], own ? *z : 0.0, v);
          if (own) *z = v;
        }
        if (keep) return 0.0;
        return ExoNoise::map_state(io.e.exo_noise[unit * io.e.period + at], v, io.e.series[unit * io.e.period + at],
                                   io.e.exo_lo[unit], io.e.exo_hi[unit]);
      }
      return ExoUniform::map(io.e.exo_lo[unit], io.e.exo_hi[unit], Philox::u01_of(q, unit));
    };
    if (mode == 1 && io.e.init_state) {
      const double* s0 = io.e.init_state + ee * W_ST;
      if (typ != DEV_NONE) { s0_p = s0[l]; s0_q = s0[d.ND + l]; }
      if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) s0_pm = s0[2 * d.ND + d.NDES + slot];
      if (typ == DEV_STORAGE) soc_req = s0[2 * d.ND + slot];
      // (correlated noise: the noise state starts where a drawn episode's does, at the factors of step index 0 of the
      // epoch -- the reset count as it stands, which the caller advances afterwards)
      if (corr && exo_unit) exo_draw(uint32_t(io.e.reset_count[ee]), 0u, 0, true, true);
    } else if (resetting) {  // autoreset: ANM6Easy.init_state with the counter-based RNG
      const uint32_t epoch = uint32_t(io.e.reset_count[ee]);
      double drawn = 0.0;
      const bool have = uni || noisy;
      if (!uni) {   // (uniform mode: the aux variable is the step index, 0)
        uint32_t r[4];
        Philox::generate(io.e.rng_seed, io.e.env_offset + uint64_t(ee), epoch, 0u, r);
        aux = int((uint64_t(r[0]) * uint64_t(io.e.period)) >> 32);
      }
      // step index 0: loads and generator P / P_max from the step stream at index 0 (noisy series: at the drawn table index)
      if (have && exo_unit) drawn = exo_draw(epoch, 0u, aux, true);
      cptr_t sd = C + d.off_dev + l * SD_SIZE;
      if (typ == DEV_LOAD) s0_p = have ? drawn : io.e.series[slot * io.e.period + aux];
      else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) {
        const double uu = Philox::unit_u01(io.e.rng_seed, io.e.env_offset + uint64_t(ee), epoch, slot);
        s0_p = s0_pm = have ? drawn : io.e.series[(d.NLOAD + slot) * io.e.period + aux];
        s0_q = sd[SD_QMIN] + (sd[SD_QMAX] - sd[SD_QMIN]) * uu;
      } else if (typ == DEV_STORAGE) {
        const double uu = Philox::unit_u01(io.e.rng_seed, io.e.env_offset + uint64_t(ee), epoch, d.NGEN + slot);
        soc_req = sd[SD_SOC_MIN] + (sd[SD_SOC_MAX] - sd[SD_SOC_MIN]) * uu;
      }
    }
    if (resetting) {
      in_p = s0_p; in_q = s0_q; in_pot = s0_pm;
      if (typ == DEV_STORAGE) {
        cptr_t sd = C + d.off_dev + l * SD_SIZE;
        soc = (s0_p <= 0.0) ? sd[SD_SOC_MIN] : sd[SD_SOC_MAX];  // simulator.py:273-278
      }
    } else if (!skip) {
      const double* a = io.e.action + ee * W_ACT;
      if (uni || noisy) {   // the draws are keyed by the NEW step index of the episode and the episode's epoch
        const double av = io.e.state[ee * W_ST + d.SDIM];
        uint32_t step;
        if (uni) {          // the aux variable is that step index
          aux = int(av) + 1;
          step = uint32_t(aux);
        } else {            // the aux variable is the table index, as in series mode; the step index is timestep + 1
          aux = int(fmod(av + 1.0, double(io.e.period)));
          step = uint32_t(io.e.timestep[ee]) + 1u;
        }
        if (exo_unit) {
          const double x = exo_draw(uint32_t(io.e.reset_count[ee]) - 1u, step, aux, false);
          if (typ == DEV_LOAD) in_p = x;
          else in_pot = x;
        }
      } else if (series) {
        const double av = io.e.state[ee * W_ST + d.SDIM];
        aux = int(fmod(av + 1.0, double(io.e.period)));
        if (typ == DEV_LOAD) in_p = io.e.series[slot * io.e.period + aux];
        else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) in_pot = io.e.series[(d.NLOAD + slot) * io.e.period + aux];
      } else {
        if (typ == DEV_LOAD) in_p = io.e.exo[ee * W_EXO + slot];
        else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) in_pot = io.e.exo[ee * W_EXO + d.NLOAD + slot];
      }
      // (float32 I/O, EnvIO::io32: the action row holds floats, widened here; ONE wave-uniform branch, the float64 arm is
      // the code it was)
      if (io.e.io32) {
        const float* af = reinterpret_cast<const float*>(io.e.action) + ee * W_ACT;
        if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) { in_p = af[slot]; in_q = af[d.NGEN + slot]; }
        else if (typ == DEV_STORAGE) {
          in_p = af[2 * d.NGEN + slot];
          in_q = af[2 * d.NGEN + d.NDES + slot];
          soc = io.e.soc[ee * W_DES + slot];
        }
      } else if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) { in_p = a[slot]; in_q = a[d.NGEN + slot]; }
      else if (typ == DEV_STORAGE) {
        in_p = a[2 * d.NGEN + slot];
        in_q = a[2 * d.NGEN + d.NDES + slot];
        soc = io.e.soc[ee * W_DES + slot];
      }
      // (affine I/O map, the kernel's MAP instantiation: what was read is u, the set-points are a = clamp(fma(half, u, mid))
      // -- IoMap::action; behind the reads, which are the code they were)
      if constexpr (MAP) {
        const int A = 2 * (d.NGEN + d.NDES);
        if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) {
          in_p = IoMap::action(io.e.iomap, A, slot, in_p);
          in_q = IoMap::action(io.e.iomap, A, d.NGEN + slot, in_q);
        } else if (typ == DEV_STORAGE) {
          in_p = IoMap::action(io.e.iomap, A, 2 * d.NGEN + slot, in_p);
          in_q = IoMap::action(io.e.iomap, A, 2 * d.NGEN + d.NDES + slot, in_q);
        }
      }
    }
  }
#elif ANM_LANE_IO_PART == 2   // ---- mode 0: what Simulator.transition returns beside the dump
  if (mode == 0) {
    if (typ == DEV_STORAGE) io.t.soc[e * W_DES + slot] = soc;
    if (l == 0) {
      io.t.reward[e] = reward; io.t.e_loss[e] = e_loss; io.t.penalty[e] = penalty;
      io.t.converged[e] = converged ? 1 : 0;
      if (io.t.nr_iters) io.t.nr_iters[e] = it;
      if (nr_diff) nr_diff[e] = fdiff;
    }
    dump = true;
    break;
  }
#elif ANM_LANE_IO_PART == 3   // ---- modes 1 and 2: where environment e's state, observation and reward go
  double* state = io.e.state + e * W_ST;
  // the observation: clip(state, Box) next to the state row, or (a list is set: anm_env.py:497-521, 562-592)
  // n_obs entries gathered from this environment's electrical state
  const bool list = mode == 2 && io.e.n_obs > 0;
  const int ON = list ? io.e.n_obs : W_ST;                                  // entries of an observation row
  const int OW = list ? (io.v.w_obs > 0 ? io.v.w_obs : io.e.n_obs) : W_ST;   // its stride (a view pads the rows)
  double* obs = io.e.obs + e * OW;
  float* obs32 = reinterpret_cast<float*>(io.e.obs) + e * OW;
  auto put_obs = [&](int k, double v) {
    if constexpr (MAP) io_store(io.e.obs, e * OW + k, IoMap::observation(io.e.iomap, 2 * (d.NGEN + d.NDES), ON, k, v), io.e.io32 != 0);
    else if constexpr (f32) obs32[k] = float(v);
    else obs[k] = v;
  };
  auto put_reward = [&](double v) {
    if constexpr (MAP) io_store(io.e.reward, e, IoMap::reward(io.e.iomap, v), io.e.io32 != 0);
    else if constexpr (f32) reinterpret_cast<float*>(io.e.reward)[e] = float(v);
    else io.e.reward[e] = v;
  };
  cptr_t lo = C + d.off_obs_lo, hi = C + d.off_obs_hi;
  auto put = [&](int k, double v) {
    state[k] = v;
    if (!list) put_obs(k, fmin(fmax(v, lo[k]), hi[k]));
  };
#elif ANM_LANE_IO_PART == 4   // ---- modes 1 and 2: absorbing row, the reset branches, the regular step
  if (skip) {
    if (mode == 2) {  // absorbing terminal state
      if (list) ANM_LIST_OBS_DUE(true);
      else for (int k = l; k < d.SDIM + K; k += G) put_obs(k, 0.0);
      if (l == 0) { put_reward(0.0); if (io.e.nr_iters) io.e.nr_iters[e] = 0; }
    }
    break;
  }
  if (l == 0 && io.e.nr_iters) io.e.nr_iters[e] = it;
  if (resetting) {
    if (typ == DEV_STORAGE) {
      soc = soc_req / base;  // simulator.py:284-288
      io.e.soc[e * W_DES + slot] = soc;
    }
    if (mode == 2 && !converged) {
      // a redraw whose first power flow does not converge looks like the absorbing terminal state until the next call
      // draws again
      for (int k = l; k < d.SDIM + K; k += G) { state[k] = 0.0; if (!list) put_obs(k, 0.0); }
    } else {
      if (typ != DEV_NONE) { put(l, dev_p * base); put(d.ND + l, dev_q * base); }
      if (typ == DEV_STORAGE) put(2 * d.ND + slot, soc * base);
      if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) put(2 * d.ND + d.NDES + slot, p_pot * base);
    }
    if (mode == 1) {
      if (sampled) {
        if (l == 0) { put(d.SDIM, double(aux)); io.e.reset_count[e] += 1; }
      } else {
        const double* s0 = io.e.init_state + e * W_ST;
        for (int k = l; k < K; k += G) put(d.SDIM + k, s0[d.SDIM + k]);
      }
      if (l == 0) { io.e.converged[e] = converged ? 1 : 0; io.e.terminated[e] = 0; if (io.e.timestep) io.e.timestep[e] = 0; }
      if (l == 0 && io.e.ep.on) episode_clear(io.e.ep, e);
      if (l == 0 && nr_diff) nr_diff[e] = fdiff;
    } else {
      if (l == 0) {
        if (converged) put(d.SDIM, double(aux));
        io.e.reset_count[e] += 1;
        io.e.terminated[e] = converged ? 0 : 1;
        if (io.e.timestep) io.e.timestep[e] = 0;
        put_reward(0.0); io.e.e_loss[e] = 0.0; io.e.penalty[e] = 0.0;
        if (io.e.ep.on) episode_clear(io.e.ep, e);
      }
      ANM_LIST_OBS_DUE(!converged);
    }
    // (the forecast row is due, part 5, at the table index of the row: the caller's, the drawn one, or 0 where a redraw left
    // the zero row)
    fc_due = true;
    fc_at = mode == 1 ? (sampled ? aux : int(io.e.init_state[e * W_ST + d.SDIM])) : (converged ? aux : 0);
    dump = true;
    break;
  }
  // regular step
  if (typ == DEV_STORAGE) io.e.soc[e * W_DES + slot] = soc;
  const bool term = !converged;
  if (!term) {
    if (typ != DEV_NONE) { put(l, dev_p * base); put(d.ND + l, dev_q * base); }
    if (typ == DEV_STORAGE) put(2 * d.ND + slot, soc * base);
    if (typ == DEV_CLASSICAL || typ == DEV_RENEWABLE) put(2 * d.ND + d.NDES + slot, p_pot * base);
    if (io.e.exo == nullptr) {
      if (l == 0) put(d.SDIM, double(aux));
    } else {
      for (int k = l; k < K; k += G) put(d.SDIM + k, io.e.aux_next[e * W_AUX + k]);
    }
  } else {
    for (int k = l; k < d.SDIM + K; k += G) { state[k] = 0.0; if (!list) put_obs(k, 0.0); }
  }
  ANM_LIST_OBS_DUE(term);
  if (l == 0) {
    const double c1 = rd[SF_C1], c2 = rd[SF_C2];
    io.e.terminated[e] = term ? 1 : 0;
    double rwd;
    if (!term) {
      const double sg2 = (e_loss > 0.0) ? 1.0 : ((e_loss < 0.0) ? -1.0 : 0.0);
      const double elc = sg2 * fmin(fabs(e_loss), c1);
      const double pn = fmin(fmax(penalty, 0.0), c2);
      rwd = -(elc + pn);
      io.e.e_loss[e] = elc; io.e.penalty[e] = pn; put_reward(rwd);
    } else {
      rwd = rd[SF_RTERM];
      put_reward(rwd); io.e.e_loss[e] = c1; io.e.penalty[e] = c2;
    }
    if (io.e.ep.on) episode_step(io.e.ep, e, rwd, term, io.e.timestep[e] + 1);   // (before the increment below)
    if (io.e.timestep) io.e.timestep[e] += 1;
  }
  fc_due = true;
  fc_at = term ? 0 : aux;   // (a terminal step writes the zero row: table index 0, the noise state as stored)
  dump = true;
#elif ANM_LANE_IO_PART == 5   // ---- modes 1 and 2: the expected forecast, the kernel's last stores
  // (io.e.forecast bound, wave-uniform; rng.py: exo_forecast_expected)  The load or generator lane forms the H entries of its
  // own unit from the table index the state row got (fc_at) and the noise state it stored itself at the draw site, re-read
  // here.  The tables come from the block behind io.e.forecast, loaded HERE: nothing of the feature lives across the Newton
  // trips but that pointer, and the electrical state is dead by now.  fc_due is set by part 4 alone, which runs for the
  // lane's OWN environment (env_ok) on the paths that write the state row (not skip).
  if (fc_due && io.e.forecast && (typ == DEV_LOAD || typ == DEV_CLASSICAL || typ == DEV_RENEWABLE)) {
    const ExoForecastIO f = *io.e.forecast;
    const int unit = typ == DEV_LOAD ? slot : d.NLOAD + slot;
    const int64_t zi = e * (d.NLOAD + d.NGEN) + unit, fo = zi * f.H;
    const bool f32 = io.e.io32 != 0;
    ExoNoise::forecast_row(f.z ? f.rho[unit] : 0.0, f.z ? f.z[zi] : 0.0, f.noise + unit * f.period, f.series + unit * f.period, f.lo[unit],
                           f.hi[unit], fc_at, f.period, f.H, [&](int i, double v) { io_store(static_cast<double*>(f.out), fo + i, v, f32); });
  }
#else
#error "ANM_LANE_IO_PART: 1 ... 5"
#endif
#undef ANM_LANE_IO_PART
