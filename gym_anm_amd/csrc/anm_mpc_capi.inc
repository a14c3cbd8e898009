// anm_mpc_capi.inc -- the MPC part of the C ABI (include/anm_mi355x.h: anm_mpc_*), shared by the per-topology library
// (anm_capi.hip) and by the MPC-only library (anm_mpc_only.hip: networks whose step runs on the table-driven lane-group
// kernels of some other library still need the MPC kernel compiled for THEIR topology).  Included inside extern "C";
// expects Topo, fail(), fail_hip(), g_err and struct anm_mpc (anm_mpc_capi_types.inc) in scope.
typedef mpc::NoTheta<Topo> TopoNoTheta;

extern "C++" template <class TT>
bool mpc_lds_attribute() {   // above the default per-workgroup limit: ask for the compute unit's whole LDS (once, at creation)
  if (mpc::Sz<TT>::LDS_BYTES <= 64 * 1024) return true;
  return hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 0, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 0, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 1, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
         hipFuncSetAttribute((const void*)mpc::k_mpc<TT, 2, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
}

// one group of G lanes per environment: one thread (N = 1), a part of a DPP row (N <= 16), half or all of a wavefront
// STREAM 1: the instantiations whose lanes draw the forecasts from the tasks' stream (anm_mpc_act_stream_f64); 2: ... and
// roll the correlated task's noise states forward from exo_z (anm_mpc_act_chain_f64); 3: the expected forecast, the noise
// states rolled forward without draws (anm_mpc_act_expect_f64)
extern "C++" template <class TT, int STREAM = 0>
void launch_mpc(unsigned grid, hipStream_t s, anm_mpc* m, const mpc::IO& io, const mpc::Opts& o, int64_t num_envs, int G) {
  const size_t lds_bytes = mpc::Sz<TT>::LDS_BYTES;
  if (G == 1)
    hipLaunchKernelGGL((mpc::k_mpc<TT, 0, STREAM>), dim3(grid), dim3(64), lds_bytes, s, (cptr_t)m->d_tab, io, o, num_envs, m->N, G);
  else if (G <= 16)
    hipLaunchKernelGGL((mpc::k_mpc<TT, 1, STREAM>), dim3(grid), dim3(64), lds_bytes, s, (cptr_t)m->d_tab, io, o, num_envs, m->N, G);
  else
    hipLaunchKernelGGL((mpc::k_mpc<TT, 2, STREAM>), dim3(grid), dim3(64), lds_bytes, s, (cptr_t)m->d_tab, io, o, num_envs, m->N, G);
}

int anm_mpc_create(const anm_network_desc* desc, double gamma, double safety_margin, int32_t planning_steps, anm_mpc** out) {
  if (!desc || !out) return fail("anm_mpc_create: null argument");
  constexpr bool FITS_FULL = mpc::Sz<Topo>::FITS, FITS_RELAXED = mpc::Sz<TopoNoTheta>::FITS;
  if constexpr (!FITS_RELAXED) {
    return fail("anm_mpc_create: this network has too many rows per stage for the register-resident MPC kernel");
  } else {
    std::string err;
    if constexpr (!mpc::is_padded<Topo>::value) {   // (a size class takes whatever fits: build_tables checks the counts)
      if (!check_topology<Topo>(*desc, err)) { g_err = err; return -3; }
    } else {
      // a size class has no compiled topology to compare with: the description itself must be sound before the tables
      // are built from it (indices in range, exactly one slack device, on bus 0)
      if (desc->n_bus < 2 || desc->n_dev < 1 || desc->n_branch < 1) return fail("anm_mpc_create: empty network description");
      int n_slack = 0;
      for (int b = 0; b < desc->n_branch; ++b)
        if (desc->br_from[b] < 0 || desc->br_from[b] >= desc->n_bus || desc->br_to[b] < 0 || desc->br_to[b] >= desc->n_bus ||
            desc->br_from[b] == desc->br_to[b])
          return fail("anm_mpc_create: a branch joins buses outside the network (or a bus with itself)");
      for (int k = 0; k < desc->n_dev; ++k) {
        const int ty = desc->dev_type[k];
        if (desc->dev_bus[k] < 0 || desc->dev_bus[k] >= desc->n_bus) return fail("anm_mpc_create: a device sits on a bus outside the network");
        if (ty != DEV_LOAD && ty != DEV_SLACK && ty != DEV_CLASSICAL && ty != DEV_RENEWABLE && ty != DEV_STORAGE)
          return fail("anm_mpc_create: unknown device type");
        if (ty == DEV_SLACK) { ++n_slack; if (desc->dev_bus[k] != 0) return fail("anm_mpc_create: the slack device must sit on bus 0"); }
      }
      if (n_slack != 1) return fail("anm_mpc_create: the network needs exactly one slack device");
    }
    anm_mpc* m = new (std::nothrow) anm_mpc();
    if (!m) return fail("out of host memory");
    for (int k = 0; k < desc->n_dev; ++k) {
      const int ty = desc->dev_type[k];
      if (ty == DEV_LOAD) { if (m->nl < 32) m->load_col[m->nl] = short(k); m->nl++; }
      m->ng += ty == DEV_CLASSICAL || ty == DEV_RENEWABLE;
      m->ns += ty == DEV_STORAGE;
    }
    m->nd = desc->n_dev;
    m->nbr = desc->n_branch;
    if (!mpc::build_tables<Topo>(*desc, gamma, safety_margin, planning_steps, m->tab, err, &m->theta_bound)) {
      delete m;
      g_err = err;
      return -3;
    }
    m->N = planning_steps;
    m->base_mva = desc->base_mva;
    // the angle rows ride along only where an angle could come near pi while the devices stay inside their limits
    m->angle_rows = m->theta_bound >= 0.98 * 3.14159265358979323846;
    if (m->angle_rows && !FITS_FULL) {
      delete m;
      return fail("anm_mpc_create: this network needs its angle rows (an angle can reach pi within the device limits) and has too "
                  "many rows per stage with them for the register-resident MPC kernel");
    }
    bool ok = mpc_lds_attribute<TopoNoTheta>();
    if constexpr (FITS_FULL) ok = ok && mpc_lds_attribute<Topo>();
    if (!ok) {
      delete m;
      return fail("anm_mpc_create: LDS size attribute");
    }
    hipError_t e = hipMalloc(&m->d_tab, m->tab.size() * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(m->d_tab, m->tab.data(), m->tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      anm_mpc_destroy(m);
      return fail_hip(e, "anm_mpc_create: device tables");
    }
    *out = m;
    return 0;
  }
}

void anm_mpc_destroy(anm_mpc* m) {
  if (!m) return;
  if (m->d_tab) hipFree(m->d_tab);
  delete m;
}

int anm_mpc_dims_of(const anm_mpc* m, anm_mpc_dims* o) {
  if (!m || !o) return fail("anm_mpc_dims_of: null argument");
  typedef mpc::Sz<Topo> S;
  // the network's own counts (they size the caller's arrays); rows / variables per stage and the table are the kernel's
  // (a size class: with its padding)
  o->planning_steps = m->N; o->n_load = m->nl; o->n_gen = m->ng; o->n_des = m->ns; o->n_branch = m->nbr;
  o->n_ctrl = m->ng + m->ns; o->n_stage_vars = S::NV; o->table_doubles = S::T_TOTAL;
  o->n_stage_rows = m->angle_rows ? S::NR : mpc::Sz<TopoNoTheta>::NR;
  o->angle_rows = m->angle_rows ? 1 : 0;
  o->angle_bound = m->theta_bound;
  return 0;
}

int anm_mpc_get_tables(const anm_mpc* m, double* out) {
  if (!m || !out) return fail("anm_mpc_get_tables: null argument");
  std::memcpy(out, m->tab.data(), m->tab.size() * sizeof(double));
  return 0;
}

static int mpc_launch(anm_mpc* m, int64_t num_envs, mpc::IO io, const anm_mpc_opts* opts, void* stream, const char* who) {
  const bool drawn = io.act.mode == ANM_MPC_FORECAST_STREAM, chain = io.act.mode == ANM_MPC_FORECAST_CHAIN,
             expect = io.act.mode == ANM_MPC_FORECAST_EXPECT;
  typedef mpc::Sz<Topo> S;
  mpc::Opts o{1e-11, 40};
  if (opts) {
    if (opts->tol > 0.0) o.tol = opts->tol;
    if (opts->max_iter > 0) o.max_iter = opts->max_iter;
    io.trace = opts->trace;
  }
  io.nl = m->nl;
  io.ng = m->ng;
  bool full = m->angle_rows;
  if (opts && opts->angle_rows == 1) full = true;
  if (opts && opts->angle_rows == 2) full = false;
  int G = 1;
  while (G < m->N) G *= 2;
  const int per_wave = 64 / G;
  const unsigned grid = unsigned((num_envs + per_wave - 1) / per_wave);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (full) {
    if constexpr (S::FITS) {
      if (expect) launch_mpc<Topo, 3>(grid, s, m, io, o, num_envs, G);
      else if (chain) launch_mpc<Topo, 2>(grid, s, m, io, o, num_envs, G);
      else if (drawn) launch_mpc<Topo, 1>(grid, s, m, io, o, num_envs, G);
      else launch_mpc<Topo>(grid, s, m, io, o, num_envs, G);
    } else { g_err = std::string(who) + ": with its angle rows this network has too many rows per stage for the MPC kernel"; return -1; }
  } else if (expect) {
    launch_mpc<TopoNoTheta, 3>(grid, s, m, io, o, num_envs, G);
  } else if (chain) {
    launch_mpc<TopoNoTheta, 2>(grid, s, m, io, o, num_envs, G);
  } else if (drawn) {
    launch_mpc<TopoNoTheta, 1>(grid, s, m, io, o, num_envs, G);
  } else {
    launch_mpc<TopoNoTheta>(grid, s, m, io, o, num_envs, G);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "launch k_mpc");
  return 0;
}

int anm_mpc_solve_f64(anm_mpc* m, int64_t num_envs, const double* p_load_forecast, const double* p_gen_forecast,
                      const double* soc, double* u0, double* objective, int32_t* iters, double* info, double* solution,
                      const anm_mpc_opts* opts, void* stream) {
  typedef mpc::Sz<Topo> S;
  if (!m || (m->ng + m->ns > 0 && !u0) || !objective || !iters) return fail("anm_mpc_solve_f64: null argument");
  if ((m->nl > 0 && !p_load_forecast) || (m->ng > 0 && !p_gen_forecast) || (S::NS > 0 && !soc))
    return fail("anm_mpc_solve_f64: a forecast / state-of-charge array is missing");
  if (num_envs <= 0) return 0;
  mpc::IO io{p_load_forecast, p_gen_forecast, soc, u0, objective, iters, info, solution, nullptr, mpc::Act{}, 0, 0};
  return mpc_launch(m, num_envs, io, opts, stream, "anm_mpc_solve_f64");
}

// what anm_mpc_act_f64, anm_mpc_act_stream_f64, anm_mpc_act_chain_f64 and anm_mpc_act_expect_f64 share: the checks of the
// common arguments, the Act, the launch.  `chain`: the three device arrays of the correlated task (with `exo` its stream
// part), or null; `expect`: the arrays of the expected forecast (then `exo` and `chain` are null), or null
static int mpc_act(anm_mpc* m, int64_t num_envs, int32_t forecast, const double* state, const double* state_alt,
                   const uint8_t* state_same, int32_t state_dim, const int32_t* aux_index, const double* series,
                   int32_t period, const double* soc, const double* act_low, const double* act_high, double* action,
                   double* u0, double* objective, int32_t* iters, double* info, const anm_mpc_opts* opts,
                   const anm_mpc_stream* exo, const anm_mpc_chain* chain, const anm_mpc_expect* expect, void* stream,
                   const char* who) {
  typedef mpc::Sz<Topo> S;
  const std::string w(who);
  if (!m || !state || !action || !act_low || !act_high || (m->ng + m->ns > 0 && !u0) || !objective || !iters)
    return fail((w + ": null argument").c_str());
  if (S::NS > 0 && !soc) return fail((w + ": the state-of-charge array is missing").c_str());
  if (state_same && !state_alt) return fail((w + ": state_same given without the rows to read instead").c_str());
  const int sdim = 2 * m->nd + m->ns + m->ng;
  if (state_dim < sdim) return fail((w + ": state_dim is smaller than the state vector").c_str());
  const bool table = forecast == ANM_MPC_FORECAST_PERFECT || (exo && exo->exo_mode == ANM_EXO_SERIES_NOISE) ||
                     (expect && expect->exo_mode == ANM_EXO_SERIES_NOISE);
  if (forecast == ANM_MPC_FORECAST_PERFECT && (!series || period <= 0))
    return fail((w + ": a perfect forecast needs the task's periodic tables").c_str());
  if (exo) {
    if (exo->exo_mode != ANM_EXO_UNIFORM && exo->exo_mode != ANM_EXO_SERIES_NOISE)
      return fail((w + ": exo_mode must be ANM_EXO_UNIFORM or ANM_EXO_SERIES_NOISE (the modes drawn inside the step kernels)").c_str());
    if (!exo->timestep || !exo->reset_count) return fail((w + ": the stream forecast needs timestep and reset_count").c_str());
    if (!exo->exo_low || !exo->exo_high) return fail((w + ": the stream forecast needs exo_low and exo_high (device arrays)").c_str());
    if (table && (!series || period <= 0 || !exo->exo_noise))
      return fail((w + ": the series-noise mode needs the task's table (series, period) and its amplitudes (exo_noise)").c_str());
  }
  if (chain && (!chain->exo_rho || !chain->exo_innov || !chain->exo_z))
    return fail((w + ": the chain forecast needs exo_rho, exo_innov and exo_z (device arrays)").c_str());
  if (expect) {
    if (expect->exo_mode != ANM_EXO_UNIFORM && expect->exo_mode != ANM_EXO_SERIES_NOISE)
      return fail((w + ": exo_mode must be ANM_EXO_UNIFORM or ANM_EXO_SERIES_NOISE (the modes drawn inside the step kernels)").c_str());
    if (!expect->exo_low || !expect->exo_high) return fail((w + ": the expected forecast needs exo_low and exo_high (device arrays)").c_str());
    if (table && (!series || period <= 0 || !expect->exo_noise))
      return fail((w + ": the series-noise mode needs the task's table (series, period) and its amplitudes (exo_noise)").c_str());
    if (!expect->exo_rho != !expect->exo_z)
      return fail((w + ": exo_rho and exo_z go together (both device arrays: correlated noise; both null: none)").c_str());
    if (!table && expect->exo_rho) return fail((w + ": the uniform mode has no noise states (exo_rho and exo_z must be null)").c_str());
  }
  if (table && !aux_index && state_dim < sdim + 1)
    return fail((w + ((exo || expect) ? ": the series-noise mode" : ": a perfect forecast") + " needs the time index (aux_index, or the last column of the state)").c_str());
  if (num_envs <= 0) return 0;
  mpc::Act a{forecast, state, state_alt, state_same, state_dim, aux_index, series, period, m->base_mva, action, act_low, act_high, {0}, 0};
  for (int l = 0; l < m->nl && l < 32; ++l) a.load_col[l] = m->load_col[l];
  a.gen_col0 = 2 * m->nd + m->ns;
  if (exo) {
    a.exo_mode = exo->exo_mode;
    a.seed = exo->rng_seed;
    a.env_offset = exo->env_offset;
    a.timestep = exo->timestep;
    a.reset_count = exo->reset_count;
    a.exo_low = exo->exo_low;
    a.exo_high = exo->exo_high;
    a.exo_noise = exo->exo_noise;
  }
  if (chain) {
    a.exo_rho = chain->exo_rho;
    a.exo_innov = chain->exo_innov;
    a.exo_z = chain->exo_z;
  }
  if (expect) {
    a.exo_mode = expect->exo_mode;
    a.exo_low = expect->exo_low;
    a.exo_high = expect->exo_high;
    a.exo_noise = expect->exo_noise;
    a.exo_rho = expect->exo_rho;
    a.exo_z = expect->exo_z;
  }
  mpc::IO io{nullptr, nullptr, soc, u0, objective, iters, info, nullptr, nullptr, a, 0, 0};
  return mpc_launch(m, num_envs, io, opts, stream, who);
}

int anm_mpc_act_f64(anm_mpc* m, int64_t num_envs, int32_t forecast, const double* state, const double* state_alt,
                    const uint8_t* state_same, int32_t state_dim, const int32_t* aux_index, const double* series,
                    int32_t period, const double* soc, const double* act_low, const double* act_high, double* action,
                    double* u0, double* objective, int32_t* iters, double* info, const anm_mpc_opts* opts, void* stream) {
  if (forecast != ANM_MPC_FORECAST_CONSTANT && forecast != ANM_MPC_FORECAST_PERFECT) return fail("anm_mpc_act_f64: unknown forecast");
  return mpc_act(m, num_envs, forecast, state, state_alt, state_same, state_dim, aux_index, series, period, soc, act_low, act_high,
                 action, u0, objective, iters, info, opts, nullptr, nullptr, nullptr, stream, "anm_mpc_act_f64");
}

int anm_mpc_act_stream_f64(anm_mpc* m, int64_t num_envs, const double* state, const double* state_alt,
                           const uint8_t* state_same, int32_t state_dim, const int32_t* aux_index, const double* series,
                           int32_t period, const double* soc, const double* act_low, const double* act_high, double* action,
                           double* u0, double* objective, int32_t* iters, double* info, const anm_mpc_opts* opts,
                           const anm_mpc_stream* exo, void* stream) {
  if (!exo) return fail("anm_mpc_act_stream_f64: null argument (anm_mpc_stream)");
  return mpc_act(m, num_envs, ANM_MPC_FORECAST_STREAM, state, state_alt, state_same, state_dim, aux_index, series, period, soc,
                 act_low, act_high, action, u0, objective, iters, info, opts, exo, nullptr, nullptr, stream,
                 "anm_mpc_act_stream_f64");
}

int anm_mpc_act_chain_f64(anm_mpc* m, int64_t num_envs, const double* state, const double* state_alt,
                          const uint8_t* state_same, int32_t state_dim, const int32_t* aux_index, const double* series,
                          int32_t period, const double* soc, const double* act_low, const double* act_high, double* action,
                          double* u0, double* objective, int32_t* iters, double* info, const anm_mpc_opts* opts,
                          const anm_mpc_chain* exo, void* stream) {
  if (!exo) return fail("anm_mpc_act_chain_f64: null argument (anm_mpc_chain)");
  if (exo->exo.exo_mode != ANM_EXO_SERIES_NOISE)
    return fail("anm_mpc_act_chain_f64: exo_mode must be ANM_EXO_SERIES_NOISE (the mode that has correlated noise)");
  return mpc_act(m, num_envs, ANM_MPC_FORECAST_CHAIN, state, state_alt, state_same, state_dim, aux_index, series, period, soc,
                 act_low, act_high, action, u0, objective, iters, info, opts, &exo->exo, exo, nullptr, stream,
                 "anm_mpc_act_chain_f64");
}

int anm_mpc_act_expect_f64(anm_mpc* m, int64_t num_envs, const double* state, const double* state_alt,
                           const uint8_t* state_same, int32_t state_dim, const int32_t* aux_index, const double* series,
                           int32_t period, const double* soc, const double* act_low, const double* act_high, double* action,
                           double* u0, double* objective, int32_t* iters, double* info, const anm_mpc_opts* opts,
                           const anm_mpc_expect* exo, void* stream) {
  if (!exo) return fail("anm_mpc_act_expect_f64: null argument (anm_mpc_expect)");
  return mpc_act(m, num_envs, ANM_MPC_FORECAST_EXPECT, state, state_alt, state_same, state_dim, aux_index, series, period, soc,
                 act_low, act_high, action, u0, objective, iters, info, opts, nullptr, nullptr, exo, stream,
                 "anm_mpc_act_expect_f64");
}
