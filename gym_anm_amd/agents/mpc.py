"""Batched MPC DC-OPF policy: the reference's ``gym_anm/agents/mpc.py`` for ``num_envs`` environments at once.

The reference builds, per environment and per call of ``act()``, an N-stage DC optimal power flow with
cvxpy (``mpc.py:163-319``) and hands it to a generic convex solver.  The problem is a linear program whose
constraint MATRIX depends only on the network and the horizon; what changes from call to call and from
environment to environment are right-hand sides: the load / generation forecasts and the storage state
of charge (``mpc.py:390-417``).  So here

* :class:`BatchedDCOPF` solves all environments in ONE launch of the hand-written interior-point kernel
  (``csrc/anm_mpc.hpp``; the reduced, stage-structured form of the program is documented in ``dcopf.py``);
* :class:`MPCAgent` / :class:`MPCAgentConstant` / :class:`MPCAgentPerfect` keep the reference's names,
  constructor arguments and ``act(env)`` contract (``mpc.py:321-346``, ``mpc_constant.py``, ``mpc_perfect.py``)
  on a :class:`~gym_anm_amd.envs.anm_env.BatchedANMEnv`;
* :class:`MPCAgentPerfectStream` is the perfect-forecast agent of the tasks whose exogenous variables are drawn inside
  the step kernels (``exogenous="uniform"`` / ``"series_noise"``): its forecast is the tasks' own random stream,
  evaluated ahead; :class:`MPCAgentPerfectChain` is the same for the series-noise task with correlated noise
  (``exo_corr=``): the step's AR(1) recurrence rolled forward from the environment's noise states;
* :class:`MPCAgentExpected` is the informed baseline of those drawn tasks that does not know the future draws: the
  conditional mean of the noise given the task's current state, mapped like a draw;
* :class:`DCOPFProgram` spells the reference's program out row by row (``min q.x, l <= A x <= u``); nothing in
  the solve uses it -- it is what the tests check a solution's feasibility against.

All quantities are per-unit, as in the reference.  An LP optimum is not unique in general (curtailment vs
storage, charge vs discharge splits), so two exact solvers may return different optimal actions; what is
comparable is the optimal objective, the feasibility of the action, and the action itself where the minimiser
is unique (tests/test_mpc.py).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import errors as E_
from ..model import CLASSICAL, LOAD, RENEWABLE, SLACK, STORAGE

INF = np.inf


class DCOPFProgram:
    """The N-stage DC-OPF of ``mpc.py:163-319`` as  min q.x  s.t.  l0 + Lp p <= A x <= u0 + Up p.

    Variables per stage i (in this order): bus angles theta (n_bus), device injections P_dev (n_dev),
    storage charge p_c and discharge p_d (n_des each, both >= 0, ``mpc.py:282-291``) and one epigraph variable
    s per branch for ``max(0, |P_ij| - beta rate)`` (``mpc.py:308-311``).  Parameters p (per environment):
    load forecasts [n_load x N] (stage-major), generation forecasts [n_gen x N], initial SoC [n_des].
    """

    def __init__(self, model, gamma, safety_margin, planning_steps):
        m, N = model, int(planning_steps)
        self.N = N
        nb, nd, nbr = m.N_bus, m.N_device, m.N_branch
        loads, gens, des = list(m.load_idx), list(m.gen_idx), list(m.des_idx)
        nl, ng, ns = len(loads), len(gens), len(des)
        self.nl, self.ng, self.ns = nl, ng, ns
        B = np.asarray(m.Y_bus).imag  # mpc.py:113: B_bus = Im(Y_bus)
        per = nb + nd + 2 * ns + nbr
        self.per, self.n = per, per * N
        TH, PD, PC, PDIS, SB = 0, nb, nb + nd, nb + nd + ns, nb + nd + 2 * ns
        self.off = dict(theta=TH, p_dev=PD, p_c=PC, p_d=PDIS, s=SB)
        self.n_param = (nl + ng) * N + ns
        rows, lo, up, Lp, Up = [], [], [], [], []

        def add(coefs, l, u, lp=None, up_=None):
            r = np.zeros(self.n)
            for k, v in coefs:
                r[k] += v
            rows.append(r)
            lo.append(l)
            up.append(u)
            Lp.append(np.zeros(self.n_param) if lp is None else lp)
            Up.append(np.zeros(self.n_param) if up_ is None else up_)

        def pvec(idx, val=1.0):
            v = np.zeros(self.n_param)
            v[idx] = val
            return v

        q = np.zeros(self.n)
        dt = m.delta_t
        slack_theta = m.slack_dev  # mpc.py:302 indexes the ANGLES with the slack DEVICE's position (sic)
        for i in range(N):
            o = i * per
            # P_bus[i] = sum over the branches at i of B_ij (theta_i - theta_j)   (mpc.py:232-245)
            for b in range(nb):
                c = []
                for f, t in zip(m.br_f, m.br_t):
                    if f == b:
                        c += [(o + TH + f, B[f, t]), (o + TH + t, -B[f, t])]
                    elif t == b:
                        c += [(o + TH + t, B[t, f]), (o + TH + f, -B[t, f])]
                c += [(o + PD + k, -1.0) for k in range(nd) if m.dev_bus[k] == b]
                add(c, 0.0, 0.0)
            # loads follow their forecast (mpc.py:247-251)
            for j, k in enumerate(loads):
                pv = pvec(i * nl + j)
                add([(o + PD + k, 1.0)], 0.0, 0.0, pv, pv)
            # non-slack generators: P_min <= P <= min(P_max, forecast)  (mpc.py:253-258 and 267-271: two upper
            # bounds, kept as two rows)
            for j, k in enumerate(gens):
                add([(o + PD + k, 1.0)], m.dev_p_min[k], m.dev_p_max[k])
                add([(o + PD + k, 1.0)], -INF, 0.0, None, pvec(nl * N + i * ng + j))
            # storage: box, split into charge / discharge, SoC window (mpc.py:260-265, 273-291)
            for j, k in enumerate(des):
                add([(o + PD + k, 1.0)], m.dev_p_min[k], m.dev_p_max[k])
                add([(o + PD + k, 1.0), (o + PDIS + j, -1.0), (o + PC + j, 1.0)], 0.0, 0.0)
                c = []
                for ii in range(i + 1):  # soc_i = soc_0 + sum_{stages <= i} (p_c dt eff - p_d dt / eff)
                    c += [(ii * per + PC + j, dt * m.dev_eff[k]), (ii * per + PDIS + j, -dt / m.dev_eff[k])]
                ps = pvec((nl + ng) * N + j, -1.0)
                add(c, m.dev_soc_min[k], m.dev_soc_max[k], ps, ps)
                add([(o + PC + j, 1.0)], 0.0, INF)
                add([(o + PDIS + j, 1.0)], 0.0, INF)
            # angles (mpc.py:293-302)
            for b in range(nb):
                add([(o + TH + b, 1.0)], -np.pi, np.pi)
            add([(o + TH + slack_theta, 1.0)], 0.0, 0.0)
            # epigraph of max(0, |B_ft (theta_f - theta_t)| - beta rate)  (mpc.py:308-311, 148-155)
            for e, (f, t) in enumerate(zip(m.br_f, m.br_t)):
                lim = safety_margin * m.br_rate[e]
                add([(o + TH + f, B[f, t]), (o + TH + t, -B[f, t]), (o + SB + e, -1.0)], -INF, lim)
                add([(o + TH + f, -B[f, t]), (o + TH + t, B[f, t]), (o + SB + e, -1.0)], -INF, lim)
                add([(o + SB + e, 1.0)], 0.0, INF)
            # objective (mpc.py:304-313): generation of every non-renewable generator (slack included) + lambda x overloads
            w = gamma**i
            for k in range(nd):
                if m.dev_type[k] in (SLACK, CLASSICAL):
                    q[o + PD + k] += w
            for e in range(nbr):
                q[o + SB + e] += w * m.lamb
        self.A = np.array(rows)
        self.l0, self.u0 = np.array(lo, float), np.array(up, float)
        self.Lp, self.Up = np.array(Lp), np.array(Up)
        self.q = q
        self.m = len(rows)
        self.gens, self.des, self.loads = gens, des, loads
        self.base = float(m.baseMVA)

    def bounds(self, params):
        """[E, n_param] -> (l, u), each [E, m]."""
        P = torch.as_tensor(params, dtype=torch.float64)
        dev = P.device
        l = torch.as_tensor(self.l0, device=dev) + P @ torch.as_tensor(self.Lp.T, device=dev)
        u = torch.as_tensor(self.u0, device=dev) + P @ torch.as_tensor(self.Up.T, device=dev)
        return l, u

    def objective(self, x):
        return x @ torch.as_tensor(self.q, dtype=torch.float64, device=x.device)


class BatchedDCOPF:
    """The N-stage DC-OPF of every environment of a batch, solved on the device by ONE launch of the
    interior-point kernel (``anm_mpc_solve_f64``, ``csrc/anm_mpc.hpp``): one lane per stage, ``64 / 2^ceil(log2 N)``
    environments per wavefront, the network tables of the reduced program (``dcopf.py``) as scalar loads.

    ``solve(P_load_forecast [E, n_load, N], P_gen_forecast [E, n_gen, N], soc [E, n_des])`` -> the first-stage
    ``[P_gen.., P_des..]`` (p.u.); ``objective``, ``iters``, ``info`` and, on request, the whole primal solution stay
    available as tensors.  ``info[:, 0]`` is the final complementarity ``mu``, ``info[:, 1]`` a STATUS (0 ok, 1 a stage has
    no interior start, 2 an angle row left out of the solve is violated -- ``include/anm_mi355x.h``), ``info[:, 2]`` the
    largest dual residual.  ``converged`` folds them into the verdict every caller should apply."""

    TOL_DEFAULT, MAX_ITER_DEFAULT = 1e-11, 40   # the library's defaults (anm_mpc_capi.inc), always passed explicitly

    def __init__(self, simulator, gamma, safety_margin, planning_steps, tol=None, max_iter=None, keep_solution=False,
                 keep_trace=False, angle_rows=None, size_class=None):
        from .. import _lib

        self.backend, self.device = simulator.backend, simulator.device
        if getattr(self.backend, "generic", False) or size_class:
            # the simulator steps on the table-driven lane-group kernels of a library compiled for another topology; the
            # MPC kernel depends on the network's SIZES: a precompiled size class the network is padded into (no compile),
            # or a small library of its own (size_class=True forces a class: tests)
            self.backend = _lib.load_mpc_for_topology(simulator.model.topology(), size_class=size_class)
        self._device_ctx = simulator._device_ctx
        self._stream_ptr = lambda: _lib_stream(self.device)
        self.N = int(planning_steps)
        desc, self._keep = _lib.network_desc(simulator.model)
        self._handle = C.c_void_p()
        lib = self.backend.lib
        with self._device_ctx():
            self.backend.check(lib.anm_mpc_create(C.byref(desc), float(gamma), float(safety_margin), self.N,
                                                  C.byref(self._handle)), "anm_mpc_create")
        d = _lib.MpcDims()
        self.backend.check(lib.anm_mpc_dims_of(self._handle, C.byref(d)), "anm_mpc_dims_of")
        self.dims = d
        # angle_rows: None = the library's choice (dims.angle_rows: the rows |theta| <= pi ride through the solve only
        # where an angle can come near pi within the device limits); True / False force them in / out (left out, the
        # solution's angles are checked: info[:, 1] == 2 where one exceeds pi)
        # tolerance and iteration cap are always sent explicitly (0 would mean "the library's default": the trace buffer
        # below is sized by max_iter, and a default that changed under it would be an out-of-bounds write)
        self.tol = self.TOL_DEFAULT if tol is None else float(tol)
        self.max_iter = self.MAX_ITER_DEFAULT if max_iter is None else int(max_iter)
        if not (self.tol > 0.0 and self.max_iter > 0):
            raise ValueError("tol and max_iter must be positive")
        self.opts = _lib.MpcOpts(tol=self.tol, max_iter=self.max_iter, angle_rows=0 if angle_rows is None else (1 if angle_rows else 2))
        self.dual_tol = 1e-6 * (1.0 + float(simulator.lamb))   # against costs of 1 ... lamb per p.u.
        self.keep_solution, self.keep_trace = keep_solution, keep_trace
        self._E = None

    def tables(self):
        """host copy of the constant table the kernel reads (layout: ``mpc::Sz`` in csrc/anm_mpc.hpp)"""
        out = np.zeros(self.dims.table_doubles)
        self.backend.check(self.backend.lib.anm_mpc_get_tables(self._handle, out.ctypes.data_as(C.POINTER(C.c_double))),
                           "anm_mpc_get_tables")
        return out

    def _buffers(self, E):
        if self._E != E:
            d, f = self.dims, dict(dtype=torch.float64, device=self.device)
            self.u0 = torch.zeros((E, d.n_ctrl), **f)
            self.objective = torch.zeros(E, **f)
            self.iters = torch.zeros(E, dtype=torch.int32, device=self.device)
            self.info = torch.zeros((E, 3), **f)
            self.solution = torch.zeros((E, self.N, d.n_stage_vars), **f) if self.keep_solution else None
            self.trace = torch.full((E, self.max_iter + 1, 12), float("nan"), **f) if self.keep_trace else None
            self.opts.trace = None if self.trace is None else self.trace.data_ptr()
            self._E = E

    def solve(self, P_load_forecast, P_gen_forecast, soc):
        d = self.dims
        E = int(soc.shape[0])
        f = dict(dtype=torch.float64, device=self.device)
        # [E, n, N] (the reference's forecast layout, mpc.py:348-372) -> stage-major [E, N, n]
        pl = torch.as_tensor(P_load_forecast, **f).reshape(E, d.n_load, self.N).permute(0, 2, 1).contiguous()
        pg = torch.as_tensor(P_gen_forecast, **f).reshape(E, d.n_gen, self.N).permute(0, 2, 1).contiguous()
        sc = torch.as_tensor(soc, **f).reshape(E, d.n_des).contiguous()
        self._buffers(E)
        with self._device_ctx():
            rc = self.backend.lib.anm_mpc_solve_f64(
                self._handle, E, pl.data_ptr(), pg.data_ptr(), sc.data_ptr(), self.u0.data_ptr(), self.objective.data_ptr(),
                self.iters.data_ptr(), self.info.data_ptr(), 0 if self.solution is None else self.solution.data_ptr(),
                C.byref(self.opts), self._stream_ptr())
        self.backend.check(rc, "anm_mpc_solve_f64")
        return self.u0

    def act(self, forecast, env, act_low, act_high):
        """``MPCAgent.act`` as ONE launch (``anm_mpc_act_f64``): the forecasts are gathered inside the kernel -- ``forecast``
        1: constant, from the state rows of ``env``; 2: perfect, from its periodic tables; 3: the stream of a task drawn
        inside the step kernels, evaluated ahead (``anm_mpc_act_stream_f64``); 4: the same for the correlated series-noise
        task, rolled forward from ``env.exo_z`` (``anm_mpc_act_chain_f64``); 5: the expected forecast of a drawn task, the
        noise states rolled forward without draws (``anm_mpc_act_expect_f64``) -- and the first stage's set-points come back
        as the clipped MW action rows ``[E, 2 n_gen + 2 n_des]`` (a persistent buffer)."""
        d = self.dims
        E = int(env.num_envs)
        self._buffers(E)
        if getattr(self, "_action", None) is None or self._action.shape[0] != E:
            self._action = torch.zeros((E, 2 * d.n_gen + 2 * d.n_des), dtype=torch.float64, device=self.device)
        series_ptr, period = None, 0
        if forecast == 2 or (forecast in (3, 4, 5) and getattr(env, "_series", None) is not None):
            if getattr(self, "_series_src", None) is not env._series:
                self._series_src = env._series
                self._series_dev = torch.as_tensor(env._series, dtype=torch.float64, device=self.device).contiguous()
            series_ptr, period = self._series_dev.data_ptr(), int(self._series_dev.shape[1])
        same = env._state_same
        aux = None   # the time index is read from the last column of the state row (what `forecast()` does)
        soc = env.simulator.soc
        if forecast == 3:
            return self._act_stream(env, E, same, aux, series_ptr, period, soc, act_low, act_high)
        if forecast == 4:
            return self._act_chain(env, E, same, aux, series_ptr, period, soc, act_low, act_high)
        if forecast == 5:
            return self._act_expect(env, E, same, aux, series_ptr, period, soc, act_low, act_high)
        with self._device_ctx():
            rc = self.backend.lib.anm_mpc_act_f64(
                self._handle, E, int(forecast), env._state_buf.data_ptr(), None if same is None else env._state_obs.data_ptr(),
                None if same is None else same.data_ptr(), int(env._state_buf.shape[1]), None if aux is None else aux.data_ptr(),
                series_ptr, period, soc.data_ptr(), act_low.data_ptr(), act_high.data_ptr(), self._action.data_ptr(),
                self.u0.data_ptr(), self.objective.data_ptr(), self.iters.data_ptr(), self.info.data_ptr(), C.byref(self.opts),
                self._stream_ptr())
        self.backend.check(rc, "anm_mpc_act_f64")
        return self._action

    def _act_stream(self, env, E, same, aux, series_ptr, period, soc, act_low, act_high):
        from .. import _lib

        if not getattr(env, "_drawn", False):
            raise E_.ArgsError("the stream forecast needs an environment with exogenous='uniform' or 'series_noise'")
        if getattr(env, "exo_corr", None) is not None:
            raise E_.ArgsError("the stream forecast is a function of the step index alone: it does not serve a task with "
                               "correlated noise (exo_corr=)")
        # device copies of the ends and of the amplitude table (host arrays of the environment), cached per environment
        if getattr(self, "_exo_src", None) is not env:
            dev = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64, device=self.device).contiguous()  # noqa: E731
            self._exo_src, self._exo_dev = env, (dev(env.exo_low), dev(env.exo_high), dev(env.exo_noise))
        lo, hi, amp = self._exo_dev
        st = _lib.MpcStream(exo_mode=_lib.EXO_SERIES_NOISE if env._noisy else _lib.EXO_UNIFORM, rng_seed=int(env.rng_seed),
                            env_offset=int(env.env_offset), timestep=env.timestep.data_ptr(), reset_count=env._reset_count.data_ptr(),
                            exo_low=lo.data_ptr(), exo_high=hi.data_ptr(), exo_noise=None if amp is None else amp.data_ptr())
        with self._device_ctx():
            rc = self.backend.lib.anm_mpc_act_stream_f64(
                self._handle, E, env._state_buf.data_ptr(), None if same is None else env._state_obs.data_ptr(),
                None if same is None else same.data_ptr(), int(env._state_buf.shape[1]), None if aux is None else aux.data_ptr(),
                series_ptr, period, soc.data_ptr(), act_low.data_ptr(), act_high.data_ptr(), self._action.data_ptr(),
                self.u0.data_ptr(), self.objective.data_ptr(), self.iters.data_ptr(), self.info.data_ptr(), C.byref(self.opts),
                C.byref(st), self._stream_ptr())
        self.backend.check(rc, "anm_mpc_act_stream_f64")
        return self._action

    def _act_chain(self, env, E, same, aux, series_ptr, period, soc, act_low, act_high):
        from .. import _lib

        if not getattr(env, "_noisy", False) or getattr(env, "exo_corr", None) is None:
            raise E_.ArgsError("the chain forecast needs an environment with exogenous='series_noise' and exo_corr=")
        # device copies of the ends, the amplitude table and the AR(1) tables (host arrays of the environment), cached per
        # environment; exo_z is the environment's own tensor, read in place
        if getattr(self, "_chain_src", None) is not env:
            dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device=self.device).contiguous()  # noqa: E731
            self._chain_src, self._chain_dev = env, tuple(dev(a) for a in (env.exo_low, env.exo_high, env.exo_noise, env.exo_corr,
                                                                           env._exo_innov))
        lo, hi, amp, rho, innov = self._chain_dev
        st = _lib.MpcChain(exo_mode=_lib.EXO_SERIES_NOISE, rng_seed=int(env.rng_seed), env_offset=int(env.env_offset),
                           timestep=env.timestep.data_ptr(), reset_count=env._reset_count.data_ptr(), exo_low=lo.data_ptr(),
                           exo_high=hi.data_ptr(), exo_noise=amp.data_ptr(), exo_rho=rho.data_ptr(), exo_innov=innov.data_ptr(),
                           exo_z=env.exo_z.data_ptr())
        with self._device_ctx():
            rc = self.backend.lib.anm_mpc_act_chain_f64(
                self._handle, E, env._state_buf.data_ptr(), None if same is None else env._state_obs.data_ptr(),
                None if same is None else same.data_ptr(), int(env._state_buf.shape[1]), None if aux is None else aux.data_ptr(),
                series_ptr, period, soc.data_ptr(), act_low.data_ptr(), act_high.data_ptr(), self._action.data_ptr(),
                self.u0.data_ptr(), self.objective.data_ptr(), self.iters.data_ptr(), self.info.data_ptr(), C.byref(self.opts),
                C.byref(st), self._stream_ptr())
        self.backend.check(rc, "anm_mpc_act_chain_f64")
        return self._action

    def _act_expect(self, env, E, same, aux, series_ptr, period, soc, act_low, act_high):
        from .. import _lib

        if not getattr(env, "_drawn", False):
            raise E_.ArgsError("the expected forecast needs an environment with exogenous='uniform' or 'series_noise'")
        # device copies of the ends, the amplitude table and rho (host arrays of the environment; None where the task has
        # none), cached per environment; exo_z is the environment's own tensor, read in place
        if getattr(self, "_expect_src", None) is not env:
            dev = lambda a: None if a is None else torch.tensor(np.array(a, dtype=np.float64), device=self.device)  # noqa: E731
            self._expect_src, self._expect_dev = env, tuple(dev(a) for a in (env.exo_low, env.exo_high, env.exo_noise, env.exo_corr))
        lo, hi, amp, rho = self._expect_dev
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        st = _lib.MpcExpect(exo_mode=_lib.EXO_SERIES_NOISE if env._noisy else _lib.EXO_UNIFORM, exo_low=lo.data_ptr(),
                            exo_high=hi.data_ptr(), exo_noise=ptr(amp), exo_rho=ptr(rho), exo_z=None if rho is None else env.exo_z.data_ptr())
        with self._device_ctx():
            rc = self.backend.lib.anm_mpc_act_expect_f64(
                self._handle, E, env._state_buf.data_ptr(), None if same is None else env._state_obs.data_ptr(),
                None if same is None else same.data_ptr(), int(env._state_buf.shape[1]), None if aux is None else aux.data_ptr(),
                series_ptr, period, soc.data_ptr(), act_low.data_ptr(), act_high.data_ptr(), self._action.data_ptr(),
                self.u0.data_ptr(), self.objective.data_ptr(), self.iters.data_ptr(), self.info.data_ptr(), C.byref(self.opts),
                C.byref(st), self._stream_ptr())
        self.backend.check(rc, "anm_mpc_act_expect_f64")
        return self._action

    @property
    def converged(self):
        """``[E]`` bool: the last solve reached the complementarity tolerance ``mu <= tol (1 + |objective|)`` (the kernel's
        own stop test, read from ``info[:, 0]``: a solve that meets it in its last allowed iteration counts), status 0,
        and a dual residual that is small against the costs (the kernel's stop test does not look at it)."""
        mu_ok = self.info[:, 0] <= self.tol * (1.0 + self.objective.abs())
        return mu_ok & (self.info[:, 1] == 0) & (self.info[:, 2] <= self.dual_tol)

    def __del__(self):
        try:
            if getattr(self, "_handle", None) and self._handle.value:
                self.backend.lib.anm_mpc_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass


def _lib_stream(device):
    if device.type != "cuda":
        return None
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class MPCAgent:
    """``MPCAgent(simulator, action_space, gamma, safety_margin=0.9, planning_steps=1)`` (``mpc.py:33-122``):
    ``act(env)`` returns the ``[num_envs, action_dim]`` tensor of the first-stage set-points (MW; reactive
    set-points 0, ``mpc.py:383-388``), clipped to the action space.

    ``last_converged`` is the per-environment mask of solves that reached the tolerance; like the reference, which
    prints ``OPF problem is <status>`` and goes on (``mpc.py:377-379``), ``act`` warns when it is not all true."""

    def __init__(self, simulator, action_space, gamma, safety_margin=0.9, planning_steps=1, tol=None, max_iter=None,
                 size_class=None):
        self.simulator = simulator
        self.action_space = action_space
        self.gamma, self.safety_margin, self.planning_steps = gamma, safety_margin, int(planning_steps)
        self.baseMVA, self.lamb, self.delta_t = simulator.baseMVA, simulator.lamb, simulator.delta_t
        m = simulator.model
        self.load_ids = [m.dev_ids[k] for k in m.load_idx]
        self.non_slack_gen_ids = [m.dev_ids[k] for k in m.gen_idx]
        self.des_ids = [m.dev_ids[k] for k in m.des_idx]
        self.device = simulator.device
        self.solver = BatchedDCOPF(simulator, gamma, safety_margin, planning_steps, tol=tol, max_iter=max_iter, size_class=size_class)
        self._acted, self._conv = False, None
        # `tensor / python scalar` is a multiplication by the reciprocal on the GPU; the reference divides (`/ self.baseMVA`):
        # the forecasts are divided by this 0-dim tensor (a true division), like the fused kernel does
        self._base_t = torch.tensor(float(self.baseMVA), dtype=torch.float64, device=self.device)
        self._lo = torch.as_tensor(np.asarray(action_space.low, float), device=self.device)
        self._hi = torch.as_tensor(np.asarray(action_space.high, float), device=self.device)

    def forecast(self, env):
        """-> (P_load_forecast [E, n_load, N], P_gen_forecast [E, n_gen, N]) in p.u.  (``mpc.py:348-372``)."""
        raise NotImplementedError()

    def _soc(self, env):
        return env.simulator.soc  # p.u., [E, n_des]  (mpc.py:417 reads des_soc in pu)

    def solve(self, P_load_forecast, P_gen_forecast, soc):
        """-> first-stage [P_gen.., P_des..] in p.u., [E, n_gen + n_des]"""
        return self.solver.solve(P_load_forecast, P_gen_forecast, soc)

    FUSED_FORECAST = 0   # the stock agents: which forecast anm_mpc_act_f64 gathers inside the kernel (0: none, use forecast())

    def _fused(self, env):
        """The whole of act() can run as one launch: a stock forecast (not overridden by a subclass), the stock solve and
        state of charge, a batched environment of this package that has what the kernel reads."""
        cls = type(self)
        mode = self.FUSED_FORECAST
        stock = {1: MPCAgentConstant, 2: MPCAgentPerfect, 3: MPCAgentPerfectStream, 4: MPCAgentPerfectChain,
                 5: MPCAgentExpected}.get(mode)
        symbol = {3: "anm_mpc_act_stream_f64", 4: "anm_mpc_act_chain_f64", 5: "anm_mpc_act_expect_f64"}.get(mode, "anm_mpc_act_f64")
        # what the kernel reads: the tables (2), a drawn mode (3, 5), the noise states (4); the time index in the last
        # column where a table is indexed
        has = {1: True, 2: getattr(env, "_series", None) is not None, 3: bool(getattr(env, "_drawn", False)),
               4: bool(getattr(env, "_noisy", False)) and getattr(env, "exo_z", None) is not None,
               5: bool(getattr(env, "_drawn", False))}.get(mode, False)
        indexed = mode in (2, 4) or (mode in (3, 5) and getattr(env, "_noisy", False))
        return (stock is not None and cls.forecast is stock.forecast and cls.solve is MPCAgent.solve and cls._soc is MPCAgent._soc
                and hasattr(self.solver.backend.lib, symbol) and hasattr(env, "_state_buf") and has
                and env._state_buf.shape[1] >= 2 * env.simulator.model.N_device + env.simulator.model.N_des
                + env.simulator.model.N_non_slack_gen + (1 if indexed else 0))

    warn_unconverged = True   # False: act() neither synchronises nor launches anything but the solve (last_converged stays lazy)
    # False (default): act() returns a tensor of its own, like the reference's fresh array and like the unfused path --
    # actions kept across steps (rollout lists, replay buffers) stay what they were.  True: the fused path returns the
    # solver's persistent buffer, which the next act() overwrites (no allocation, no copy kernel: what bench.py times)
    reuse_action_buffer = False

    @property
    def last_converged(self):
        """per-environment mask of the solves of the last ``act`` that reached the tolerance (``BatchedDCOPF.converged``);
        None before the first ``act``"""
        if self._conv is None and self._acted:
            self._conv = self.solver.converged
        return self._conv

    def _check_converged(self, n):
        self._acted, self._conv = True, None
        if self.warn_unconverged and not bool(self.last_converged.all()):
            import warnings

            warnings.warn("OPF problem did not reach the tolerance in %d of %d environments (see last_converged)"
                          % (int((~self.last_converged).sum()), n))

    def act(self, env):
        """``env``: a batched environment -> ``[num_envs, action_dim]`` tensor; or one of the NumPy-facing
        single-environment classes (``ANMEnv``, ``ANM6``, ``ANM6Easy``) -> 1-D NumPy action, as in the reference's
        ``examples/mpc_*.py``.  With a stock forecast the whole call is ONE kernel launch (forecast gather, solve, scaling
        to MW, clipping: ``anm_mpc_act_f64``); the tensor returned is the caller's own unless ``reuse_action_buffer`` is set
        (then it is the solver's buffer, overwritten by the next call)."""
        if hasattr(env, "vec"):
            return self.act(env.vec)[0].cpu().numpy()
        if self._fused(env):
            a = self.solver.act(self.FUSED_FORECAST, env, self._lo, self._hi)
            self._check_converged(a.shape[0])
            return a if self.reuse_action_buffer else a.clone()
        pl, pg = self.forecast(env)
        u0 = self.solve(pl, pg, self._soc(env)) * self.baseMVA
        ng = self.solver.dims.n_gen
        P_gen, P_des = u0[:, :ng], u0[:, ng:]
        a = torch.cat((P_gen, torch.zeros_like(P_gen), P_des, torch.zeros_like(P_des)), dim=1)
        # reached the tolerance with status 0 and a dual residual that is small against the costs (BatchedDCOPF.converged)
        self._check_converged(a.shape[0])
        return torch.minimum(torch.maximum(a, self._lo), self._hi)  # mpc.py:341-344


class MPCAgentConstant(MPCAgent):
    """Constant forecasts: the current loads and generation potentials persist over the horizon
    (``mpc_constant.py:24-35``).  They are read from the state vector: dev_p of the loads and gen_p_max, MW."""

    FUSED_FORECAST = 1

    def forecast(self, env):
        m = env.simulator.model
        s = env.state
        D, nd = m.N_device, m.N_des
        pl = s[:, list(m.load_idx)] / self._base_t
        pg = s[:, 2 * D + nd : 2 * D + nd + m.N_non_slack_gen] / self._base_t
        N = self.planning_steps
        return pl.unsqueeze(2).expand(-1, -1, N), pg.unsqueeze(2).expand(-1, -1, N)


class MPCAgentPerfect(MPCAgent):
    """Perfect forecasts for series-mode tasks (ANM6Easy): the next N columns of the task's periodic tables
    (``mpc_perfect.py:24-40``).

    On a ``exogenous="series_noise"`` task this is the PROFILE forecast -- the noise-free table the noise is added to --
    not a perfect one: the agent that knows the draws too is :class:`MPCAgentPerfectStream`
    (:class:`MPCAgentPerfectChain` with ``exo_corr=``), and the informed baseline that does NOT know them -- the profile
    plus the conditional mean of the noise given the task's current noise state, which this forecast ignores -- is
    :class:`MPCAgentExpected`.  A task without tables
    (``exogenous="uniform"``, a host hook) has no such forecast: ``ArgsError``."""

    FUSED_FORECAST = 2

    def forecast(self, env):
        if getattr(env, "_series", None) is None:
            raise E_.ArgsError("MPCAgentPerfect forecasts from the periodic tables of a series-mode task and this environment has "
                               "none; for a task drawn inside the step kernels (exogenous='uniform' / 'series_noise') use "
                               "MPCAgentPerfectStream")
        tab = torch.as_tensor(env._series, dtype=torch.float64, device=self.device)  # [n_load + n_gen, period]
        period = tab.shape[1]
        t0 = env.state[:, -1].long() + 1
        idx = (t0.unsqueeze(1) + torch.arange(self.planning_steps, device=self.device).unsqueeze(0)) % period  # [E, N]
        cols = tab[:, idx]  # [n, E, N]
        nl = env.simulator.N_load
        return cols[:nl].permute(1, 0, 2) / self._base_t, cols[nl:].permute(1, 0, 2) / self._base_t


class MPCAgentPerfectStream(MPCAgent):
    """Perfect forecasts for the tasks whose loads and generator potentials are drawn INSIDE the step kernels
    (``exogenous="uniform"``, ``exogenous="series_noise"``): stage ``i`` is the task's own draw of step index
    ``timestep + 1 + i`` of the running episode -- a pure function of (seed, global environment index, reset epoch, step
    index, unit), so the lanes of the solve evaluate the Philox stream ahead themselves (``rng.exo_forecast`` is the
    specification; ``anm_mpc_act_stream_f64``, still ONE launch per ``act``).  This is the upper bound a learned policy is
    measured against on these tasks, what :class:`MPCAgentPerfect` is on a series-mode task.

    The forecast of an environment that is terminated or past its episode limit is the same pure function (the step that
    follows resets it and ignores the action); the horizon is not cut at ``max_episode_steps`` -- the reference's perfect
    agent looks past episode ends too.

    A task with correlated noise (``exo_corr=``) is refused, ``ArgsError``: its draws depend on the noise state of every
    unit, not on the step index alone, and this agent's forecast is a pure function of the step index.
    (:class:`MPCAgentPerfectChain` rolls the chain forward from ``exo_z`` inside the solve and is the perfect agent of such
    a task; :class:`MPCAgentPerfect`, the profile forecast, and :class:`MPCAgentConstant` read only state and tables and
    work on it too.)"""

    FUSED_FORECAST = 3
    _CORR_REFUSAL = ("MPCAgentPerfectStream has no forecast for a task with correlated noise (exo_corr=): the draws depend "
                     "on the noise state exo_z, not on the step index alone; use MPCAgentPerfectChain")

    def __init__(self, simulator, *args, **kw):
        if getattr(simulator, "exogenous", None) not in ("uniform", "series_noise"):
            raise E_.ArgsError("MPCAgentPerfectStream needs the simulator of an environment with exogenous='uniform' or "
                               "'series_noise' (the modes drawn inside the step kernels); this one is in mode %r"
                               % (getattr(simulator, "exogenous", None),))
        if getattr(simulator, "exo_corr", None) is not None:
            raise E_.ArgsError(self._CORR_REFUSAL)
        super().__init__(simulator, *args, **kw)

    def _drawn_env(self, env):
        if not getattr(env, "_drawn", False):
            raise E_.ArgsError("MPCAgentPerfectStream needs an environment with exogenous='uniform' or 'series_noise'")
        if getattr(env, "exo_corr", None) is not None:
            raise E_.ArgsError(self._CORR_REFUSAL)

    def act(self, env):
        if not hasattr(env, "vec"):
            self._drawn_env(env)
        return super().act(env)

    def forecast(self, env):
        """The unfused path: the specification itself (``rng.exo_forecast_v``, exact) on the host."""
        from .. import rng

        self._drawn_env(env)
        noisy = bool(env._noisy)
        f = rng.exo_forecast_v(
            env.rng_seed, env.env_offset, env._reset_count.cpu().numpy(), env.timestep.cpu().numpy(), self.planning_steps,
            env.exo_low, env.exo_high, series=env._series if noisy else None, noise=env.exo_noise if noisy else None,
            aux=env.state[:, -1].cpu().numpy().astype(np.int64) if noisy else None)
        f = torch.as_tensor(f, dtype=torch.float64, device=self.device)   # [E, n_load + n_gen, N] MW
        nl = env.simulator.N_load
        return f[:, :nl] / self._base_t, f[:, nl:] / self._base_t


class MPCAgentPerfectChain(MPCAgent):
    """Perfect forecasts for the series-noise task with CORRELATED noise (``exogenous="series_noise", exo_corr=rho``): stage
    ``i`` is the step kernels' own AR(1) recurrence applied ``i + 1`` times to the environment's noise states ``exo_z``, at
    step index ``timestep + 1 + i`` and table index ``aux + 1 + i`` of the running episode -- what the environment then
    draws, bit for bit (``rng.exo_forecast_corr`` is the specification).  The stages are the lanes of the solve: each draws
    its own factor, the states travel up the group one stage per exchange (``anm_mpc_act_chain_f64``, still ONE launch per
    ``act``; ``exo_z`` is only read).  This is the upper bound a learned policy is measured against on such a task.

    As for :class:`MPCAgentPerfectStream`, the forecast of an environment that is terminated or past its episode limit is
    the same pure function, and the horizon is not cut at ``max_episode_steps``.  An uncorrelated drawn task
    (``exo_corr=None``) keeps no noise states: ``ArgsError``, use :class:`MPCAgentPerfectStream`."""

    FUSED_FORECAST = 4

    @staticmethod
    def _check_task(exogenous, exo_corr, what):
        if exogenous != "series_noise":
            raise E_.ArgsError("MPCAgentPerfectChain needs %s with exogenous='series_noise' and exo_corr= (the task with "
                               "correlated noise); this one is in mode %r" % (what, exogenous))
        if exo_corr is None:
            raise E_.ArgsError("MPCAgentPerfectChain rolls the noise states of an exogenous='series_noise' task with correlated noise forward "
                               "and %s has none (exo_corr=None); for an uncorrelated task drawn inside the step kernels use "
                               "MPCAgentPerfectStream" % what)

    def __init__(self, simulator, *args, **kw):
        self._check_task(getattr(simulator, "exogenous", None), getattr(simulator, "exo_corr", None), "the simulator of an environment")
        super().__init__(simulator, *args, **kw)

    def _chain_env(self, env):
        self._check_task(getattr(env, "exogenous", None), getattr(env, "exo_corr", None), "an environment")

    def act(self, env):
        if not hasattr(env, "vec"):
            self._chain_env(env)
        return super().act(env)

    def forecast(self, env):
        """The unfused path: the specification itself (``rng.exo_forecast_corr_v``, exact) on the host, from ``env.exo_z``."""
        from .. import rng

        self._chain_env(env)
        f = rng.exo_forecast_corr_v(
            env.rng_seed, env.env_offset, env._reset_count.cpu().numpy(), env.timestep.cpu().numpy(), self.planning_steps,
            env.state[:, -1].cpu().numpy().astype(np.int64), env.exo_z.cpu().numpy(), env._series, env.exo_noise, env.exo_corr,
            env._exo_innov, env.exo_low, env.exo_high)
        f = torch.as_tensor(f, dtype=torch.float64, device=self.device)   # [E, n_load + n_gen, N] MW
        nl = env.simulator.N_load
        return f[:, :nl] / self._base_t, f[:, nl:] / self._base_t


class MPCAgentExpected(MPCAgent):
    """Conditional-mean forecasts for the tasks drawn INSIDE the step kernels (``exogenous="uniform"``, ``"series_noise"``,
    with or without ``exo_corr=``): the forecast of an operator who knows the task's noise model and its current state, but
    not the future draws.  The innovations have mean 0, so with correlated noise stage ``i`` maps the noise state
    ``rho^(i+1) exo_z`` -- the step kernels' own recurrence with the innovation at its mean, applied ``i + 1`` times -- at
    table index ``aux + 1 + i``; without correlation it maps a noise of 0, and in uniform mode every stage is the middle of
    the ends (``rng.exo_forecast_expected`` is the specification).  The stages are the lanes of the solve and the states
    travel up the group like the chain agent's, without any draw (``anm_mpc_act_expect_f64``, ONE launch per ``act``;
    ``exo_z`` is only read).

    This is the honest baseline of these tasks: :class:`MPCAgentConstant` ignores the daily profile, :class:`MPCAgentPerfect`
    ignores the noise state, and the perfect agents (:class:`MPCAgentPerfectStream`, :class:`MPCAgentPerfectChain`) know
    draws nobody can know.  A pure function of the table index and the row of ``exo_z``: the same for an environment that
    is terminated or past its limit, and the horizon is not cut at ``max_episode_steps``.  A series-mode or host-hook task
    draws nothing inside the kernels: ``ArgsError``."""

    FUSED_FORECAST = 5

    @staticmethod
    def _check_task(exogenous, what):
        if exogenous not in ("uniform", "series_noise"):
            raise E_.ArgsError("MPCAgentExpected needs %s with exogenous='uniform' or 'series_noise' (the modes drawn inside the "
                               "step kernels); this one is in mode %r: a series-mode task is forecast by MPCAgentPerfect, any "
                               "task by MPCAgentConstant" % (what, exogenous))

    def __init__(self, simulator, *args, **kw):
        self._check_task(getattr(simulator, "exogenous", None), "the simulator of an environment")
        super().__init__(simulator, *args, **kw)

    def _drawn_env(self, env):
        self._check_task(getattr(env, "exogenous", None), "an environment")

    def act(self, env):
        if not hasattr(env, "vec"):
            self._drawn_env(env)
        return super().act(env)

    def forecast(self, env):
        """The unfused path: the rows the step kernels wrote themselves (``env.exo_forecast``, a float64 environment built
        with ``forecast_horizon >= planning_steps``: a slice on the device, the prefix property of the forecast), else the
        specification itself (``rng.exo_forecast_expected_v``, exact) on the host."""
        from .. import rng

        self._drawn_env(env)
        nl = env.simulator.N_load
        H = getattr(env, "forecast_horizon", None)
        if H is not None and H >= self.planning_steps and env.exo_forecast.dtype == torch.float64:
            f = env.exo_forecast[:, :, :self.planning_steps].to(self.device)
            return f[:, :nl] / self._base_t, f[:, nl:] / self._base_t
        noisy, corr = bool(env._noisy), env.exo_corr is not None
        f = rng.exo_forecast_expected_v(
            env.num_envs, self.planning_steps, env.exo_low, env.exo_high,
            aux=env.state[:, -1].cpu().numpy().astype(np.int64) if noisy else None, z=env.exo_z.cpu().numpy() if corr else None,
            series=env._series if noisy else None, noise=env.exo_noise if noisy else None, rho=env.exo_corr if corr else None)
        f = torch.as_tensor(f, dtype=torch.float64, device=self.device)   # [E, n_load + n_gen, N] MW
        return f[:, :nl] / self._base_t, f[:, nl:] / self._base_t
