#!/usr/bin/env python
"""Time the env-step of a stochastic task -- P_load ~ U(p_min, 0), P_pot ~ U(0, p_max) per step -- on the 30-bus feeder
(BASELINE.json config 4) in the two ways the package offers:

  uniform  BatchedANMEnv(exogenous="uniform"): the draws are made inside the step kernel (one launch per step);
  hook     the host-hook path: `exo` / `aux_next` handed to anm_step_f64 from a PRE-GENERATED pool of device tensors, so the
           cost of generating the draws (and of next_vars() itself) is left out in this path's favour.  The pool holds one
           tensor per step: with a short pool that repeats, the environments a (draw, action) pair collapses are dead after
           its first round and the later steps meet no diverging solve at all -- milder inputs than the task's.

Both call the step entry point directly (no action checks, no Python hook) between two HIP events.  One JSON line per run.
`--root DIR` imports the package from another checkout (the hook path exists on older revisions too), so that both can be
timed in one process sequence on the same card:

    python scripts/exo_uniform_bench.py --mode uniform --max-iter 100
    python scripts/exo_uniform_bench.py --mode hook --max-iter 100 --root ../parent
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["uniform", "hook"], required=True)
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--impl", default="radial")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import numpy as np
    import torch

    from gym_anm_amd import networks
    from gym_anm_amd.envs.anm_env import BatchedANMEnv

    dev = torch.device("cuda:0")
    net = networks.synthetic_radial_network(30, 0)
    kw = dict(aux_bounds=np.array([[0, 1e9]]), costs_clipping=(1, 100), seed=7, num_envs=a.envs, device="cuda:0", tol=1e-6,
              max_iter=a.max_iter, impl=a.impl)
    if a.mode == "uniform":
        kw["exogenous"] = "uniform"
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **kw)
    env.check_actions = False
    sim, m = env.simulator, env.simulator.model
    n_exo = sim.N_load + sim.N_non_slack_gen
    lo, hi = np.zeros(n_exo), np.zeros(n_exo)
    for s, k in enumerate(m.load_idx):
        lo[s] = m.dev_p_min[k] * m.baseMVA
    for g, k in enumerate(m.gen_idx):
        hi[m.N_load + g] = m.dev_p_max[k] * m.baseMVA
    gen = torch.Generator(device=dev).manual_seed(5)
    f64 = dict(dtype=torch.float64, device=dev)
    lo_t, hi_t = torch.as_tensor(lo, **f64), torch.as_tensor(hi, **f64)
    a_lo, a_hi = torch.as_tensor(env.action_space.low, **f64), torch.as_tensor(env.action_space.high, **f64)
    n_pool = 16
    actions = [(a_lo + (a_hi - a_lo) * torch.rand((a.envs, a_lo.numel()), generator=gen, **f64)).contiguous() for _ in range(n_pool)]
    n_exo_pool = (a.warmup + a.steps) if a.mode == "hook" else 1
    exo = [(lo_t + (hi_t - lo_t) * torch.rand((a.envs, n_exo), generator=gen, **f64)).contiguous() for _ in range(n_exo_pool)]
    aux = [torch.full((a.envs, 1), float(k + 1), **f64) for k in range(n_pool)]

    def initial_rows():   # the same kind of initial state for both paths: exogenous part uniform, Q and SoC mid-range
        D, nd = m.N_device, m.N_des
        s0 = torch.zeros((a.envs, env.state_N), **f64)
        x = exo[0]
        for s, k in enumerate(m.load_idx):
            s0[:, k] = x[:, s]
        for g, k in enumerate(m.gen_idx):
            s0[:, k] = x[:, m.N_load + g]
            s0[:, 2 * D + nd + g] = x[:, m.N_load + g]
        for e, k in enumerate(m.des_idx):
            s0[:, 2 * D + e] = 0.5 * (m.dev_soc_min[k] + m.dev_soc_max[k])
        return s0

    def step(k):
        if a.mode == "uniform":
            env._step_call(actions[k % n_pool].data_ptr(), None, None)
        else:
            env._step_call(actions[k % n_pool].data_ptr(), exo[k % n_exo_pool].data_ptr(), aux[k % n_pool].data_ptr())

    s0 = initial_rows()
    times, iters, dead = [], [], []
    for rep in range(a.repeat):
        env.reset(options={"init_state": s0})
        for k in range(a.warmup):
            step(k)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(a.steps):
            step(a.warmup + k)
        t1.record()
        torch.cuda.synchronize()
        times.append(1e3 * t0.elapsed_time(t1) / a.steps)
        alive = ~env.terminated
        iters.append(float(sim.nr_iters[alive].double().mean()) if bool(alive.any()) else float("nan"))
        dead.append(float(env.terminated.double().mean()) / (a.warmup + a.steps))
    print(json.dumps(dict(label=a.label or a.mode, mode=a.mode, impl=a.impl, envs=a.envs, max_iter=a.max_iter, steps=a.steps,
                          us_per_step=[round(t, 2) for t in times], us_min=round(min(times), 2), us_max=round(max(times), 2),
                          mean_newton_iters=round(float(np.mean(iters)), 3),
                          collapsed_share_per_step=float(np.mean(dead)), device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
