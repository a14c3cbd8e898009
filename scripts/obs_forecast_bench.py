#!/usr/bin/env python
"""Time the env-step of the correlated series-noise task without and with the expected forecast the step kernels write
beside the state row (``forecast_horizon``), on ANM6Easy (65 536 environments, thread-per-environment family) and on the
30-bus feeder (16 384 environments, radial lane-group family).  The method is that of scripts/exo_corr_bench.py: the step entry
point called directly between two HIP events, 200 steps after 20 warm-up steps, three timed runs per process, no autoreset,
one JSON line per process.  `--root DIR` imports the package from another checkout, so that revisions can be alternated on
one card:

    python scripts/obs_forecast_bench.py --net anm6 --root ../parent      (a) the parent revision, exo_corr=0.8
    python scripts/obs_forecast_bench.py --net anm6                       (b) this revision, the feature off
    python scripts/obs_forecast_bench.py --net anm6 --horizon 8           (c) H = 8, float64
    python scripts/obs_forecast_bench.py --net anm6 --horizon 8 --io32    (d) H = 8, float32 I/O
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corr", default="0.8", help="'none' or a correlation in [0, 1)")
    ap.add_argument("--horizon", type=int, default=0, help="forecast_horizon (0: the keyword is not passed: works on older revisions)")
    ap.add_argument("--io32", action="store_true", help="io_dtype=torch.float32 (actions, observations, reward and the forecast)")
    ap.add_argument("--net", choices=["anm6", "case30"], default="anm6")
    ap.add_argument("--envs", type=int, default=0, help="0: 65 536 for anm6, 16 384 for case30")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--impl", default=None, help="default: thread for anm6, radial for case30")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import numpy as np
    import torch

    from gym_anm_amd import networks
    from gym_anm_amd.envs.anm6 import anm6easy_series
    from gym_anm_amd.envs.anm_env import BatchedANMEnv
    from gym_anm_amd.model import NetworkModel

    dev = torch.device("cuda:0")
    E_ = a.envs or (65536 if a.net == "anm6" else 16384)
    impl = a.impl or ("thread" if a.net == "anm6" else "radial")
    net = networks.anm6_network() if a.net == "anm6" else networks.synthetic_radial_network(30, 0)
    m = NetworkModel(net, 0.25, 100)
    n_exo = m.N_load + m.N_non_slack_gen
    lo, hi = np.zeros(n_exo), np.zeros(n_exo)
    for s, k in enumerate(m.load_idx):
        lo[s] = m.dev_p_min[k] * m.baseMVA
    for g, k in enumerate(m.gen_idx):
        hi[m.N_load + g] = m.dev_p_max[k] * m.baseMVA
    if a.net == "anm6":
        ser = anm6easy_series()
        amp = 0.25 * np.abs(ser)
    else:   # the feeder task of scripts/exo_noise_bench.py: a smooth daily profile, 10 % of every unit's range as amplitude
        j = np.arange(96)
        phase = 2 * np.pi * np.arange(n_exo) / n_exo
        ser = np.ascontiguousarray((lo + hi)[:, None] * (0.5 + 0.3 * np.sin(2 * np.pi * j[None, :] / 96 + phase[:, None])))
        amp = np.ascontiguousarray(np.broadcast_to(0.1 * np.abs(lo + hi)[:, None], ser.shape))
    period = ser.shape[1]
    kw = dict(aux_bounds=np.array([[0, 1e9]]), costs_clipping=(1, 100), seed=7, num_envs=E_, device="cuda:0", tol=1e-6,
              max_iter=a.max_iter, impl=impl, exogenous="series_noise", series=ser, exo_noise=amp)
    if a.corr != "none":
        kw["exo_corr"] = float(a.corr)
    if a.horizon:
        kw["forecast_horizon"] = a.horizon
    if a.io32:
        kw["io_dtype"] = torch.float32
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **kw)
    env.check_actions = False
    sim = env.simulator
    gen = torch.Generator(device=dev).manual_seed(5)
    f64 = dict(dtype=torch.float64, device=dev)
    lo_t, hi_t, ser_t = torch.as_tensor(lo, **f64), torch.as_tensor(hi, **f64), torch.as_tensor(ser, **f64)
    a_lo, a_hi = torch.as_tensor(env.action_space.low, **f64), torch.as_tensor(env.action_space.high, **f64)
    n_pool = 16
    actions = [(a_lo + (a_hi - a_lo) * torch.rand((E_, a_lo.numel()), generator=gen, **f64)).contiguous() for _ in range(n_pool)]
    if a.io32:   # (the float32 of the same draws: not the same steps bit for bit, the same workload)
        actions = [x.float().contiguous() for x in actions]
    t0_idx = torch.randint(0, period, (E_,), generator=gen, device=dev)      # the table index every environment starts at

    # the same initial rows for every variant: the table at t0, Q = 0, SoC mid-range
    D, nd = m.N_device, m.N_des
    s0 = torch.zeros((E_, env.state_N), **f64)
    x = torch.minimum(torch.maximum(ser_t.t()[t0_idx], lo_t), hi_t)
    for s, k in enumerate(m.load_idx):
        s0[:, k] = x[:, s]
    for g, k in enumerate(m.gen_idx):
        s0[:, k] = x[:, m.N_load + g]
        s0[:, 2 * D + nd + g] = x[:, m.N_load + g]
    for e, k in enumerate(m.des_idx):
        s0[:, 2 * D + e] = 0.5 * (m.dev_soc_min[k] + m.dev_soc_max[k]) * m.baseMVA
    s0[:, -1] = t0_idx.to(torch.float64)

    times, iters, dead = [], [], []
    for rep in range(a.repeat):
        env._reset_count.zero_()            # (every timed run replays the same episodes)
        env.reset(options={"init_state": s0})
        for k in range(a.warmup):
            env._step_call(actions[k % n_pool].data_ptr(), None, None)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(a.steps):
            env._step_call(actions[(a.warmup + k) % n_pool].data_ptr(), None, None)
        t1.record()
        torch.cuda.synchronize()
        times.append(1e3 * t0.elapsed_time(t1) / a.steps)
        alive = ~env.terminated
        iters.append(float(sim.nr_iters[alive].double().mean()) if bool(alive.any()) else float("nan"))
        dead.append(float(env.terminated.double().mean()))
    print(json.dumps(dict(label=a.label or ("corr=%s H=%d%s" % (a.corr, a.horizon, " f32" if a.io32 else "")), corr=a.corr, horizon=a.horizon,
                          io32=bool(a.io32), net=a.net, impl=impl, envs=E_, max_iter=a.max_iter, steps=a.steps,
                          us_per_step=[round(t, 2) for t in times], us_min=round(min(times), 2), us_max=round(max(times), 2),
                          mean_newton_iters=round(float(np.mean(iters)), 3), terminated_share_at_end=round(float(np.mean(dead)), 4),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
