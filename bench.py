#!/usr/bin/env python
"""Headline benchmark: env-steps/sec of ANM6Easy at num_envs=65536 per MI355X (BASELINE.json).

    python bench.py --gpus 1 --steps 200 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one ``ANM6EasyVec.step(action)`` over the whole batch = one launch of the fused HIP
kernel: fused next_vars lookup, set-point projection, Newton-Raphson AC power flow (flat start,
||F||inf <= tol, cap max_iter), branch flows, reward + clipping, state and observation, plus
in-kernel autoreset of the environments that collapsed at the previous step (random agent: ~0.5 %
of the environments per step), so every environment does a full simulator transition every step.
Actions are uniform in the action Box (seeded), pre-generated in HBM; nothing is copied to or from
the host and nothing synchronises inside the timed region.

Multi-GPU: environments are independent, so the batch is sharded (65536 per rank, weak scaling)
with no data-path collective; RCCL only carries the max-over-ranks time and the step total.

A plain run sets up, warms up, times the --steps steps and prints the JSON line; its roofline
divides the algorithmic bytes by the step time from HIP events over the timed steps.

    --dump-outputs DIR  after the timed steps, what the last one handed its caller (observation,
                        reward, terminated, truncated) as DIR/<name>.npy in float64 -- inputs are
                        seeded, so two builds of the project can be compared output for output
    --full              everything beyond the headline figure, each in runs of its own:
  roofline     -- algorithmic HBM bytes per launch / kernel duration (launches issued back to back
                  from C, HIP events on the launch stream) against the 8 TB/s HBM3E peak, the PMC
                  traffic and fp64 issue figures, iteration and collapse statistics;
  config       -- the cap-20 and tol-1e-5 variants, every other BASELINE configuration;
  cpu_baseline -- the NumPy/SciPy restatement of the reference algorithm (oracle/anm_oracle.py,
                  literal scipy.sparse + spsolve path) timed on one host core for a bounded sample.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# Host wait mode: completion signals polled instead of interrupt-driven (a ROCm runtime setting, read when the runtime
# starts -- hence before torch is imported; an explicit setting of the caller wins).  It shortens the host's wake-up behind
# the closing synchronize of a timed window, which a 20-step window of 75 us steps feels (measured on MI355X, 20 steps, 5
# warm-up: 0.0816-0.0825 -> 0.0798-0.0808 ms per step; profiles/r06_w_sync_latency.txt); nothing on the device changes.
os.environ.setdefault("HSA_ENABLE_INTERRUPT", "0")

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md


def algorithmic_bytes_per_env_step(A, O, n_des, K):
    """read action (8A), read+write soc and aux (16(n_des+K)), write obs (8O),
    write reward+e_loss+penalty (24), read+write terminated (2)."""
    return 8 * (A + O + 2 * (n_des + K) + 3) + 2


def cpu_baseline(budget_s=12.0, all_cores=True):
    """Reference algorithm on the host: per-environment NumPy/SciPy restatement (the oracle), same
    workload (ANM6Easy, uniform random actions, reset on collapse): one core in-process for a bounded
    sample, then one process per host core (independent environments) for a second bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_bench

    n, dt, _ = cpu_bench.run(budget_s, seed=0)
    out = {
        "value": n / dt, "unit": "env-steps/s", "cores": 1, "kind": "port",
        "sample": "%d sequential ANM6Easy env-steps (%.1f s) of oracle/anm_oracle.py, scipy.sparse Jacobian + spsolve "
                  "exactly as the reference, exact polygon projection instead of cvxpy/OSQP, tol 1e-5; host has %d cores"
                  % (n, dt, os.cpu_count()),
    }  # fmt: skip
    if all_cores:
        try:
            tot, slow, n_proc, wall, eff = cpu_bench.run_all_cores(max(4.0, budget_s * 0.6))
            out["all_cores"] = {"value": tot / slow, "unit": "env-steps/s", "cores": n_proc,
                                "effective_cores": round(eff, 1),
                                "sample": "%d env-steps over %d independent processes (one per usable core), %.1f s "
                                          "each (wall %.1f s incl. interpreter start-up); effective_cores = CPU time "
                                          "the processes received / wall" % (tot, n_proc, slow, wall)}  # fmt: skip
        except Exception as ex:  # the 1-core figure is the contract; never lose the line over this
            out["all_cores"] = {"error": str(ex)[:200]}
        # upper bound for a compiled CPU port: the kernel templates built for the host (g++ -O2), SURVEY 8(d)
        try:
            n2, dt2, _ = cpu_bench.run_cpp(3.0)
            tot, slow, n_proc, wall, eff = cpu_bench.run_all_cores(4.0, impl="cpp")
            out["cpp_port"] = {"value": n2 / dt2, "unit": "env-steps/s", "cores": 1, "kind": "port",
                               "all_cores": {"value": tot / slow, "cores": n_proc, "effective_cores": round(eff, 1)},
                               "sample": "tests/hostsim (the HIP kernel templates compiled with g++ -O2), 2048 "
                                         "environments per step, %d env-steps in %.1f s on one core; then one process "
                                         "per usable core for 4 s" % (n2, dt2)}  # fmt: skip
        except Exception as ex:
            out["cpp_port"] = {"error": str(ex)[:200]}
    return out


def live_pmc(args, kernel="k_step_rows", timeout_s=150):
    """HBM bytes and VALU instructions per launch of the headline kernel from the PMC counters, collected NOW: this
    process spawns `rocprofv3 --kernel-trace --pmc <one counter group>` around a short headline-only run of this very
    script and configuration -- separate passes, as /opt/skills/guides/MI355X_MICROARCH.md prescribes (FETCH_SIZE,
    WRITE_SIZE in KiB; FETCH_SIZE doubled: the gfx950 correction for coalesced reads) -- and averages the kernel's rows.
    Returns None when rocprofv3 is missing or a pass fails (the committed figure of an earlier run is attached then)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None:
        return None
    base = [sys.executable, os.path.abspath(__file__), "--headline-only", "--no-cpu-baseline", "--no-live-pmc", "--steps", "24", "--warmup", "6",
            "--num-envs", str(args.num_envs), "--tol", repr(args.tol), "--max-iter", str(args.max_iter), "--precision", args.precision]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = {}
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        for name, counters in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("valu", ["SQ_INSTS_VALU", "SQ_WAVES"])):
            d = os.path.join(td, name)
            try:
                subprocess.run([rocprof, "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", d, "--"] + base,
                               cwd="/tmp", env=env, capture_output=True, timeout=timeout_s, check=True)
                f = glob.glob(os.path.join(d, "*", "*_counter_collection.csv"))[0]
            except Exception:
                return None
            acc = {}
            for r in csv.DictReader(open(f)):
                if kernel in r["Kernel_Name"]:
                    acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
            if not all(c in acc and acc[c] for c in counters):
                return None
            for c in counters:
                out[c] = sum(acc[c]) / len(acc[c])
            out["launches_" + name] = len(acc[counters[0]])
    fetch_b, write_b = out["FETCH_SIZE"] * 1024.0, out["WRITE_SIZE"] * 1024.0
    return {"hbm_bytes_per_launch": 2.0 * fetch_b + write_b, "fetch_bytes_raw": fetch_b, "write_bytes_raw": write_b,
            "valu_wave_insts_per_launch": out["SQ_INSTS_VALU"], "waves_per_launch": out["SQ_WAVES"],
            "launches_averaged": out["launches_fetch"]}


def transition_figure(dev, net, E, cap, n, load_scale=1.0, note=""):
    """Simulator.transition launches on a fixed batch of random inputs (the SoC is restored before every launch so that
    each launch does the same work), with the HBM roofline of the launch"""
    from gym_anm_amd.simulator import BatchedSimulator

    sim = BatchedSimulator(net, 0.25, 100, num_envs=E, device=dev, tol=1e-6, max_iter=cap)
    m, b = sim.model, sim.model.baseMVA
    g = torch.Generator(device=dev).manual_seed(0)

    def U(lo, hi, scale=1.0):
        lo, hi = torch.as_tensor(lo, device=dev) * scale, torch.as_tensor(hi, device=dev) * scale
        return lo + (hi - lo) * torch.rand((E, lo.numel()), generator=g, dtype=torch.float64, device=dev)

    pl = U(m.dev_p_min[m.load_idx] * b, 0 * m.dev_p_min[m.load_idx], load_scale)
    pp = U(0 * m.dev_p_max[m.gen_idx], m.dev_p_max[m.gen_idx] * b)
    ps = U(m.dev_p_min[m.setp_idx] * b, m.dev_p_max[m.setp_idx] * b, load_scale)
    qs = U(m.dev_q_min[m.setp_idx] * b, m.dev_q_max[m.setp_idx] * b, load_scale)
    soc = U(m.dev_soc_min[m.des_idx], m.dev_soc_max[m.des_idx])
    if load_scale != 1.0:
        pl[-max(1, E // 1024):] *= 40.0 / load_scale   # the diverging solves a large batch always holds
    for _ in range(3):
        sim.soc.copy_(soc)
        sim.transition(pl, pp, ps, qs)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        sim.soc.copy_(soc)
        sim.transition(pl, pp, ps, qs)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / n
    # HBM roofline of this launch (Simulator.transition with the electrical-state dump): compulsory bytes per
    # transition = inputs (P_load, P_pot, P/Q set-points) + SoC in/out + dump + reward/e_loss/penalty +
    # converged + nr_iters
    nbytes = 8 * (m.N_load + m.N_non_slack_gen + 2 * len(m.setp_idx)) + 16 * m.N_des + 8 * sim.full_dim + 24 + 1 + 4
    return {
        "env_steps_per_s": E / dt, "us_per_launch": dt * 1e6, "impl": sim.impl, "lanes_per_env": sim.lanes_per_env,
        "converged_frac": float(sim.pfe_converged.double().mean()),
        "roofline": {"bound": "hbm", "algorithmic_bytes_per_transition": nbytes, "achieved": nbytes * E / dt / 1e9,
                     "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": nbytes * E / dt / 1e9 / HBM_PEAK_GBPS,
                     "note": "wall clock per launch incl. the SoC restore copy; lane-group kernel, fp64" + note},
    }


def case30_side_figure(dev, E=16384, n=20):
    """BASELINE.json config 4: the synthetic random radial 30-bus feeder (seed 0), 16 384 transitions per launch, the
    reference's cap and a cap of 20.  Every rank measures it on its own GPU (main reduces: sum of rates, slowest launch)."""
    from gym_anm_amd import networks

    out = {}
    for cap in (100, 20):
        out["case30_radial_16384_cap%d" % cap] = transition_figure(dev, networks.synthetic_radial_network(30, 0), E, cap, n)
    return out


def case30_envstep_figure(dev, args, E=16384, n=100):
    """BASELINE.json config 4 on the metric's own terms (VERDICT r5 #1b): env-steps of `BatchedANMEnv.step` over the synthetic
    30-bus radial feeder -- a series-mode task (daily tables for its loads and generators), the "state" observation, uniform
    random actions in the action Box, in-kernel autoreset -- one launch of the tree kernel per step, with SURVEY 8(d)'s
    algorithmic bytes per env-step: 8 (A + O + 2 (n_des + K) + 3) + 2 = 658 B for this feeder (A = 16, O = 51, n_des = 5,
    K = 1).  The reference's cap (100) and a cap of 20."""
    import numpy as np

    from gym_anm_amd import networks
    from gym_anm_amd.envs import BatchedANMEnv
    from gym_anm_amd.model import NetworkModel

    net = networks.synthetic_radial_network(30, 0)
    m = NetworkModel(net, 0.25, 100)
    period = 96
    r, t = np.random.default_rng(3), np.arange(period) / period
    rows = [m.dev_p_min[k] * m.baseMVA * (0.25 + 0.3 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.load_idx]
    rows += [m.dev_p_max[k] * m.baseMVA * (0.1 + 0.45 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.gen_idx]
    series = np.array(rows)
    out = {}
    for cap in (100, 20):
        env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, period - 1]]), costs_clipping=(1, 100), seed=11,
                            num_envs=E, device=dev, tol=args.tol, max_iter=cap, autoreset=True, series=series)
        env.check_actions = False
        env.reset(seed=11, options={"sampler": "device"})
        gen = torch.Generator(device=dev).manual_seed(23)
        lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
        A = int(lo.numel())
        pool = [lo + (hi - lo) * torch.rand((E, A), generator=gen, dtype=torch.float64, device=dev) for _ in range(8)]
        wall, evs = _timed_env_steps(env, pool, n, dev)
        nbytes = algorithmic_bytes_per_env_step(A, env.state_N, m.N_des, 1)
        term = float(env.terminated.double().mean())
        out["case30_envstep_16384" + ("" if cap == 100 else "_cap%d" % cap)] = {
            "env_steps_per_s": E / wall, "us_per_step": wall * 1e6, "us_per_step_events": evs * 1e6, "impl": env.simulator.impl,
            "lanes_per_env": env.simulator.lanes_per_env, "nr_tol": args.tol, "nr_max_iter": cap,
            "mean_nr_iters": float(env.simulator.nr_iters.double().mean()), "collapsed_per_step": term,
            "roofline": {"bound": "hbm", "achieved": nbytes * E / evs / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": nbytes * E / evs / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_env_step": nbytes,
                         "note": "k_radial (mode: step), one launch per step; HIP events over %d steps; SURVEY 8(d)'s formula with "
                                 "A = %d, O = %d, n_des = %d, K = 1" % (n, A, env.state_N, m.N_des)}}
        del env
    return out


def mesh_side_figure(dev, E=16384, n=20):
    """the general lane-group family: a meshed 30-bus network inside a wavefront, a meshed 200-bus network as one
    workgroup of 256 lanes per environment (loads scaled with 40 / n_bus: the synthetic feeders carry the same load
    per bus whatever their size)"""
    from gym_anm_amd import networks

    out = {}
    out["mesh30_16384_cap100"] = transition_figure(dev, networks.synthetic_meshed_network(30, 6, 4), E, 100, n,
                                                   note="; LDS-bound (block-sparse Jacobian in LDS), see DESIGN.md")
    out["mesh200_4096_cap100"] = transition_figure(dev, networks.synthetic_meshed_network(200, 13, 30), 4096, 100, max(4, n // 4), 40.0 / 200,
                                                   note="; one workgroup of 256 lanes per environment, see DESIGN.md")
    return out


def _timed_env_steps(env, pool, n, dev):
    for i in range(10):
        env.step(pool[i % len(pool)])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ev0.record()
    for i in range(n):
        env.step(pool[i % len(pool)])
    ev1.record()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / n, ev0.elapsed_time(ev1) * 1e-3 / n


def baseline_configs_side_figure(dev, args, n=100):
    """The BASELINE.json configurations the headline does not cover, each as a timed line of this run:
    config 2 -- ANM6Easy, 4 096 environments, fp64 (one wavefront on one SIMD in sixteen: a latency figure);
    config 3 -- ANM6Easy, 65 536 environments with the Jacobian + LU in fp32 (mismatch, stop test and update stay fp64),
    timed like the headline, plus the tolerance report: the same 65 536 seeded transitions through the fp64 and the fp32
    solve -- largest deviation of |V|, theta and the branch flows, flag mismatches, iteration histograms."""
    from gym_anm_amd import networks
    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.simulator import BatchedSimulator

    out = {}
    nbytes = algorithmic_bytes_per_env_step(6, 18, 1, 1)
    for key, E, prec in (("anm6easy_4096", 4096, "f64"), ("anm6easy_65536_f32", 65536, "f32")):
        env = ANM6EasyVec(num_envs=E, device=dev, seed=4321, tol=args.tol, max_iter=args.max_iter, precision=prec, autoreset=True)
        env.check_actions = False
        env.reset(seed=4321)
        gen = torch.Generator(device=dev).manual_seed(17)
        lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
        pool = [lo + (hi - lo) * torch.rand((E, 6), generator=gen, dtype=torch.float64, device=dev) for _ in range(8)]
        wall, evs = _timed_env_steps(env, pool, n, dev)
        out[key] = {"env_steps_per_s": E / wall, "us_per_step": wall * 1e6, "us_per_step_events": evs * 1e6,
                    "dtype": "f64" if prec == "f64" else "f64 (f32 Jacobian/LU)", "nr_tol": args.tol, "nr_max_iter": args.max_iter,
                    "roofline": {"bound": "hbm", "achieved": nbytes * E / evs / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                 "frac": nbytes * E / evs / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_env_step": nbytes}}
        del env
    # tolerance report of config 3 (Simulator.transition with the electrical-state dump, same inputs, both precisions)
    E = 65536
    res = {}
    for prec in ("f64", "f32"):
        sim = BatchedSimulator(networks.anm6_network(), 0.25, 100, num_envs=E, device=dev, tol=args.tol, max_iter=args.max_iter,
                               precision=prec)
        m, b = sim.model, sim.model.baseMVA
        g = torch.Generator(device=dev).manual_seed(0)

        def U(lo, hi):
            lo, hi = torch.as_tensor(lo, device=dev), torch.as_tensor(hi, device=dev)
            return lo + (hi - lo) * torch.rand((E, lo.numel()), generator=g, dtype=torch.float64, device=dev)

        pl = U(m.dev_p_min[m.load_idx] * b, 0 * m.dev_p_min[m.load_idx])
        pp = U(0 * m.dev_p_max[m.gen_idx], m.dev_p_max[m.gen_idx] * b)
        ps = U(m.dev_p_min[m.setp_idx] * b, m.dev_p_max[m.setp_idx] * b)
        qs = U(m.dev_q_min[m.setp_idx] * b, m.dev_q_max[m.setp_idx] * b)
        sim.soc.copy_(U(m.dev_soc_min[m.des_idx], m.dev_soc_max[m.des_idx]))
        st, _, _, _, conv = sim.transition(pl, pp, ps, qs)
        res[prec] = {"vm": st.tensor("bus_v_magn", "pu").clone(), "va": st.tensor("bus_v_ang", "rad").clone(),
                     "bp": st.tensor("branch_p", "pu").clone(), "bq": st.tensor("branch_q", "pu").clone(),
                     "bs": st.tensor("branch_s", "pu").clone(), "conv": conv.clone(), "it": sim.nr_iters.clone()}
        del sim
    a, c = res["f64"], res["f32"]
    both = a["conv"] & c["conv"]

    def hist(t):
        v, n_ = torch.unique(t[both], return_counts=True)
        return {str(int(k)): int(x) for k, x in zip(v.tolist(), n_.tolist())}

    out["anm6easy_65536_f32"]["tolerance_report"] = {
        "transitions": E, "converged_f64": int(a["conv"].sum()), "converged_f32": int(c["conv"].sum()),
        "flag_mismatches": int((a["conv"] != c["conv"]).sum()),
        "max_abs_dV_pu": float((a["vm"] - c["vm"]).abs()[both].max()), "max_abs_dtheta_rad": float((a["va"] - c["va"]).abs()[both].max()),
        "max_abs_dbranch_p_pu": float((a["bp"] - c["bp"]).abs()[both].max()), "max_abs_dbranch_q_pu": float((a["bq"] - c["bq"]).abs()[both].max()),
        "max_abs_dbranch_s_pu": float((a["bs"] - c["bs"]).abs()[both].max()),
        "nr_iters_hist_f64": hist(a["it"]), "nr_iters_hist_f32": hist(c["it"]),
        "note": "same seeded inputs through Simulator.transition with the Jacobian + LU in fp64 and in fp32; deviations over the "
                "transitions both solves converged on; BASELINE asks for 1e-6 p.u. against the reference"}
    return out


def throughput_side_figure(dev, args, E=524288, n=60):
    """BASELINE config 5's per-GPU load when 524 288 environments sit on ONE GPU (the strong-scaling N = 1 point):
    the two-launch step (stragglers of the whole batch packed into a second launch), same workload as the headline."""
    from gym_anm_amd.envs import ANM6EasyVec

    env = ANM6EasyVec(num_envs=E, device=dev, seed=77, tol=args.tol, max_iter=args.max_iter, precision=args.precision,
                      autoreset=True)  # fmt: skip
    env.check_actions = False
    env.reset(seed=77)
    gen = torch.Generator(device=dev).manual_seed(5)
    lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
    pool = [lo + (hi - lo) * torch.rand((E, 6), generator=gen, dtype=torch.float64, device=dev) for _ in range(4)]
    for i in range(10):
        env.step(pool[i % 4])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ev0.record()
    for i in range(n):
        env.step(pool[i % 4])
    ev1.record()
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / n
    kern = ev0.elapsed_time(ev1) * 1e-3 / n
    nbytes = algorithmic_bytes_per_env_step(6, 18, 1, 1)
    return {"anm6easy_524288_1gpu": {
        "env_steps_per_s": E / wall, "us_per_step": wall * 1e6, "us_per_step_events": kern * 1e6,
        "launches_per_step": 3 if env._ws is not None else 1,
        "roofline": {"bound": "hbm", "achieved": nbytes * E / kern / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": nbytes * E / kern / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_env_step": nbytes,
                     "note": "k_step_rows + k_step_stragglers + k_step_scatter per step; HIP events over %d steps" % n}}}


def mixed_side_figure(dev, E=16384, n=40):
    """Environments over DIFFERENT networks in one batch (gym_anm/envs/anm_env.py:79-156 builds one ANMEnv per network):
    ANM6Easy, the 3-bus loop, a meshed 20-bus network and config 4's 30-bus feeder dealt at random to 16 384 environments,
    series-mode tasks with autoreset, random agent; one launch per topology, each in its own kernel family, on its own
    stream (MixedBatchedANMEnv) -- and the same launches one after the other on one stream."""
    import numpy as np

    from gym_anm_amd import networks
    from gym_anm_amd.envs import MixedBatchedANMEnv
    from gym_anm_amd.envs.anm6 import anm6easy_series
    from gym_anm_amd.model import NetworkModel

    def table(net, period, seed):
        m = NetworkModel(net, 0.25, 100)
        r, t = np.random.default_rng(seed), np.arange(period) / period
        rows = [m.dev_p_min[k] * m.baseMVA * (0.25 + 0.3 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.load_idx]
        rows += [m.dev_p_max[k] * m.baseMVA * (0.1 + 0.45 * (1 + np.sin(2 * np.pi * (t + r.uniform())))) for k in m.gen_idx]
        return np.array(rows)

    nets = [networks.anm6_network(), networks.three_bus_loop_network(gen_max=1.5), networks.synthetic_meshed_network(20, 3, 6),
            networks.synthetic_radial_network(30, 0)]
    series = [anm6easy_series(), table(nets[1], 24, 1), table(nets[2], 48, 2), table(nets[3], 96, 3)]
    tasks = [dict(network=nw, series=s, delta_t=dt, costs_clipping=(1, 100)) for nw, s, dt in zip(nets, series, (0.25, 0.5, 0.25, 0.25))]
    env_task = np.random.default_rng(5).integers(0, 4, E)
    out = {}
    for streams in (True, False):
        env = MixedBatchedANMEnv(tasks, env_task, device=dev, seed=7, tol=1e-6, max_iter=100, autoreset=True, streams=streams)
        env.check_actions = False
        env.reset(seed=7)
        g = torch.Generator(device=dev).manual_seed(1)
        lo, hi = torch.as_tensor(env.action_space.low, device=dev), torch.as_tensor(env.action_space.high, device=dev)
        pool = [lo + (hi - lo) * torch.rand((E, env.A), generator=g, dtype=torch.float64, device=dev) for _ in range(4)]
        wall, evs = _timed_env_steps(env, pool, n, dev)
        out["streams" if streams else "one_stream"] = {"us_per_step": wall * 1e6, "us_per_step_events": evs * 1e6, "env_steps_per_s": E / wall}
    out["families"] = dict(zip(("anm6", "3bus_loop", "mesh20", "case30"), env.impls))
    out["envs_per_network"] = [int((env_task == k).sum()) for k in range(4)]
    return {"mixed_topologies_16384": out}


def mpc_side_figure(dev):
    """the batched MPC DC-OPF policy (gym_anm/agents/mpc.py), all environments' programs in one launch of
    k_mpc.  Algorithmic bytes per program: forecasts in, first-stage set-points + value + iteration count out."""
    from gym_anm_amd.agents import MPCAgentPerfect
    from gym_anm_amd.envs import ANM6EasyVec

    out = {}
    E = 65536
    env = ANM6EasyVec(num_envs=E, device=dev, seed=3)
    env.reset(seed=3)
    for N in (1, 10):
        ag = MPCAgentPerfect(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N)
        pl, pg = ag.forecast(env)
        soc = ag._soc(env)
        sol = ag.solver
        for _ in range(3):
            sol.solve(pl, pg, soc)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        ev0.record()
        for _ in range(10):
            sol.solve(pl, pg, soc)
        ev1.record()
        torch.cuda.synchronize(dev)
        ms = ev0.elapsed_time(ev1) / 10
        # the whole of act() -- forecast gather, solve, scaling to MW, clipping -- as the caller sees it: ONE launch
        # (anm_mpc_act_f64), wall clock per call
        ag.warn_unconverged = False
        ag.reuse_action_buffer = True   # (the zero-allocation form: act() hands out the solver's own action buffer)
        for _ in range(3):
            ag.act(env)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            ag.act(env)
        torch.cuda.synchronize(dev)
        act_ms = (time.perf_counter() - t0) / 20 * 1e3
        d = sol.dims
        nbytes = 8 * (N * (d.n_load + d.n_gen) + d.n_des + d.n_ctrl + 1 + 3) + 4
        out["mpc_dcopf_anm6_65536_N%d" % N] = {
            "programs_per_s": E / (ms * 1e-3), "ms_per_solve": ms, "mpc_act_ms_wall": act_ms, "act_is_one_launch": bool(ag._fused(env)),
            "mean_iterations": float(sol.iters.double().mean()),
            "max_iterations": int(sol.iters.max()), "rows_per_stage": int(d.n_stage_rows), "angle_rows_carried": bool(d.angle_rows),
            "roofline": {"bound": "hbm", "achieved": nbytes * E / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": nbytes * E / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_program": nbytes,
                         "note": "an interior-point solve per program: fp64-issue bound by nature (~%d iterations of a few "
                                 "thousand instructions per lane), the HBM figure is the contract's" % round(float(sol.iters.double().mean()))}}
    return out


# --------------------------------------------------------------------------------------------
# Ranks.  One process per GPU; the environment batch is sharded contiguously, no data-path collective.
# `python bench.py --gpus N` starts its own ranks (torch.distributed.run) when it was not started by a launcher;
# everything about ranks that does not need a GPU is in the functions below so that the CPU tier can drive it with
# two gloo ranks (tests/test_bench_launcher.py).
# --------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--num-envs", type=int, default=65536, help="environments per GPU (weak scaling: the default)")
    ap.add_argument("--global-envs", type=int, default=0,
                    help="strong scaling: this many environments in total, split evenly over the GPUs (BASELINE config 5: "
                         "524288); overrides --num-envs")
    ap.add_argument("--tol", type=float, default=1e-6, help="Newton stop: ||F||inf <= tol (metric: 1e-6; reference: 1e-5)")
    ap.add_argument("--max-iter", type=int, default=100, help="Newton iteration cap (reference: 100)")
    ap.add_argument("--precision", choices=["f64", "f32"], default="f64", help="Jacobian/LU precision (F, x always fp64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--no-live-pmc", action="store_true", help="do not spawn the rocprofv3 counter passes (roofline.traffic then "
                    "carries the committed figure of an earlier run)")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: skip the secondary figures (cap-20, case30) so that a rocprofv3 trace of this "
                         "command holds only launches of the headline configuration")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the kernel timed from C, PMC passes, "
                         "workload statistics, secondary figures, other configurations, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (obs, reward, terminated, truncated) as DIR/<name>.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1: ms_per_step and --dump-outputs come from the timed steps")
    return args


def rank_info(environ=None):
    """(rank, local_rank, world, launched): what torch.distributed.run put in the environment (launched = it did)."""
    env = os.environ if environ is None else environ
    return (int(env.get("RANK", "0")), int(env.get("LOCAL_RANK", "0")), int(env.get("WORLD_SIZE", "1")),
            "RANK" in env and "WORLD_SIZE" in env)


def free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch_command(n, script, argv):
    """`python bench.py --gpus N ...` typed without a launcher: the same command under torch.distributed.run, one rank
    per GPU of this node, rendezvous on 127.0.0.1 (what the driver's own multi-GPU command line looks like)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
            "127.0.0.1", "--master-port", str(free_port()), script] + list(argv)


def self_launch(n, script=None, argv=None):
    import subprocess

    cmd = self_launch_command(n, os.path.abspath(script or sys.argv[0]), sys.argv[1:] if argv is None else argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL on this pool: dmabuf IPC only
    return subprocess.call(cmd, env=env)


def preflight_devices(n, visible):
    """`--gpus n` against the devices this process can see: None when it fits, else the one line to exit with BEFORE any rank
    is spawned (a rank that cannot set its device would leave the others waiting in the rendezvous)"""
    if n <= visible:
        return None
    return ("bench.py: --gpus %d but only %d GPU%s visible here (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES narrow the set): "
            "nothing started" % (n, visible, " is" if visible == 1 else "s are"))


def rendezvous_timeout_s():
    """how long a rank waits for the others in init_process_group before it gives up with a message instead of hanging
    (ANM_BENCH_RDZV_TIMEOUT seconds; default 180: a fresh box can take two minutes over its first `import torch`)"""
    try:
        return max(1.0, float(os.environ.get("ANM_BENCH_RDZV_TIMEOUT", "180")))
    except ValueError:
        return 180.0


def shard(args, world, rank):
    """environments of this rank, global index of its first one, scaling mode"""
    if args.global_envs:
        if args.global_envs % world:
            raise SystemExit("--global-envs %d is not a multiple of the %d ranks" % (args.global_envs, world))
        per = args.global_envs // world
        return per, rank * per, "strong"
    return args.num_envs, rank * args.num_envs, "weak"


class Comm:
    """The reporting collectives (nothing else crosses ranks): barrier, MAX and SUM of a few scalars."""

    def __init__(self, backend, rank, world, device, launched):
        self.dist, self.rank, self.world, self.device, self.ranks_seen = None, rank, world, device, None
        if world > 1 or launched:
            import torch.distributed as dist

            import datetime

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            kw = {"device_id": device} if device.type == "cuda" else {}
            t_out = rendezvous_timeout_s()
            try:
                dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=t_out), **kw)
            except Exception as ex:  # a peer that never arrived (it could not set its device, or was never started)
                raise SystemExit("bench.py rank %d/%d: the rendezvous on %s:%s did not complete within %.0f s (%s: %s) -- a peer "
                                 "rank is missing; nothing was measured" % (rank, world, os.environ.get("MASTER_ADDR"),
                                                                            os.environ.get("MASTER_PORT"), t_out, type(ex).__name__, str(ex)[:200]))
            self.dist = dist
            # the communicator really spans `world` ranks: one all-reduce of ones must come back as the world size
            self.ranks_seen = int(round(self.reduce([1.0], "sum")[0]))
            if self.ranks_seen != world or dist.get_world_size() != world:
                raise SystemExit("the communicator sees %d ranks (get_world_size %d), expected %d"
                                 % (self.ranks_seen, dist.get_world_size(), world))

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def reduce(self, values, op):
        """element-wise SUM / MAX over the ranks of a short list of floats (the same list on every rank afterwards)"""
        if self.dist is None:
            return [float(v) for v in values]
        t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM if op == "sum" else self.dist.ReduceOp.MAX)
        return [float(v) for v in t.tolist()]

    def close(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()


def reduce_side_figure(comm, fig):
    """A per-rank side figure {name: {"env_steps_per_s", "us_per_launch", ...}} measured by EVERY rank on its own GPU
    -> the job's figure: rates summed, launch times the slowest rank's; the rank-0 entry keeps its other fields."""
    names = sorted(fig)
    rates = comm.reduce([fig[k]["env_steps_per_s"] for k in names], "sum")
    slow = comm.reduce([fig[k]["us_per_launch"] for k in names], "max")
    out = {}
    for k, r, u in zip(names, rates, slow):
        out[k] = dict(fig[k])
        out[k]["env_steps_per_s"] = r
        out[k]["us_per_launch"] = u
        out[k]["ranks"] = comm.world
        if comm.world > 1 and "roofline" in out[k]:
            rl = dict(out[k]["roofline"])
            rl["note"] = rl.get("note", "") + "; roofline of rank 0's GPU, env_steps_per_s summed over the ranks, us_per_launch the slowest rank's"
            out[k]["roofline"] = rl
    return out


def default_make_env(num_envs, device, args, env_offset, seed):
    from gym_anm_amd.envs import ANM6EasyVec

    return ANM6EasyVec(num_envs=num_envs, device=device, seed=seed, tol=args.tol, max_iter=args.max_iter,
                       precision=args.precision, autoreset=True, env_offset=env_offset)  # fmt: skip


DUMP_LIMIT_BYTES = 64 * 2**20


def dump_outputs(directory, result, rank=0, world=1, limit=DUMP_LIMIT_BYTES):
    """`env.step`'s return of the last timed step -- obs, reward, terminated, truncated -- as <directory>/<name>.npy in
    float64 (flags as 0 / 1), this rank's shard (file names carry the rank when there are several).  Above `limit` bytes
    in all, a fixed seeded sample of environments is written instead, with their indices as rows.npy."""
    import numpy as np

    obs, rew, term, trunc, _ = result
    arrays = {"obs": obs, "reward": rew, "terminated": term, "truncated": trunc}
    arrays = {k: v.detach().to("cpu", torch.float64).numpy() for k, v in arrays.items()}
    n = len(arrays["reward"])
    row_bytes = sum(a[0].nbytes if a.ndim > 1 else 8 for a in arrays.values())
    if n * row_bytes > limit:
        rows = np.sort(np.random.default_rng(0).choice(n, size=limit // (row_bytes + 8), replace=False))
        arrays = {k: v[rows] for k, v in arrays.items()}
        arrays["rows"] = rows.astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    suffix = "" if world == 1 else "_rank%d" % rank
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + suffix + ".npy"), np.ascontiguousarray(a))


def main(argv=None, make_env=None, backend="nccl", device_type="cuda", script=None):
    """make_env / backend / device_type: the CPU tier's launcher test passes the host test double, "gloo" and "cpu";
    the benchmark itself never does (no flag selects them)."""
    args = parse_args(argv)
    rank, local_rank, world, launched = rank_info()
    gpu = device_type == "cuda"
    if not launched and args.gpus > 1:
        # typed as `python bench.py --gpus N`: start one rank per GPU and let rank 0 print the line
        if gpu:
            msg = preflight_devices(args.gpus, torch.cuda.device_count() if torch.cuda.is_available() else 0)
            if msg:
                raise SystemExit(msg)
        raise SystemExit(self_launch(args.gpus, script, argv))
    if world != args.gpus:
        args.gpus = world
    if gpu and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the simulator has no CPU path")
    if gpu:
        # a rank without a device of its own leaves with one line; its peers then time out of the rendezvous (Comm) instead
        # of waiting for it for ever (under torch.distributed.run the agent ends them at once)
        n_vis = torch.cuda.device_count()
        if local_rank >= n_vis:
            raise SystemExit("bench.py rank %d: LOCAL_RANK %d but %d GPU%s visible to this process; this rank leaves before the "
                             "rendezvous" % (rank, local_rank, n_vis, " is" if n_vis == 1 else "s are"))
        try:
            torch.cuda.set_device(local_rank)
        except Exception as ex:
            raise SystemExit("bench.py rank %d: torch.cuda.set_device(%d) failed (%s); this rank leaves before the rendezvous"
                             % (rank, local_rank, str(ex)[:200]))
    dev = torch.device("cuda", local_rank) if gpu else torch.device("cpu")
    comm = Comm(backend, rank, world, dev, launched)
    rccl_ranks = comm.ranks_seen

    E, env_offset, scaling = shard(args, world, rank)
    env = (make_env or default_make_env)(E, dev, args, env_offset, 1234)
    env.check_actions = False  # the Box check is a device reduction + host sync; actions are in the Box by construction
    env.reset(seed=1234 + rank)
    gen = torch.Generator(device=dev).manual_seed(99 + rank)
    lo = torch.as_tensor(env.action_space.low, device=dev)
    hi = torch.as_tensor(env.action_space.high, device=dev)
    n_pool = 16
    pool = [lo + (hi - lo) * torch.rand((E, 6), generator=gen, dtype=torch.float64, device=dev) for _ in range(n_pool)]

    for i in range(args.warmup):
        env.step(pool[i % n_pool])
    iters_sum = torch.zeros((), dtype=torch.float64, device=dev)
    term_sum = torch.zeros((), dtype=torch.float64, device=dev)
    if gpu:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    comm.barrier()
    t0 = time.perf_counter()
    if gpu:
        ev0.record()  # torch's current stream == the stream every step kernel is launched on (_step_call)
    for i in range(args.steps):
        result = env.step(pool[i % n_pool])
    if gpu:
        ev1.record()
    comm.barrier()
    elapsed = time.perf_counter() - t0
    # HIP events over the timed region: kernel + launch gap
    step_events_s = ev0.elapsed_time(ev1) * 1e-3 / args.steps if gpu else elapsed / args.steps
    if args.dump_outputs:  # before any further step overwrites the buffers the last one returned
        dump_outputs(args.dump_outputs, result, rank, world)
    # statistics of the workload (outside the timed region)
    if args.full:
        for i in range(8):
            env.step(pool[i % n_pool])
            iters_sum += env.simulator.nr_iters.double().mean()
            term_sum += env.terminated.double().mean()
    elapsed = comm.reduce([elapsed], "max")[0]                       # the slowest rank's clock
    total_steps = comm.reduce([float(E * args.steps)], "sum")[0]     # the units all ranks processed

    sim = env.simulator
    kernel_s = step_events_s
    n_launch = args.steps
    if gpu and args.full:
        # cross-check: the same launch issued back to back from C (no Python between launches), HIP events
        # on the launch stream; one fixed action batch
        import ctypes as C

        ms = C.c_float(0.0)
        n_launch = max(50, min(args.steps, 400))
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = sim.backend.lib.anm_time_step_launches(
                sim._handle, E, pool[0].data_ptr(), sim.soc.data_ptr(), env._state_buf.data_ptr(), env._term_u8.data_ptr(),
                env.timestep.data_ptr(), env._state_obs.data_ptr(), env.reward.data_ptr(), env.e_loss.data_ptr(),
                env.penalty.data_ptr(), 1, env.rng_seed, env.env_offset, env._reset_count.data_ptr(), env._aux_index_ptr,
                env._ws_ref, C.byref(sim.opts), stream,
                n_launch, C.byref(ms),
            )  # fmt: skip
        sim.backend.check(rc, "anm_time_step_launches")
        # the kernel's own duration: launches issued back to back from C, HIP events on the launch stream around them
        # (nothing between two launches; agrees with the rocprofv3 kernel-trace average, profiles/).  The events over the
        # timed region above additionally hold the gap the Python caller leaves between two launches.
        kernel_s = ms.value * 1e-3

    def timed_steps(n):
        for i in range(10):
            env.step(pool[i % n_pool])
        if gpu:
            torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(n):
            env.step(pool[i % n_pool])
        if gpu:
            torch.cuda.synchronize(dev)
        return time.perf_counter() - t1

    # secondary figure: same workload with a 20-iteration cap.  Diverging solves (the only ones that
    # ever exceed ~8 iterations) are then cut off early; on every sample tested the terminated flags
    # are identical to the reference's cap of 100, but that is an observation, not a proof, so the
    # headline `value` above keeps the reference's cap.
    side = args.full and not args.headline_only
    alt = None
    if rank == 0 and args.max_iter == 100 and side:
        sim.opts.max_iter = 20
        alt_elapsed = timed_steps(args.steps)
        alt = {"nr_max_iter": 20, "value_1gpu": E * args.steps / alt_elapsed, "ms_per_step": 1e3 * alt_elapsed / args.steps}
        sim.opts.max_iter = args.max_iter

    # the reference's own stop tolerance (simulator.py:529 passes 1e-5) as a second secondary figure
    alt_tol = None
    if rank == 0 and args.tol != 1e-5 and side:
        sim.opts.tol = 1e-5
        dt1 = timed_steps(args.steps)
        alt_tol = {"nr_tol": 1e-5, "nr_max_iter": args.max_iter, "value_1gpu": E * args.steps / dt1,
                   "ms_per_step": 1e3 * dt1 / args.steps, "mean_nr_iters": float(sim.nr_iters.double().mean())}
        sim.opts.tol = args.tol

    # Side figures.  BASELINE.json config 4 (30-bus radial feeder, 16384 transitions per launch, lane-group family) is
    # measured by EVERY rank on its own GPU (north_star: "larger random radial networks at 1/2/4/8 GPUs") and reported
    # as sum of rates / slowest launch like the headline; the others (one-GPU configurations) by rank 0 of a 1-GPU run.
    other = None
    if gpu and side:
        other = {}
        try:
            fig = case30_side_figure(dev)
        except Exception as ex:  # never let a side figure break the headline line (every rank must still reduce)
            fig = {"case30_radial_16384_cap%d" % c: {"env_steps_per_s": 0.0, "us_per_launch": 0.0, "error": str(ex)[:200]}
                   for c in (100, 20)}
        other.update(reduce_side_figure(comm, fig))
        if rank == 0 and world == 1:
            for f in (lambda: case30_envstep_figure(dev, args), lambda: mesh_side_figure(dev), lambda: throughput_side_figure(dev, args),
                      lambda: baseline_configs_side_figure(dev, args), lambda: mixed_side_figure(dev), lambda: mpc_side_figure(dev)):
                try:
                    other.update(f())
                except Exception as ex:
                    other.setdefault("errors", []).append(str(ex)[:200])

    if rank == 0:
        bytes_per = algorithmic_bytes_per_env_step(6, 18, 1, 1)
        achieved = bytes_per * E / kernel_s / 1e9
        # HBM bytes per launch from the PMC passes (scripts/pmc_run.sh -> profiles/pmc_traffic.json):
        # bench.py cannot collect counters itself, so the committed figure is attached when it was
        # measured on this very configuration, else null.
        traffic = None
        traffic_source = None
        valu = None
        if args.full:
            try:
                pt = None
                if gpu and world == 1 and side and not args.no_live_pmc:
                    pt = live_pmc(args)   # counters of THIS configuration on THIS box, collected by this run
                    if pt is not None:
                        pt.update(num_envs=E, nr_max_iter=args.max_iter, precision=args.precision)
                        src = ("live: rocprofv3 --kernel-trace --pmc passes (FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU, one group per pass) "
                               "spawned by this run around a %d-launch headline-only run of the same configuration; FETCH_SIZE %.2f MB x2 "
                               "(gfx950 correction) + WRITE_SIZE %.2f MB" % (pt["launches_averaged"], pt["fetch_bytes_raw"] / 1e6, pt["write_bytes_raw"] / 1e6))
                if pt is None:
                    pt = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
                    src = "profiles/pmc_traffic.json (%s): PMC passes of an earlier run of this configuration, not of this run" % pt.get("source", "?")
                if gpu and pt["num_envs"] == E and pt["nr_max_iter"] == args.max_iter and pt["precision"] == args.precision:
                    traffic = pt["hbm_bytes_per_launch"]
                    traffic_source = src
                    # what really bounds the kernel: fp64 VALU issue.  A wave64 fp64 instruction occupies its
                    # SIMD for 4 cycles, so the chip issues at most 256 CU x 4 SIMD x 2.4 GHz / 4 of them per s.
                    peak_issue = 256 * 4 * 2.4e9 / 4
                    valu = {"wave_instructions_per_launch": pt["valu_wave_insts_per_launch"],
                            "achieved_per_s": pt["valu_wave_insts_per_launch"] / kernel_s, "peak_per_s": peak_issue,
                            "frac": pt["valu_wave_insts_per_launch"] / kernel_s / peak_issue,
                            "note": "chip-wide average; after ~9 iterations only waves holding a diverging solve run"}
            except Exception:
                pass
        out = {
            "metric": "env-steps/sec (whole node) at num_envs=%s, ANM6Easy; NR iters to 1e-6"
                      % ("65536" if (scaling == "weak" and E == 65536) else ("%d in total" % (E * world) if scaling == "strong" else "%d per GPU" % E)),
            "value": total_steps / elapsed,
            "unit": "env-steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": "f64" if args.precision == "f64" else "f64 (f32 Jacobian/LU)",
            "data": "synthetic",
            "config": {
                "workload": "ANM6Easy-v0 (6-bus), num_envs=%d per GPU, uniform random actions in the action Box, "
                            "in-kernel autoreset of collapsed environments" % E,
                "num_envs_per_gpu": E, "global_num_envs": E * world,
                "parallelism": "env-sharded x%d%s" % (world, "" if rccl_ranks is None else ", rccl_ranks=%d" % rccl_ranks),
                "rccl_ranks": rccl_ranks,
                "host_wait": "HSA_ENABLE_INTERRUPT=%s" % os.environ.get("HSA_ENABLE_INTERRUPT", "unset"),
                "straggler_handoff": {"after_iterations": int(sim.opts.handoff_after), "meaning": "Newton iterations a "
                                      "solve spends in its own lane before a still-running one continues on a lane "
                                      "group of the same wavefront (-2: library default, -1: never)"},
                "nr_tol": args.tol, "nr_max_iter": args.max_iter, "nr_start": "flat",
            },
            "roofline": {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_source,
                "kernel": "k_step_rows<double, false>" if args.precision == "f64" else "k_step_rows<float, false>",
                "kernel_ms": kernel_s * 1e3, "launches_timed": n_launch,
                "kernel_ms_source": ("HIP events on the launch stream around %d launches issued back to back from C "
                                     "(anm_time_step_launches), live in this run, rank 0's GPU" % n_launch) if gpu and args.full else
                                    ("HIP events on the launch stream over the %d timed steps (kernel + the caller's gap between "
                                     "launches), rank 0's GPU; --full times launches issued back to back from C" % n_launch),
                "step_ms_hip_events": step_events_s * 1e3, "steps_timed": args.steps,
                "algorithmic_bytes_per_env_step": bytes_per, "valu_fp64_issue": valu,
                "note": "fp64-ALU/latency-bound (Newton-Raphson in registers), not HBM-bound: see DESIGN.md",
            },
        }  # fmt: skip
        if not gpu:
            out["config"]["test_double"] = "host test double (CPU tier launcher test): not a measurement"
        if args.full:
            out["config"]["mean_nr_iters"] = float(iters_sum.item() / 8)
            out["config"]["collapsed_per_step"] = float(term_sum.item() / 8)
            # secondary: algorithmic fp64 flops (per Newton iteration F ~ 8 nnz + 10 n, J ~ 16 nnz + 12 n,
            # dense LU (2/3)(2n)^3 + 2(2n)^2, sincos n; ANM6: n = 5, nnz = 16 -> ~1.4 kflop, plus the final F)
            n_, nnz_ = 5, 16
            per_iter = (8 * nnz_ + 10 * n_) + (16 * nnz_ + 12 * n_) + (2.0 / 3.0) * (2 * n_) ** 3 + 2 * (2 * n_) ** 2 + n_
            flops = per_iter * out["config"]["mean_nr_iters"] + (8 * nnz_ + 10 * n_)
            out["roofline"]["fp64_flops"] = {"algorithmic_per_env_step": flops, "achieved_tflops": flops * E / kernel_s / 1e12,
                                             "peak_tflops": 78.6, "frac": flops * E / kernel_s / 78.6e12}
        if alt is not None:
            out["config"]["alt_iteration_cap"] = alt
        if alt_tol is not None:
            out["config"]["alt_reference_tol"] = alt_tol
        if other is not None:
            out["config"]["other_workloads"] = other
        if gpu and world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cpu_budget)
        print(json.dumps(out), flush=True)
    comm.close()


if __name__ == "__main__":
    main()
