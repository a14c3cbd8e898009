#!/usr/bin/env python
"""What a float32 policy loop costs per step: the float32 I/O mode of the step kernels against a float64 environment with the
three casts such a loop needs without it.

One variant per process, one JSON line per run (HIP events on the launch stream around `--steps` steps after `--warmup`):

  f64    the plain float64 step, fed float64 actions (with `--root ../parent`: the revision before the feature)
  casts  a float64 environment driven by a float32 policy: step(a32.double()), obs.float(), reward.float() -- a dtype-converting
         copy (an allocation and a launch) before the step and two after it
  f32    io_dtype=torch.float32, fed the same float32 actions: the kernels read and write float32 themselves

on `--task anm6` (ANM6Easy, 65 536 environments, the coalesced-row fast path) or `--task feeder` (the 30-bus feeder, 16 384
environments, lane-group kernel, loads and generation drawn in the kernel).  Every variant goes through the public `step()`.
Run the variants ALTERNATED on one card, several rounds, and summarise the lines:

    python scripts/io_f32_bench.py --task anm6 --variant casts --root ../parent --label a >> runs.jsonl
    python scripts/io_f32_bench.py --task anm6 --variant f32 --label b >> runs.jsonl
    python scripts/io_f32_bench.py --task anm6 --variant f64 --root ../parent --label c0 >> runs.jsonl
    python scripts/io_f32_bench.py --task anm6 --variant f64 --label c1 >> runs.jsonl
    ...
    python scripts/io_f32_bench.py --summarise runs.jsonl
"""
import argparse
import json
import os
import statistics
import sys


def summarise(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    groups = {}
    for r in rows:
        groups.setdefault((r["task"], r["label"]), []).extend(r["us_per_step"])
    print("%-8s %-6s %5s %10s %10s %10s   (us per step; every timed run of every round)" % ("task", "label", "runs", "median", "min", "max"))
    for (task, label), v in sorted(groups.items()):
        print("%-8s %-6s %5d %10.2f %10.2f %10.2f" % (task, label, len(v), statistics.median(v), min(v), max(v)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--task", choices=["anm6", "feeder"], default="anm6")
    ap.add_argument("--variant", choices=["f64", "casts", "f32"], default="f64")
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    sys.path.insert(0, os.path.abspath(a.root))

    import numpy as np
    import torch

    from gym_anm_amd import networks
    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.envs.anm_env import BatchedANMEnv

    dev = torch.device("cuda:0")
    kw = dict(io_dtype=torch.float32) if a.variant == "f32" else {}
    if a.task == "anm6":
        E_ = a.envs or 65536
        env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, autoreset=True, **kw)
    else:
        E_ = a.envs or 16384
        env = BatchedANMEnv(networks.synthetic_radial_network(30, 0), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 1e9]]),
                            costs_clipping=(1, 100), seed=7, num_envs=E_, device="cuda:0", tol=1e-6, impl="radial", exogenous="uniform",
                            autoreset=True, **kw)
    env.check_actions = False
    gen = torch.Generator(device=dev).manual_seed(5)
    # the same float32 actions for every variant, inside the float32 Box (a float64 environment gets them widened)
    a_lo = torch.as_tensor(np.asarray(env.action_space.low, np.float64), device=dev)
    a_hi = torch.as_tensor(np.asarray(env.action_space.high, np.float64), device=dev)
    n_pool = 16
    pool32 = [(a_lo + (a_hi - a_lo) * (0.001 + 0.998 * torch.rand((E_, a_lo.numel()), generator=gen, dtype=torch.float64, device=dev)))
              .float().contiguous() for _ in range(n_pool)]
    pool64 = [x.double() for x in pool32]
    sink = None

    def step(k):
        nonlocal sink
        if a.variant == "f64":
            env.step(pool64[k % n_pool])
        elif a.variant == "f32":
            env.step(pool32[k % n_pool])
        else:
            obs, rew, _, _, _ = env.step(pool32[k % n_pool].double())
            sink = (obs.float(), rew.float())

    times = []
    for rep in range(a.repeat):
        env.reset(seed=7, options={"sampler": "device"})
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
    print(json.dumps(dict(task=a.task, label=a.label or a.variant, variant=a.variant, root=os.path.basename(os.path.abspath(a.root)),
                          envs=E_, steps=a.steps, us_per_step=[round(t, 2) for t in times],
                          collapsed_now=float(env.terminated.double().mean()), device=torch.cuda.get_device_name(0))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
