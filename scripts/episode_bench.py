#!/usr/bin/env python
"""What the in-kernel episode time limit and statistics cost a step, and what they save over doing the same on the host.

One variant per process, one JSON line per run (HIP events on the launch stream around `--steps` steps after `--warmup`):

  off    no limit, no statistics (with `--root ../parent`: the revision before the feature)
  limit  max_episode_steps = T (default 3000, the fixed episode length of the reference's write-ups)
  stats  ... and episode_stats=True
  host   what a user has without the feature: step(), then `timestep >= T` as a torch op, then a masked reset(), every step

on `--task anm6` (ANM6Easy, 65 536 environments, the coalesced-row fast path) or `--task feeder` (the 30-bus feeder, 16 384
environments, lane-group kernel, loads and generation drawn in the kernel).  Run the variants ALTERNATED on one card, several
rounds, and summarise the lines:

    python scripts/episode_bench.py --task anm6 --variant off --root ../parent --label a >> runs.jsonl
    python scripts/episode_bench.py --task anm6 --variant off --label b >> runs.jsonl
    ...
    python scripts/episode_bench.py --summarise runs.jsonl
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
    ap.add_argument("--variant", choices=["off", "limit", "stats", "host"], default="off")
    ap.add_argument("--limit", type=int, default=3000)
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
    kw = {}
    if a.variant in ("limit", "stats"):
        kw["max_episode_steps"] = a.limit
    if a.variant == "stats":
        kw["episode_stats"] = True
    if a.task == "anm6":
        E_ = a.envs or 65536
        env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, autoreset=True, **kw)
    else:
        E_ = a.envs or 16384
        env = BatchedANMEnv(networks.synthetic_radial_network(30, 0), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array([[0, 1e9]]),
                            costs_clipping=(1, 100), seed=7, num_envs=E_, device="cuda:0", tol=1e-6, impl="radial", exogenous="uniform",
                            autoreset=True, **kw)
    env.check_actions = False
    f64 = dict(dtype=torch.float64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    a_lo, a_hi = torch.as_tensor(env.action_space.low, **f64), torch.as_tensor(env.action_space.high, **f64)
    n_pool = 16
    actions = [(a_lo + (a_hi - a_lo) * torch.rand((E_, a_lo.numel()), generator=gen, **f64)).contiguous() for _ in range(n_pool)]

    def step(k):
        env._step_call(actions[k % n_pool].data_ptr(), None, None)
        if a.variant == "host":
            env.reset(options={"sampler": "device", "mask": env.timestep >= a.limit})

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
                          envs=E_, limit=a.limit if a.variant != "off" else None, steps=a.steps,
                          us_per_step=[round(t, 2) for t in times], collapsed_now=float(env.terminated.double().mean()),
                          device=torch.cuda.get_device_name(0))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
