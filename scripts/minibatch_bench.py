#!/usr/bin/env python
"""Time one PPO epoch's minibatch sampling on the rollout buffer of ANM6Easy (65 536 environments, float32 I/O, T = 128,
autoreset, a time limit of 100 steps, a random policy; B = 65 536): the device sampler (gym_anm_amd/minibatch.py) against the
same sampling written with torch ops, both on the same finished buffer.  One process per arm, one JSON line per process, so
that the two can be alternated on one card:

    python scripts/minibatch_bench.py --arm torch      (a) valid.flatten().nonzero() (a host sync), randperm(n), then per
                                                           minibatch six index_select: obs, actions, logp, values, returns, adv
    python scripts/minibatch_bench.py --arm device     (b) sampler.prepare(), then sampler.gather(m, ep) for every m below
                                                           ceil(T E / B), the bound that needs no sync
    python scripts/minibatch_bench.py --summarise runs.jsonl      min / median / max per arm and figure

Figures, all from HIP events, per timed round (a warm-up epoch comes first in every process):
  epoch_us    one epoch -- (a): nonzero, randperm and ceil(n / B) minibatches; (b): prepare and ceil(T E / B) gathers --, one window
  gather_us   (device arm) k_mb_gather alone: a window around 20 launches of minibatch 0 (every row live) back to back, per
              launch; `gather_bytes` are its bytes from the shapes (per row: the index read, the row's words read and written,
              weight and slot written), `gather_tb_s` their quotient
  prepare_us  (device arm) the three launches of prepare: a window around 20 of them, per prepare"""
import argparse
import json
import os
import sys


def summarise(path):
    import statistics as st

    rows = [json.loads(x) for x in open(path) if x.startswith("{")]
    by = {}
    for r in rows:
        for fig in ("epoch_us", "gather_us", "gather_tb_s", "prepare_us"):
            if r.get(fig):
                by.setdefault((r["arm"], fig), []).extend(r[fig])
    print("%-7s %-12s %4s %10s %10s %10s" % ("arm", "figure", "n", "min", "median", "max"))
    for k in sorted(by):
        v = by[k]
        print("%-7s %-12s %4d %10.2f %10.2f %10.2f" % (k + (len(v), min(v), st.median(v), max(v))))
    for r in rows[:1]:
        print("envs %d, T %d, B %d, %d of %d slots valid, %s" % (r["envs"], r["T"], r["B"], r["n_valid"], r["envs"] * r["T"], r["device"]))
    for r in rows:
        if r.get("gather_bytes"):
            print("k_mb_gather moves %.1f MB per launch (from the shapes); %d gathers per epoch against %d torch minibatches" % (
                r["gather_bytes"] / 1e6, r["n_minibatches"], -(-r["n_valid"] // r["B"])))
            break
    d, t = by.get(("device", "epoch_us")), by.get(("torch", "epoch_us"))
    if d and t:
        print("condition (device median epoch not above torch median): %s (%.1f against %.1f us)" % (
            "met" if st.median(d) <= st.median(t) else "NOT MET", st.median(d), st.median(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["torch", "device"], default="device")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds in this process")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch

    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.rollout import RolloutBuffer

    dev, E_, T, B = torch.device("cuda:0"), a.envs, a.T, a.B
    f32 = torch.float32
    env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True, io_dtype=f32, max_episode_steps=100)
    env.check_actions = False
    lo, hi = (torch.as_tensor(x, dtype=f32, device=dev) for x in (env.action_space.low, env.action_space.high))
    gen = torch.Generator(device=dev).manual_seed(5)
    pool = [torch.minimum(torch.maximum(lo + (hi - lo) * torch.rand((E_, 6), generator=gen, dtype=f32, device=dev), lo), hi).contiguous()
            for _ in range(16)]
    obs0, _ = env.reset(seed=7)
    D = obs0.shape[1]
    w = torch.randn(D, generator=gen, dtype=f32, device=dev) * 0.1
    buf = RolloutBuffer(env, T, gae_lambda=0.95)
    buf.begin(obs0)
    for k in range(T):          # the rollout both arms sample from
        buf.actions[k].copy_(pool[k % 16])
        torch.mv(buf.obs[k], w, out=buf.values[k])
        buf.logp[k].normal_(generator=gen)
        buf.add(*env.step(buf.actions[k])[:4])
    torch.mv(buf.obs[T], w, out=buf.values[T])
    buf.finish(normalize=True)
    N, A = T * E_, buf.actions.shape[2]
    n_valid = int(buf.valid.sum())

    if a.arm == "device":
        sampler = buf.sampler(B, seed=11)
        n_mb = sampler.n_minibatches

        def epoch(ep=0):
            sampler.prepare()
            for m in range(n_mb):
                sampler.gather(m, ep)
    else:
        flat = (buf.obs[:T].reshape(N, D), buf.actions.reshape(N, A), buf.logp.reshape(N), buf.values[:T].reshape(N), buf.returns.reshape(N),
                buf.adv_norm.reshape(N))
        n_mb = -(-n_valid // B)

        def epoch(ep=0):
            idx = buf.valid.flatten().nonzero().squeeze(1)          # (dynamic shape: the host waits here)
            n = idx.numel()
            order = idx[torch.randperm(n, device=dev)]
            for m in range(-(-n // B)):
                s = order[m * B:(m + 1) * B]
                mb = [x.index_select(0, s) for x in flat]
            return mb

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return 1e3 * t0.elapsed_time(t1)

    epoch()                                          # warm-up: every kernel and torch op has run once
    res = dict(epoch_us=[], gather_us=[], gather_tb_s=[], prepare_us=[])
    gather_bytes = B * (4 + 2 * (4 * (D + A) + 4 * 4) + 4 + 4)
    for r in range(a.rounds):
        res["epoch_us"].append(window(lambda: epoch(r + 1)))
        if a.arm == "device":
            us = window(lambda: [sampler.gather(0, r) for _ in range(20)]) / 20
            res["gather_us"].append(us)
            res["gather_tb_s"].append(gather_bytes / us / 1e6)
            res["prepare_us"].append(window(lambda: [sampler.prepare() for _ in range(20)]) / 20)
    print(json.dumps(dict(arm=a.arm, envs=E_, T=T, B=B, n_valid=n_valid, n_minibatches=n_mb,
                          gather_bytes=gather_bytes if a.arm == "device" else None, device=torch.cuda.get_device_name(0),
                          **{k: [round(x, 3) for x in v] for k, v in res.items()})), flush=True)


if __name__ == "__main__":
    main()
