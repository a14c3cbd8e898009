#!/usr/bin/env python
"""Time the rollout bookkeeping of an on-policy loop on ANM6Easy (65 536 environments, float32 I/O, T = 128, autoreset, a
time limit of 100 steps, a random policy): the device rollout buffer (gym_anm_amd/rollout.py) against the same bookkeeping
and GAE written with torch ops.  One process per arm, one JSON line per process; `--root DIR` imports the package from
another checkout, so that the torch arm runs against the parent revision (it never imports the new module) and the two can be
alternated on one card:

    python scripts/rollout_bench.py --arm torch --root ../parent    (a) per step: copies of obs / reward / flags into [T, E, ...]
                                                                        tensors and the rule-2 mask; then GAE as a Python loop
                                                                        over T, returns, masked moments, normalisation
    python scripts/rollout_bench.py --arm buffer                     (b) RolloutBuffer: add per step, finish(normalize=True)
    python scripts/rollout_bench.py --summarise runs.jsonl           min / median / max per arm and figure

Figures, all from HIP events, per timed round (a warm-up rollout comes first in every process):
  add_us      the per-step bookkeeping alone, behind no step: a window around T of them, divided by T
  finish_us   GAE + advantage normalisation, one window
  rollout_us  a whole rollout -- T x (policy write, step, bookkeeping) and the finish --, one window, per step
  finish_graph_us  (buffer arm) the same four launches replayed from a captured HIP graph: without the host's issue time
  gae_us      (buffer arm) k_rollout_gae alone: a window around 20 launches back to back, per launch; `gae_bytes` are its bytes
              from the shapes (per slot: reward, value, flags byte read, advantage and return written; per environment the
              bootstrap value), `gae_tb_s` their quotient, to set against the 8.0 TB/s HBM3E peak of one MI355X (6.29 TB/s
              measured for a float4 copy)"""
import argparse
import json
import os
import sys


def summarise(path):
    import statistics as st

    rows = [json.loads(x) for x in open(path) if x.startswith("{")]
    by = {}
    for r in rows:
        for fig in ("add_us", "finish_us", "finish_graph_us", "rollout_us", "gae_us", "gae_tb_s"):
            if r.get(fig):
                by.setdefault((r["arm"], fig), []).extend(r[fig])
    print("%-7s %-16s %4s %10s %10s %10s" % ("arm", "figure", "n", "min", "median", "max"))
    for k in sorted(by):
        v = by[k]
        print("%-7s %-16s %4d %10.2f %10.2f %10.2f" % (k + (len(v), min(v), st.median(v), max(v))))
    for r in rows[:1]:
        print("envs %d, T %d, %s" % (r["envs"], r["T"], r["device"]))
    for r in rows:
        if r.get("gae_bytes"):
            print("k_rollout_gae moves %.1f MB per launch (from the shapes)" % (r["gae_bytes"] / 1e6))
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["torch", "buffer"], default="buffer")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds in this process")
    ap.add_argument("--root", default=None, help="another checkout to import the package from (the parent revision)")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.abspath(a.root or here))

    import torch

    from gym_anm_amd.envs import ANM6EasyVec

    dev, E_, T = torch.device("cuda:0"), a.envs, a.T
    f32 = torch.float32
    env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True, io_dtype=f32, max_episode_steps=100)
    env.check_actions = False
    lo, hi = (torch.as_tensor(x, dtype=f32, device=dev) for x in (env.action_space.low, env.action_space.high))
    gen = torch.Generator(device=dev).manual_seed(5)
    pool = [torch.minimum(torch.maximum(lo + (hi - lo) * torch.rand((E_, 6), generator=gen, dtype=f32, device=dev), lo), hi).contiguous()
            for _ in range(16)]
    obs0, _ = env.reset(seed=7)
    D = obs0.shape[1]
    gamma, lam, eps = float(env.gamma), 0.95, 1e-8
    w = torch.randn(D, generator=gen, dtype=f32, device=dev) * 0.1

    if a.arm == "buffer":
        from gym_anm_amd.rollout import RolloutBuffer

        buf = RolloutBuffer(env, T, gae_lambda=lam)
        obs, actions, values = buf.obs, buf.actions, buf.values

        def begin(o):
            buf.begin(o)

        def add(k, out):
            if k == 0:
                buf._k = 0          # (the add-alone window fills the slots again without a begin)
            buf.add(*out[:4])

        def finish():
            buf.finish(normalize=True)
    else:
        z = lambda *s, dt=f32: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
        obs, actions, rewards, values = z(T + 1, E_, D), z(T, E_, 6), z(T, E_), z(T + 1, E_)
        valid, term, trunc = z(T, E_, dt=torch.bool), z(T, E_, dt=torch.bool), z(T, E_, dt=torch.bool)
        adv, ret, adv_norm = z(T, E_), z(T, E_), z(T, E_)
        t_seen = z(E_, dt=torch.int32)

        def begin(o):
            obs[0].copy_(o)
            t_seen.copy_(env.timestep)

        def add(k, out):
            o, r, te, tr = out[:4]
            ts = env.timestep
            obs[k + 1].copy_(o)
            rewards[k].copy_(r)
            torch.logical_and(ts != t_seen, ts != 0, out=valid[k])
            term[k].copy_(te)
            trunc[k].copy_(tr)
            t_seen.copy_(ts)

        def finish():
            a_next = torch.zeros(E_, dtype=f32, device=dev)
            for k in range(T - 1, -1, -1):
                boot = gamma * values[k + 1] * ~term[k]
                delta = rewards[k] + boot - values[k]
                cont = ~(term[k] | trunc[k])
                a_next = (delta + gamma * lam * cont * a_next) * valid[k]
                adv[k].copy_(a_next)
            torch.add(adv, values[:T], out=ret)
            ret.mul_(valid)
            n = valid.sum()
            m = (adv * valid).sum() / n
            var = (((adv - m) ** 2) * valid).sum() / (n - 1)
            torch.mul((adv - m) / (var.sqrt() + eps), valid, out=adv_norm)

    def policy(k):
        actions[k].copy_(pool[k % 16])
        torch.mv(obs[k], w, out=values[k])

    def rollout(o):
        begin(o)
        for k in range(T):
            policy(k)
            add(k, env.step(actions[k]))
        torch.mv(obs[T], w, out=values[T])
        finish()

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return 1e3 * t0.elapsed_time(t1)

    rollout(obs0)                                    # warm-up: every kernel and torch op has run once
    out = env.step(actions[0])
    res = dict(add_us=[], finish_us=[], finish_graph_us=[], rollout_us=[], gae_us=[], gae_tb_s=[])
    graph = None
    if a.arm == "buffer":
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            finish()
    gae_bytes = T * E_ * (4 + 4 + 1 + 4 + 4) + 4 * E_
    for _ in range(a.rounds):
        res["rollout_us"].append(window(lambda: rollout(obs[T].clone())) / T)
        res["add_us"].append(window(lambda: [add(k, out) for k in range(T)]) / T)
        res["finish_us"].append(window(finish))
        if a.arm == "buffer":
            res["finish_graph_us"].append(window(graph.replay))
            us = window(lambda: [buf.finish(normalize=False) for _ in range(20)]) / 20
            res["gae_us"].append(us)
            res["gae_tb_s"].append(gae_bytes / us / 1e6)
    print(json.dumps(dict(arm=a.arm, revision="parent" if a.root else "this", envs=E_, T=T, gae_bytes=gae_bytes if a.arm == "buffer" else None,
                          device=torch.cuda.get_device_name(0), **{k: [round(x, 3) for x in v] for k, v in res.items()})), flush=True)


if __name__ == "__main__":
    main()
