#!/usr/bin/env python
"""Time the gradient of one PPO minibatch on ANM6Easy (hidden (64, 64), tanh, float32, B = 65 536) on one finished rollout:
``PPOGradient`` (gym_anm_amd/policy_grad.py, two launches) against the same loss written with torch ops.  One process per arm,
one JSON line per process, so that the arms can be alternated on one card:

    python scripts/ppo_grad_bench.py --arm grad       (a) g(mb)
    python scripts/ppo_grad_bench.py --arm torch      (b) evaluate, the clipped loss, zero_grad and backward: eager torch
    python scripts/ppo_grad_bench.py --arm graph      (c) arm (b) captured into a HIP graph and replayed
    python scripts/ppo_grad_bench.py --arm grad --rows-per-partial 128     (a) with another R than rows_per_partial(B)
    python scripts/ppo_grad_bench.py --summarise runs.jsonl      min / median / max per arm

The figure, from HIP events, per timed round (a warm-up comes first in every process): ``grad_us``, a window around 20
gradient calls on one gathered minibatch, per call."""
import argparse
import json
import os
import sys


def summarise(path):
    import statistics as st

    rows = [json.loads(x) for x in open(path) if x.startswith("{")]
    by = {}
    for r in rows:
        key = r["arm"] if r["arm"] != "grad" else "grad R=%d" % r["rows_per_partial"]
        by.setdefault(key, []).extend(r["grad_us"])
    print("%-14s %4s %10s %10s %10s" % ("arm", "n", "min", "median", "max"))
    for k in sorted(by):
        v = by[k]
        print("%-14s %4d %10.2f %10.2f %10.2f" % (k, len(v), min(v), st.median(v), max(v)))
    for r in rows[:1]:
        print("B %d, envs %d x %d steps, hidden %s, %s" % (r["B"], r["envs"], r["steps"], r["hidden"], r["device"]))
    a = [v for k, v in by.items() if k.startswith("grad")]
    b = by.get("torch")
    if a and b:
        best = min(st.median(v) for v in a)
        print("condition (g(mb) median not above eager torch median): %s (%.1f against %.1f us)" % (
            "met" if best <= st.median(b) else "NOT MET", best, st.median(b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["grad", "torch", "graph"], default="grad")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=2, help="slots of the rollout")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows-per-partial", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds in this process")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch

    from gym_anm_amd import policy_grad
    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.policy import GaussianMLPPolicy
    from gym_anm_amd.rollout import RolloutBuffer

    E_, T, B, hidden, reps = a.envs, a.steps, a.batch, (64, 64), 20
    clip, vf_coef, ent_coef = 0.2, 0.5, 0.0
    f32 = torch.float32
    env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True, io_dtype=f32, max_episode_steps=100,
                      action_map="unit")
    env.check_actions = False
    obs0, _ = env.reset(seed=7)
    pi = GaussianMLPPolicy(env, hidden=hidden, seed=1, init_seed=2)
    buf = RolloutBuffer(env, T, gae_lambda=0.95)
    buf.obs[T].copy_(obs0)
    buf.begin()
    for k in range(T):
        pi.act(buf.obs[k], buf.actions[k], buf.values[k], buf.logp[k])
        buf.add(*env.step(buf.actions[k])[:4])
    pi.value(buf.obs[T], buf.values[T])
    buf.finish(normalize=True)
    sampler = buf.sampler(B, seed=3)
    sampler.prepare()
    mb = sampler.gather(0, 0)
    torch.manual_seed(11)
    with torch.no_grad():                                 # a second epoch's parameters: the ratio is not 1 everywhere
        pi.flat.add_(0.01 * torch.randn_like(pi.flat))
    torch.cuda.synchronize()

    R = 0
    if a.arm == "grad":
        g = pi.ppo_gradient(B, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef)
        if a.rows_per_partial:                            # (a measurement's own R: the class takes rows_per_partial(B))
            g.rows_per_partial = g._struct.rows_per_partial = a.rows_per_partial
            g.partials = torch.zeros(-(-B // a.rows_per_partial) * (pi.n_params + policy_grad.STATS), dtype=f32, device=pi.device)
            g._struct.partials = g.partials.data_ptr()
        R = g.rows_per_partial

        def once():
            g(mb)
    else:
        opt = torch.optim.Adam([pi.flat], lr=3e-4)

        def once():
            logp, entropy, values = pi.evaluate(mb.obs, mb.actions)
            ratio = torch.exp(logp - mb.logp)
            pg = -torch.min(ratio * mb.adv, torch.clamp(ratio, 1 - clip, 1 + clip) * mb.adv)
            v = 0.5 * (values - mb.returns) ** 2
            n = (mb.weight != 0).sum()
            loss = (mb.weight * (pg + vf_coef * v)).sum() / n - ent_coef * entropy[0]
            opt.zero_grad()
            loss.backward()

    def calls():
        for _ in range(reps):
            once()

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return 1e3 * t0.elapsed_time(t1)

    timed = calls
    if a.arm == "graph":
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                     # warm-up on a side stream, as capture of autograd asks for
            for _ in range(3):
                once()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            calls()
        timed = graph.replay
    calls()                                               # warm-up: every kernel and torch op has run once
    torch.cuda.synchronize()
    res = [window(timed) / reps for _ in range(a.rounds)]
    print(json.dumps(dict(arm=a.arm, B=B, envs=E_, steps=T, hidden=list(hidden), rows_per_partial=R, device=torch.cuda.get_device_name(0),
                          grad_norm=round(float(pi.flat.grad.norm()), 6), grad_us=[round(x, 3) for x in res])), flush=True)


if __name__ == "__main__":
    main()
