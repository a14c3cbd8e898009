#!/usr/bin/env python
"""Time the policy of an on-policy rollout on ANM6Easy (65 536 environments, float32 I/O, ``action_map="unit"``, hidden (64, 64),
tanh): ``GaussianMLPPolicy.act`` (gym_anm_amd/policy.py, one launch) against the same actor-critic written with torch ops, on
the same observations.  One process per arm, one JSON line per process, so that the arms can be alternated on one card:

    python scripts/policy_bench.py --arm act        (a) pi.act(obs, actions, values, logp)
    python scripts/policy_bench.py --arm torch      (b) the evaluate forward (two MLPs), torch.randn, the sample, log_prob: eager,
                                                        under no_grad, the way a user without the kernel has to write it
    python scripts/policy_bench.py --arm graph      (c) arm (b) captured into a HIP graph and replayed
    python scripts/policy_bench.py --summarise runs.jsonl      min / median / max per arm and figure

Figures, all from HIP events, per timed round (a warm-up comes first in every process):
  policy_us   one policy call of the arm: a window around 20 calls, per call (for arm (a) launched back to back from one
              stream this is the kernel's own duration where the host issues faster than the kernel runs)
  step_us     the full rollout step with the arm's policy -- policy, env.step, buf.add --: a window around 20 steps, eager
  step_graph_us   the same 20 steps captured into one HIP graph and replayed"""
import argparse
import json
import math
import os
import sys


def summarise(path):
    import statistics as st

    rows = [json.loads(x) for x in open(path) if x.startswith("{")]
    by = {}
    for r in rows:
        for fig in ("policy_us", "step_us", "step_graph_us"):
            if r.get(fig):
                by.setdefault((r["arm"], fig), []).extend(r[fig])
    print("%-7s %-14s %4s %10s %10s %10s" % ("arm", "figure", "n", "min", "median", "max"))
    for k in sorted(by):
        v = by[k]
        print("%-7s %-14s %4d %10.2f %10.2f %10.2f" % (k + (len(v), min(v), st.median(v), max(v))))
    for r in rows[:1]:
        print("envs %d, hidden %s, %s" % (r["envs"], r["hidden"], r["device"]))
    a, b, c = (by.get((arm, "policy_us")) for arm in ("act", "torch", "graph"))
    if a and b:
        print("condition (act median not above eager torch median): %s (%.1f against %.1f us)" % (
            "met" if st.median(a) <= st.median(b) else "NOT MET", st.median(a), st.median(b)))
    if a and c:
        print("against the captured torch formulation: %.1f against %.1f us" % (st.median(a), st.median(c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["act", "torch", "graph"], default="act")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds in this process")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch

    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.policy import GaussianMLPPolicy
    from gym_anm_amd.rollout import RolloutBuffer

    E_, hidden, reps = a.envs, (64, 64), 20
    f32 = torch.float32
    env = ANM6EasyVec(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True, io_dtype=f32, max_episode_steps=100,
                      action_map="unit")
    env.check_actions = False
    obs0, _ = env.reset(seed=7)
    pi = GaussianMLPPolicy(env, hidden=hidden, seed=1, init_seed=2)
    buf = RolloutBuffer(env, reps, gae_lambda=0.95)
    half_log_2pi = 0.5 * math.log(2.0 * math.pi)

    def torch_policy(obs, actions, values, logp):
        """arm (b): what `evaluate` computes forward, a draw, the sample and its log-probability, written into the slot views"""
        with torch.no_grad():
            x, v = obs, obs
            for i in range(len(hidden) + 1):
                x = x @ pi.actor[i].weight + pi.actor[i].bias
                v = v @ pi.critic[i].weight + pi.critic[i].bias
                if i < len(hidden):
                    x, v = torch.tanh(x), torch.tanh(v)
            eps = torch.randn_like(x)
            torch.addcmul(x, eps, torch.exp(pi.log_std), out=actions)
            torch.sum(-0.5 * eps * eps - pi.log_std - half_log_2pi, dim=1, out=logp)
            values.copy_(v[:, 0])

    policy = pi.act if a.arm == "act" else torch_policy

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return 1e3 * t0.elapsed_time(t1)

    def policy_calls():
        for k in range(reps):
            policy(obs0, buf.actions[k], buf.values[k], buf.logp[k])

    def steps():
        buf.begin()
        for k in range(reps):
            policy(buf.obs[k], buf.actions[k], buf.values[k], buf.logp[k])
            buf.add(*env.step(buf.actions[k])[:4])

    buf.obs[reps].copy_(obs0)
    policy_calls()                                   # warm-up: every kernel and torch op has run once
    steps()
    torch.cuda.synchronize()
    g_policy = g_steps = None
    if a.arm == "graph":
        g_policy = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_policy):
            policy_calls()
    g_steps = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_steps):
        steps()
    torch.cuda.synchronize()
    g_steps.replay()
    res = dict(policy_us=[], step_us=[], step_graph_us=[])
    for r in range(a.rounds):
        res["policy_us"].append(window(g_policy.replay if a.arm == "graph" else policy_calls) / reps)
        if a.arm != "graph":
            res["step_us"].append(window(steps) / reps)
        res["step_graph_us"].append(window(g_steps.replay) / reps)
    print(json.dumps(dict(arm=a.arm, envs=E_, hidden=list(hidden), device=torch.cuda.get_device_name(0),
                          **{k: [round(x, 3) for x in v] for k, v in res.items()})), flush=True)


if __name__ == "__main__":
    main()
