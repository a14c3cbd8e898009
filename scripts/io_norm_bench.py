#!/usr/bin/env python
"""Time the env-step of ANM6Easy (65 536 environments, float32 I/O, tol 1e-6, cap 100, autoreset, thread-per-environment
family) without and with the running normalisation kept on the device (``obs_norm="running"``, ``reward_norm="running"``;
gym_anm_amd/io_norm.py), and against what it replaces: the float32 step wrapped in the torch ops of a VecNormalize-style
loop.  One process per variant, one JSON line per process; `--root DIR` imports the package from another checkout, so that
this revision and its parent can be alternated on one card:

    python scripts/io_norm_bench.py --variant plain --root ../parent    (c) plain float32 step, the parent revision
    python scripts/io_norm_bench.py --variant plain                     (c) ... this revision
    python scripts/io_norm_bench.py --variant norm                      (b) step() with both parts on: the step and the pair
    python scripts/io_norm_bench.py --variant pair                          the update pair alone, behind no step
    python scripts/io_norm_bench.py --variant wrapped --root ../parent  (a) float32 step + batch mean / var, merge, addcmul
                                                                        on obs, the return recurrence, its moments and
                                                                        merge, mul on the reward -- in torch
    python scripts/io_norm_bench.py --summarise runs.jsonl              min / median / max per (variant, revision)

Two clocks.  `launch_us`: anm_time_step_launches (HIP events around `steps` launches of the bare step, inside the library) --
`plain` only; what (c) compares.  `window_us`: HIP events around a Python loop of `steps` iterations with everything the
variant does per step inside the window."""
import argparse
import ctypes as C
import json
import os
import sys


def summarise(path):
    import statistics as st

    rows = [json.loads(x) for x in open(path) if x.startswith("{")]
    by = {}
    for r in rows:
        for clock in ("launch_us", "window_us"):
            if r.get(clock) is not None:
                by.setdefault((r["variant"], r["revision"], clock), []).extend(r[clock])
    few = sorted(k for k, v in by.items() if len(v) < 5)
    if few:
        raise SystemExit("fewer than 5 repetitions of %s: no summary" % ", ".join("%s/%s/%s" % k for k in few))
    print("%-8s %-7s %-10s %4s %9s %9s %9s" % ("variant", "rev", "clock", "n", "min", "median", "max"))
    stat = {}
    for k in sorted(by):
        v = by[k]
        stat[k] = (min(v), st.median(v), max(v))
        print("%-8s %-7s %-10s %4d %9.2f %9.2f %9.2f" % (k + (len(v),) + stat[k]))
    for clock in ("launch_us", "window_us"):
        a, b = stat.get(("plain", "parent", clock)), stat.get(("plain", "this", clock))
        if a and b:
            where = "inside" if a[0] <= b[1] <= a[2] else "OUTSIDE, below its minimum (not slower)" if b[1] < a[0] else "OUTSIDE, above its maximum (SLOWER)"
            print("(c) plain f32 %s: this median %.2f us, parent spread [%.2f, %.2f] -> %s" % (clock, b[1], a[0], a[2], where))
    n, w, p = stat.get(("norm", "this", "window_us")), stat.get(("wrapped", "parent", "window_us")), stat.get(("plain", "this", "window_us"))
    if n and w:
        print("(b) step with both parts on %.2f us against (a) parent f32 step + torch ops %.2f us (medians, window)" % (n[1], w[1]))
    if n and p:
        print("(b) - plain step of this revision: %+.2f us (medians, window)" % (n[1] - p[1]))
    q = stat.get(("pair", "this", "window_us"))
    if q:
        print("the update pair alone: %.2f us (median, window)" % q[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["plain", "norm", "pair", "wrapped"], default="plain")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5, help="timed runs in this process (the summary wants at least 5 per configuration)")
    ap.add_argument("--root", default=None, help="another checkout to import the package from (the parent revision)")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.abspath(a.root or here))

    import torch

    from gym_anm_amd.envs import ANM6EasyVec

    dev, E_ = torch.device("cuda:0"), a.envs
    f32 = torch.float32
    kw = dict(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True, io_dtype=f32)
    if a.variant in ("norm", "pair"):
        kw.update(obs_norm="running", reward_norm="running")
    env = ANM6EasyVec(**kw)
    env.check_actions = False
    sim = env.simulator
    t = lambda x: torch.as_tensor(x, dtype=f32, device=dev)  # noqa: E731
    a_lo, a_hi = t(env.action_space.low), t(env.action_space.high)
    gen = torch.Generator(device=dev).manual_seed(5)
    n_pool = 16
    pool = [(a_lo.double() + (a_hi.double() - a_lo.double()) * torch.rand((E_, 6), generator=gen, dtype=torch.float64, device=dev)).to(f32)
            for _ in range(n_pool)]
    pool = [torch.minimum(torch.maximum(x, a_lo), a_hi).contiguous() for x in pool]
    ms = C.c_float(0.0)

    # the torch side of `wrapped`: Gymnasium's RunningMeanStd / NormalizeObservation / NormalizeReward on device tensors
    D = env._state_obs.shape[1]
    gamma, eps, n = float(env.gamma), 1e-8, float(E_)
    o_mean, o_var = torch.zeros(D, dtype=f32, device=dev), torch.ones(D, dtype=f32, device=dev)
    r_mean, r_var = torch.zeros((), dtype=f32, device=dev), torch.ones((), dtype=f32, device=dev)
    ret = torch.zeros(E_, dtype=f32, device=dev)
    obs_out, rew_out = torch.empty_like(env._state_obs), torch.empty_like(env.reward)
    cnt = [1e-4, 1e-4]

    def merge(mean, var, c, bmean, bvar):
        tot = c + n
        delta = bmean - mean
        m2 = var * c + bvar * n + delta * delta * (c * n / tot)
        mean.add_(delta * (n / tot))
        var.copy_(m2 / tot)
        return tot

    def one_step(k):
        if a.variant == "pair":
            env._norm_update()
            return
        if a.variant == "norm":
            env.step(pool[k % n_pool])
            return
        env._step_call(pool[k % n_pool].data_ptr(), None, None)
        if a.variant == "wrapped":
            x, r = env._state_obs, env.reward
            bvar, bmean = torch.var_mean(x, dim=0, unbiased=False)
            cnt[0] = merge(o_mean, o_var, cnt[0], bmean, bvar)
            scale = torch.rsqrt(o_var + eps)
            torch.addcmul(-o_mean * scale, x, scale, out=obs_out)
            ret.mul_(gamma).add_(r)
            bvar, bmean = torch.var_mean(ret, unbiased=False)
            cnt[1] = merge(r_mean, r_var, cnt[1], bmean, bvar)
            torch.mul(r, torch.rsqrt(r_var + eps), out=rew_out)
            ret.mul_(~env._term_bool)

    launch_us, window_us = [], []
    for rep in range(a.repeat):
        env._reset_count.zero_()            # (every timed run replays the same episodes)
        env.reset(seed=7)
        for k in range(a.warmup):
            one_step(k)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(a.steps):
            one_step(a.warmup + k)
        t1.record()
        torch.cuda.synchronize()
        window_us.append(1e3 * t0.elapsed_time(t1) / a.steps)
        if a.variant == "plain":            # the bare step, timed inside the library
            args = env._step_args
            with sim._device_ctx():
                rc = sim.backend.lib.anm_time_step_launches(
                    sim._handle, E_, pool[0].data_ptr(), args[0], args[1], args[2], args[3], args[4], args[5], args[6], args[7], 1,
                    env.rng_seed, env.env_offset, env._reset_count_ptr, env._aux_index_ptr, env._ws_ref, env._opts_ref,
                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), a.steps, C.byref(ms))
            sim.backend.check(rc, "anm_time_step_launches")
            launch_us.append(1e3 * ms.value)
    print(json.dumps(dict(variant=a.variant, revision="parent" if a.root else "this", envs=E_, steps=a.steps, warmup=a.warmup,
                          launch_us=[round(x, 2) for x in launch_us] or None, window_us=[round(x, 2) for x in window_us],
                          terminated_share_at_end=round(float(env.terminated.double().mean()), 4),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
