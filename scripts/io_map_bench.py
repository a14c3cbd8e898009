#!/usr/bin/env python
"""Time the env-step of ANM6Easy (65 536 environments, tol 1e-6, cap 100, autoreset, thread-per-environment family) without
and with the affine policy I/O of the step kernels (``action_map="unit"``, ``obs_map="box"``, ``reward_scale=``;
gym_anm_amd/io_affine.py), and against what the mode replaces: the float32 step wrapped in the torch ops of a policy loop.
One process per variant, one JSON line per process; `--root DIR` imports the package from another checkout, so that this
revision and its parent can be alternated on one card:

    python scripts/io_map_bench.py --variant f64 --root ../parent     plain float64 step, the parent revision
    python scripts/io_map_bench.py --variant f64                      ... this revision
    python scripts/io_map_bench.py --variant f32 [--root ../parent]   plain float32 step (io_dtype=torch.float32)
    python scripts/io_map_bench.py --variant mapped                   float32 step through the three maps, in the kernel
    python scripts/io_map_bench.py --variant wrapped --root ../parent float32 step + addcmul and clamp on the action, addcmul
                                                                      on obs, mul on the reward: one HIP-event window
    python scripts/io_map_bench.py --summarise runs.jsonl             min / median / max per (variant, revision), acceptance

Two clocks per run.  `launch_us`: anm_time_step_launches (HIP events around `steps` launches of the step, inside the library,
after `warmup` steps) -- the bare step; not for `wrapped`.  `window_us`: HIP events around a Python loop of the same steps,
with the torch ops of `wrapped` inside the window.  The acceptance comparisons: the plain f64 / f32 medians of
this revision inside the parent's own min-max spread (launch_us); `mapped` below `wrapped` (window_us)."""
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
    print("%-8s %-7s %-10s %4s %9s %9s %9s" % ("variant", "rev", "clock", "n", "min", "median", "max"))
    stat = {}
    few = sorted(k for k, v in by.items() if len(v) < 5)
    if few:
        raise SystemExit("fewer than 5 repetitions of %s: no summary" % ", ".join("%s/%s/%s" % k for k in few))
    for k in sorted(by):
        v = by[k]
        stat[k] = (min(v), st.median(v), max(v))
        print("%-8s %-7s %-10s %4d %9.2f %9.2f %9.2f" % (k + (len(v),) + stat[k]))
    for var in ("f64", "f32"):
        a, b = stat.get((var, "parent", "launch_us")), stat.get((var, "this", "launch_us"))
        if a and b:
            where = "inside" if a[0] <= b[1] <= a[2] else "OUTSIDE, below its minimum (not slower)" if b[1] < a[0] else "OUTSIDE, above its maximum (SLOWER)"
            print("plain %s: this median %.2f us, parent spread [%.2f, %.2f] -> %s" % (var, b[1], a[0], a[2], where))
    m, w = stat.get(("mapped", "this", "window_us")), stat.get(("wrapped", "parent", "window_us"))
    if m and w:
        print("mapped f32 %.2f us against parent f32 + torch ops %.2f us (medians, window) -> %s" % (m[1], w[1], "faster" if m[1] < w[1] else "NOT FASTER"))
    m, p = stat.get(("mapped", "this", "launch_us")), stat.get(("f32", "parent", "launch_us"))
    if m and p:
        print("mapped f32 - parent bare f32 step: %+.2f us (medians, launch)" % (m[1] - p[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["f64", "f32", "mapped", "wrapped"], default="f64")
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

    import numpy as np
    import torch

    from gym_anm_amd import networks
    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.model import NetworkModel

    dev, E_ = torch.device("cuda:0"), a.envs
    f32 = a.variant != "f64"
    kw = dict(num_envs=E_, device="cuda:0", seed=7, tol=1e-6, max_iter=100, autoreset=True)
    if f32:
        kw["io_dtype"] = torch.float32
    if a.variant == "mapped":
        kw.update(action_map="unit", obs_map="box", reward_scale=1 / 64)
    env = ANM6EasyVec(**kw)
    env.check_actions = False
    sim = env.simulator
    # the tables of the maps, for the torch ops of `wrapped` (written out: the parent revision has no io_affine)
    lo, hi = (np.asarray(x, np.float64) for x in NetworkModel(networks.anm6_network(), 0.25, 100).action_bounds())
    dt = torch.float32 if f32 else torch.float64
    t = lambda x: torch.as_tensor(x, dtype=dt, device=dev)  # noqa: E731
    mid, half, a_lo, a_hi = t(0.5 * lo + 0.5 * hi), t(0.5 * hi - 0.5 * lo), t(lo), t(hi)
    olo, ohi = np.asarray(env.observation_space.low, np.float64), np.asarray(env.observation_space.high, np.float64)
    ok = np.isfinite(olo) & np.isfinite(ohi) & (olo < ohi)
    with np.errstate(all="ignore"):
        o_scale, o_bias = t(np.where(ok, 2 / (ohi - olo), 1.0)), t(np.where(ok, -(ohi + olo) / (ohi - olo), 0.0))
    gen = torch.Generator(device=dev).manual_seed(5)
    n_pool = 16
    unit = a.variant in ("mapped", "wrapped")
    if unit:
        pool = [(2 * torch.rand((E_, 6), generator=gen, dtype=torch.float64, device=dev) - 1).to(dt).contiguous() for _ in range(n_pool)]
    else:
        pool = [(a_lo.double() + (a_hi.double() - a_lo.double()) * torch.rand((E_, 6), generator=gen, dtype=torch.float64, device=dev))
                .to(dt).contiguous() for _ in range(n_pool)]
        pool = [torch.minimum(torch.maximum(x, t(env.action_space.low)), t(env.action_space.high)).contiguous() for x in pool]
    act = torch.empty_like(pool[0])
    obs_out, rew_out = torch.empty_like(env._state_obs), torch.empty_like(env.reward)
    ms = C.c_float(0.0)

    def one_step(k):
        if a.variant == "wrapped":   # what a policy loop does around the plain float32 step
            torch.addcmul(mid, pool[k % n_pool], half, out=act)
            torch.clamp(act, a_lo, a_hi, out=act)
            env._step_call(act.data_ptr(), None, None)
            torch.addcmul(o_bias, env._state_obs, o_scale, out=obs_out)
            torch.mul(env.reward, 1 / 64, out=rew_out)
        else:
            env._step_call(pool[k % n_pool].data_ptr(), None, None)

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
        if a.variant != "wrapped":          # the bare step, timed inside the library (one action tensor: the launches are the same)
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
