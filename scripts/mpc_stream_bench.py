"""Cost of the stream forecast of the MPC agents: one act() of all environments, ANM6 at 65 536
environments in the uniform and the series-noise mode (ANM6Easy's tables, amplitude 2 MW), N = 1 and N = 10.

    (a) MPCAgentConstant.act at the parent revision     (b) MPCAgentConstant.act at this revision
    (c) MPCAgentPerfectStream.act (one launch)           (d) its unfused path (forecast on the host), for context

Method (that of DESIGN.md 3.11): HIP events around 200 calls after 20, three timed runs per process, the variants
alternated on one card over three rounds; every process is a fresh one.  (d): 10 calls after 2, one round.

    python scripts/mpc_stream_bench.py --parent PATH_TO_A_BUILT_TREE_OF_THE_PARENT_REVISION [--out FILE] [--rounds 3]
    python scripts/mpc_stream_bench.py --one VARIANT MODE N [--root TREE]       # one process, one JSON line

The claim to check: (b) lies inside (a)'s own min-max spread (the existing instantiations kept their instruction streams);
(c) - (b) is the price of the Philox rounds, 1 + ceil(n_exo / 2) blocks per lane."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E = 65536
DEV = "cuda:0"


def one(variant, mode, N, root):
    sys.path.insert(0, root)
    import numpy as np
    import torch

    from gym_anm_amd import agents, networks
    from gym_anm_amd.envs.anm6 import ANM6EasyVec
    from gym_anm_amd.envs.anm_env import BatchedANMEnv

    if mode == "noise":
        env = ANM6EasyVec(num_envs=E, device=DEV, seed=3, tol=1e-6, exogenous="series_noise", exo_noise=2.0, autoreset=True)
    else:
        env = BatchedANMEnv(networks.anm6_network(), "state", 1, 0.25, 0.995, 100, aux_bounds=np.array(((0, 1000),)),
                            costs_clipping=(1, 100), seed=3, num_envs=E, device=DEV, tol=1e-6, exogenous="uniform", autoreset=True)
    env.check_actions = False
    env.reset()
    Agent = agents.MPCAgentConstant if variant == "constant" else agents.MPCAgentPerfectStream
    if variant == "unfused":
        class Agent(agents.MPCAgentPerfectStream):   # noqa: F811
            def _fused(self, env):
                return False
    ag = Agent(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N)
    ag.warn_unconverged, ag.reuse_action_buffer = False, True
    assert ag._fused(env) == (variant != "unfused")
    for _ in range(3):                               # a few real steps: the batch is spread over its episodes
        env.step(ag.act(env).clone())
    warm, calls = (2, 10) if variant == "unfused" else (20, 200)
    runs = []
    for _ in range(3):
        for _ in range(warm):
            ag.act(env)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            ag.act(env)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / calls)
    print(json.dumps(dict(variant=variant, mode=mode, N=N, ms=runs, iters=float(ag.solver.iters.double().mean()),
                          converged=float(ag.last_converged.double().mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("VARIANT", "MODE", "N"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], int(args.one[2]), os.path.abspath(args.root))
    if not args.parent:
        ap.error("--parent: a built tree of the parent revision")
    variants = [("a", "constant", os.path.abspath(args.parent)), ("b", "constant", ROOT), ("c", "stream", ROOT)]
    res = {}

    def run(tag, variant, root, mode, N):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", variant, mode, str(N), "--root", root]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
        if p.returncode != 0:
            sys.exit("%s failed (%d): %s" % (" ".join(cmd), p.returncode, p.stderr[-2000:]))   # (nothing more is started)
        r = json.loads(p.stdout.strip().split("\n")[-1])
        res.setdefault((mode, N, tag), []).extend(r["ms"])
        res[(mode, N, tag, "iters")] = r["iters"]
        print(tag, mode, N, ["%.4f" % x for x in r["ms"]], flush=True)

    cases = [(m, N) for m in ("uniform", "noise") for N in (1, 10)]
    for _ in range(args.rounds):
        for mode, N in cases:
            for tag, variant, root in variants:
                run(tag, variant, root, mode, N)
    for mode, N in cases:
        run("d", "unfused", ROOT, mode, N)
    lines = ["# scripts/mpc_stream_bench.py: ms per act() of %d ANM6 environments; HIP events around 200 calls after 20, three timed" % E,
             "# runs per process, %d rounds of alternated fresh processes on one card: median [min - max] of the %d runs" % (args.rounds, 3 * args.rounds),
             "# (d: 10 calls after 2, one process).  a: MPCAgentConstant at the parent revision, b: at this revision,",
             "# c: MPCAgentPerfectStream (one launch), d: its unfused path (forecast on the host)",
             "%-8s %3s  %-26s %-26s %-26s %-26s %9s %12s %6s" % ("mode", "N", "a", "b", "c", "d", "c - b", "b inside a", "iters c")]
    for mode, N in cases:
        def cell(tag):
            v = res[(mode, N, tag)]
            return "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))
        a, b, c = (res[(mode, N, t)] for t in "abc")
        inside = min(a) <= statistics.median(b) <= max(a)
        lines.append("%-8s %3d  %-26s %-26s %-26s %-26s %9.4f %12s %6.1f" % (mode, N, cell("a"), cell("b"), cell("c"), cell("d"),
                                                                       statistics.median(c) - statistics.median(b), "yes" if inside else "NO",
                                                                       res[(mode, N, "c", "iters")]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
