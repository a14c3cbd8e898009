"""Cost of the expected forecast of the MPC agents: one act() of all environments, ANM6Easy in series-noise
mode (amplitude 2 MW, exo_corr=0.8) at 65 536 environments, N = 1 and N = 10.

    (a) MPCAgentPerfectChain.act at the parent revision     (b) the same at this revision
    (c) MPCAgentExpected.act at this revision (one launch)

Method (that of DESIGN.md 3.11 and of scripts/mpc_chain_bench.py): HIP events around 200 calls after 20, three timed runs per
process, the variants alternated on one card over three rounds; every process is a fresh one.

    python scripts/mpc_expect_bench.py --parent PATH_TO_A_BUILT_TREE_OF_THE_PARENT_REVISION [--out FILE] [--rounds 3]
    python scripts/mpc_expect_bench.py --one VARIANT N [--root TREE]       # one process, one JSON line

The claim to check: (b) lies inside (a)'s own min-max spread (the existing instantiations kept their instruction streams).
The figure to report: (c) - (b), the expected agent against the chain agent on the same task -- the same sweep without the
episode key and the Philox blocks of the units, on another trajectory (the agents act differently)."""
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


def one(variant, N, root):
    sys.path.insert(0, root)
    import torch

    from gym_anm_amd import agents
    from gym_anm_amd.envs.anm6 import ANM6EasyVec

    env = ANM6EasyVec(num_envs=E, device=DEV, seed=3, tol=1e-6, exogenous="series_noise", exo_noise=2.0, exo_corr=0.8, autoreset=True)
    env.check_actions = False
    env.reset()
    Agent = {"chain": "MPCAgentPerfectChain", "expect": "MPCAgentExpected"}[variant]
    ag = getattr(agents, Agent)(env.simulator, env.action_space, env.gamma, safety_margin=0.92, planning_steps=N)
    ag.warn_unconverged, ag.reuse_action_buffer = False, True
    assert ag._fused(env)
    for _ in range(3):                               # a few real steps: the batch is spread over its episodes
        env.step(ag.act(env).clone())
    runs = []
    for _ in range(3):
        for _ in range(20):
            ag.act(env)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(200):
            ag.act(env)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / 200)
    print(json.dumps(dict(variant=variant, N=N, ms=runs, iters=float(ag.solver.iters.double().mean()),
                          converged=float(ag.last_converged.double().mean()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("VARIANT", "N"))
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], int(args.one[1]), os.path.abspath(args.root))
    if not args.parent:
        ap.error("--parent: a built tree of the parent revision")
    variants = [("a", "chain", os.path.abspath(args.parent)), ("b", "chain", ROOT), ("c", "expect", ROOT)]
    res = {}

    def run(tag, variant, root, N):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", variant, str(N), "--root", root]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
        if p.returncode != 0:
            sys.exit("%s failed (%d): %s" % (" ".join(cmd), p.returncode, p.stderr[-2000:]))   # (nothing more is started)
        r = json.loads(p.stdout.strip().split("\n")[-1])
        res.setdefault((N, tag), []).extend(r["ms"])
        res[(N, tag, "iters")] = r["iters"]
        print(tag, N, ["%.4f" % x for x in r["ms"]], flush=True)

    cases = (1, 10)
    for _ in range(args.rounds):
        for N in cases:
            for tag, variant, root in variants:
                run(tag, variant, root, N)
    lines = ["# scripts/mpc_expect_bench.py: ms per act() of %d ANM6Easy environments (series-noise mode, amplitude 2 MW, exo_corr=0.8); HIP" % E,
             "# events around 200 calls after 20, three timed runs per process, %d rounds of alternated fresh processes on one card: median" % args.rounds,
             "# [min - max] of the %d runs.  a: MPCAgentPerfectChain at the parent revision, b: at this revision, c: MPCAgentExpected at" % (3 * args.rounds),
             "# this revision (one launch)",
             "%3s  %-26s %-26s %-26s %9s %12s %8s %8s" % ("N", "a", "b", "c", "c - b", "b inside a", "iters b", "iters c")]
    for N in cases:
        def cell(tag):
            v = res[(N, tag)]
            return "%.4f [%.4f - %.4f]" % (statistics.median(v), min(v), max(v))
        a, b, c = (res[(N, t)] for t in "abc")
        inside = min(a) <= statistics.median(b) <= max(a)
        lines.append("%3d  %-26s %-26s %-26s %9.4f %12s %8.1f %8.1f" % (
            N, cell("a"), cell("b"), cell("c"), statistics.median(c) - statistics.median(b), "yes" if inside else "NO",
            res[(N, "b", "iters")], res[(N, "c", "iters")]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
