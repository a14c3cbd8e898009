"""GPU tier: the row continuation on TWO lanes per bus (group::newton_rows<.., PAIRS = true>: each replica of a bus forms one row of Lk,
Sc and Lr) against one lane per bus (PAIRS = false, row_continuation=2) and against lane groups (-1).  The contract
is bit-identity of every output, on every entry point that inlines group::continue_collective.

Where the diverging solves come from.  A series-mode step takes its loads from the task's table, the same for every
environment, and a transition clips a load to its device's range, so scaling the loads of chosen environments (the x 40 of
bench.transition_figure) has nothing to act on in an ANM6Easy step and makes no ANM6 transition hopeless.  What makes a
6-bus solve run to the cap is reactive power: with the three reactive set-points of the action (generators and storage
unit) at their lower bounds the solve diverges from almost every state.  The chosen environments get exactly that on top of
the seeded random actions, and every test asserts the counts it needs -- solves at the cap, wavefronts holding more than
four and exactly one -- on the one-lane run, so none can pass on a batch without stragglers.  The first of them is also run
on the host test double (CPU tier), which shows the counts are properties of the reference algorithm."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_common as pc  # noqa: E402

from gym_anm_amd import networks  # noqa: E402

DEV = "cuda"
SEED = 311
Q_COLS = [2, 3, 5]          # Q of the two generators and of the storage unit in the ANM6 action
NAMES = ("obs", "state", "reward", "e_loss", "penalty", "terminated", "nr_iters", "soc")
# 256 environments = four wavefronts: six chosen ones in the first, one in the second, three and two in the others
CHOSEN_256 = [3, 9, 17, 30, 41, 58, 70, 130, 131, 150, 200, 255]


def _actions(env, gen, chosen):
    """seeded uniform actions drawn on the host, the reactive set-points of the chosen environments at their lower bounds"""
    shim = types.SimpleNamespace(device="cpu", action_space=env.action_space, num_envs=env.num_envs)
    a = pc.uniform_actions(shim, gen)
    low = torch.as_tensor(env.action_space.low, dtype=a.dtype)
    for c in Q_COLS:
        a[chosen, c] = low[c]
    return a


def _stepped(device, E, chosen, steps, cap, seed=SEED, **kw):
    """every output of every step, and the solves at the cap per step and wavefront"""
    from gym_anm_amd.envs import ANM6EasyVec

    env = ANM6EasyVec(num_envs=E, device=device, seed=seed, tol=1e-6, max_iter=cap, autoreset=True, **kw)
    env.reset(seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    out, at_cap = [], []
    for _ in range(steps):
        obs, reward, term, _, _ = env.step(_actions(env, g, chosen).to(device))
        it = env.simulator.nr_iters
        at_cap.append((it == cap).cpu().view(-1, 64).sum(dim=1))
        out.append([x.clone() for x in (obs, env.state, reward, env.e_loss, env.penalty, term, it, env.simulator.soc)])
    return out, torch.stack(at_cap)


def _assert_stragglers(at_cap):
    """what the identity test needs of its batch: >= 16 solves at the cap, a wavefront with more than four, one with exactly one"""
    assert int(at_cap.sum()) >= 16 and bool((at_cap > 4).any()) and bool((at_cap == 1).any()), at_cap.tolist()


def _assert_same(a, b, what):
    for t, (xs, ys) in enumerate(zip(a, b)):
        for name, x, y in zip(NAMES, xs, ys):
            assert torch.equal(x, y), (what, t, name, int((x != y).sum()))


@pytest.mark.parametrize("cap", [100, 7])
def test_the_batch_holds_the_stragglers_the_gpu_test_asserts(cap):
    """CPU tier (host test double): the counts asserted on the GPU hold for the reference algorithm, whatever continues the solves"""
    from gym_anm_amd.model import NetworkModel
    from hostsim_backend import hostsim_backend

    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    _, at_cap = _stepped("cpu", 256, CHOSEN_256, 3, cap, _backend=be)
    _assert_stragglers(at_cap)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [100, 7])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_pairs_equal_one_lane_per_bus_and_groups_on_every_solve(precision, cap):
    """ANM6Easy, 256 environments, every solve handed over before its first iteration, 3 steps: one lane per bus (2), the
    default (pairs), always rows (1: pairs for every solve) and groups (-1), every output of every step bit for bit."""
    kw = dict(handoff_after=0, precision=precision)
    one, at_cap = _stepped(DEV, 256, CHOSEN_256, 3, cap, row_continuation=2, **kw)
    print("solves at the cap per step and wavefront:", at_cap.tolist())
    _assert_stragglers(at_cap)
    for rowc in (0, 1, -1):
        got, _ = _stepped(DEV, 256, CHOSEN_256, 3, cap, row_continuation=rowc, **kw)
        _assert_same(one, got, "row_continuation=%d" % rowc)


@pytest.mark.gpu
def test_pairs_equal_one_lane_per_bus_behind_the_default_hand_over():
    """4 096 environments, one step, the default hand-over (iteration 6): the default mode against one lane per bus"""
    chosen = [64 * w + k for w in range(0, 64, 3) for k in (5, 40)] + [64 * 7 + k for k in (1, 2, 3, 9, 17, 25, 33, 41, 49, 57, 60, 62)]
    one, at_cap = _stepped(DEV, 4096, chosen, 1, 100, row_continuation=2)
    print("solves at the cap:", int(at_cap.sum()), "most in a wavefront:", int(at_cap.max()))
    _assert_stragglers(at_cap)
    got, _ = _stepped(DEV, 4096, chosen, 1, 100)
    _assert_same(one, got, "default")


def _transition_and_reset(rowc_kw):
    """Simulator.transition on 128 uniform inputs (reactive set-points of the chosen rows at their lower bounds), and the
    reset of a 128-environment task, every solve handed over before its first iteration"""
    from gym_anm_amd.envs import ANM6EasyVec
    from gym_anm_amd.simulator import BatchedSimulator

    E, chosen = 128, [2, 19, 20, 37, 50, 63, 100]
    sim = BatchedSimulator(networks.anm6_network(), 0.25, 100, num_envs=E, device=DEV, tol=1e-6, max_iter=100, handoff_after=0, **rowc_kw)
    m = sim.model
    b = m.baseMVA
    g = torch.Generator(device="cpu").manual_seed(SEED)

    def U(lo, hi):
        lo, hi = torch.as_tensor(lo), torch.as_tensor(hi)
        return lo + (hi - lo) * torch.rand((E, lo.numel()), generator=g, dtype=torch.float64)

    pl, pp = U(m.dev_p_min[m.load_idx] * b, 0 * m.dev_p_min[m.load_idx]), U(0 * m.dev_p_max[m.gen_idx], m.dev_p_max[m.gen_idx] * b)
    ps, qs = U(m.dev_p_min[m.setp_idx] * b, m.dev_p_max[m.setp_idx] * b), U(m.dev_q_min[m.setp_idx] * b, m.dev_q_max[m.setp_idx] * b)
    soc = U(m.dev_soc_min[m.des_idx], m.dev_soc_max[m.des_idx])
    qs[chosen] = torch.as_tensor(m.dev_q_min[m.setp_idx] * b).to(qs.dtype)
    sim.soc.copy_(soc.to(DEV))
    sim.transition(*(x.to(DEV).contiguous() for x in (pl, pp, ps, qs)))
    torch.cuda.synchronize()
    out = [sim.full.clone(), sim.pfe_converged.clone(), sim.nr_iters.clone(), sim.soc.clone()]
    env = ANM6EasyVec(num_envs=E, device=DEV, seed=SEED, tol=1e-6, max_iter=100, handoff_after=0, **rowc_kw)
    obs, _ = env.reset(seed=SEED)
    torch.cuda.synchronize()
    return out + [obs.clone(), env.state.clone(), env.simulator.soc.clone()]


@pytest.mark.gpu
def test_transition_and_reset_give_the_same_bits():
    """Every word of every output, NaN included (float64 compared as int64): the default (pairs) and groups (-1) against one
    lane per bus (2).  Always rows (1) hands a solve to a row where the policy of 2 keeps it on a group up to iteration 12,
    and a solve that fails with NaN in that window carries the other SIGN in its NaN on a row than on a group: the fused
    fmac(D, -x, 1.0) of a row and the subtraction of a group agree in every number, not in the sign of a NaN.  That is a
    difference between rows and groups which the parent of this change shows on this very batch (row_continuation 1 against 0
    and -1: the 12 NaN words of environment 37, nr_iters 57), not one between pairs and one lane per bus, so for 1 a NaN word
    may differ from 2's in its sign bit and in nothing else."""
    one = _transition_and_reset(dict(row_continuation=2))
    at_cap = (one[2] == 100).cpu().view(-1, 64).sum(dim=1)
    print("transition: solves at the cap per wavefront:", at_cap.tolist())
    assert bool((at_cap > 4).any()) and bool(((at_cap >= 1) & (at_cap <= 4)).any()), at_cap.tolist()
    for kw in ({}, dict(row_continuation=1), dict(row_continuation=-1)):
        got = _transition_and_reset(kw)
        for k, (x, y) in enumerate(zip(one, got)):
            if x.dtype == torch.float64:
                nan = torch.isnan(x) & torch.isnan(y)
                x, y = x.view(torch.int64), y.view(torch.int64)
                if kw.get("row_continuation") == 1:
                    sign = torch.tensor(-2 ** 63, dtype=torch.int64, device=x.device)
                    y = torch.where(nan & ((x ^ y) == sign), x, y)
            assert torch.equal(x, y), (kw, k, int((x != y).sum()))


@pytest.mark.gpu
def test_a_diverging_solve_in_every_row_reaches_no_neighbour():
    """One wavefront, always rows, every solve handed over before its first iteration: 16 passes of four.  The diverging
    solves sit at ranks 0, 5, 10 and 15 -- row 0 of the first pass, row 1 of the second, row 2 of the third, row 3 of the
    fourth -- next to three converging solves each.  The other 60 environments are bit for bit what they are when benign
    (the seeded random) actions stand in the diverging ones' places."""
    bad = [0, 5, 10, 15]
    kw = dict(handoff_after=0, row_continuation=1, seed=42)   # (a seed at which these four diverge and nobody else does)
    with_it, at_cap = _stepped(DEV, 64, bad, 1, 100, **kw)
    without, none_at_cap = _stepped(DEV, 64, [], 1, 100, **kw)
    it = with_it[0][NAMES.index("nr_iters")].cpu()
    assert (it == 100).nonzero().flatten().tolist() == bad and int(none_at_cap.sum()) == 0, (it.tolist(), none_at_cap.tolist())
    keep = torch.ones(64, dtype=torch.bool, device=DEV)
    keep[bad] = False
    _assert_same([[x[keep] for x in with_it[0]]], [[x[keep] for x in without[0]]], "neighbours of the diverging solves")
