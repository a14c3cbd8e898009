"""CPU tier: the UNCONDITIONAL schedule of group::newton_rows (csrc/anm_group.hpp) replayed as data from codegen.tree_tables
and codegen.row_plan.  Every lane of a row -- bus or not, whatever its height and depth -- rewrites its hand-over values and
its inverted pivot at every level of the elimination and its Newton step at every depth of the back substitution; nothing is
a region.  What a lane writes is modelled as a VERSION: the exact sequence of folds (parent's steps) its operands held at
that moment, each fold carrying the version it read.  The kernel gives the bits of "pivot at my height, step at my depth"
when

  * every read of a source lane sees that bus's FINAL version (all the folds of its subtree, in the order of the lane-group
    loop; the step with its parent's final step in it, once), and
  * a bus's last write equals the one at its own level (depth): what it rewrites afterwards repeats it.

Trees: the stock feeder, the 2-bus network, the 3-bus chain and star, star6 and random trees of 4 to 12 buses."""
import numpy as np
import pytest

from gym_anm_amd import codegen, networks
from gym_anm_amd.model import NetworkModel


def _tables(n_bus, branches):
    pat = set()
    for f, t in branches:
        pat.update({(f, t), (t, f), (f, f), (t, t)})
    for i in range(n_bus):
        pat.add((i, i))
    return codegen.tree_tables(n_bus, branches, sorted(pat))


def _random_tree(n_bus, rng, p_slack):
    br = [(0, 1)]
    for i in range(2, n_bus):
        br.append((0 if rng.uniform() < p_slack else int(rng.integers(1, i)), i))
    return br


def _cases():
    topo = lambda net: NetworkModel(net, 0.25, 100).topology()  # noqa: E731
    out = {}
    for name, net in (("anm6", networks.anm6_network()), ("2bus", networks.two_bus_network())):
        n_bus, branches, _ = topo(net)
        out[name] = (n_bus, [tuple(b) for b in branches])
    out["3bus_chain"] = (3, [(0, 1), (1, 2)])
    out["3bus_star"] = (3, [(0, 1), (0, 2)])
    out["star6"] = (6, [(0, 1)] + [(1, i) for i in range(2, 6)])
    for n in range(4, 13):
        for seed in range(6 if n <= 8 else 3):    # (the larger the tree, the rarer a plan: at most 4 banks)
            out["rnd%d_%d" % (n, seed)] = (n, _random_tree(n, np.random.default_rng(131 * n + seed), 0.2 * (seed % 3)))
    return out


CASES = _cases()
MIN_WITH_PLAN = 20


def _bank_lanes(mask):
    return [l for l in range(16) if (mask >> (l // 4)) & 1]


def _replay(n_bus, tt, rp):
    """one trip of the unconditional schedule; returns the number of hand-over reads checked"""
    maxch, maxh, maxd = tt["MAXCH"], tt["MAXH"], tt["MAXD"]
    parent, height, depth = tt["PARENT"], tt["HEIGHT"], tt["DEPTH"]
    ch = {b: [c for c in tt["CH"][b * maxch:(b + 1) * maxch] if c > 0] for b in range(1, n_bus)}
    lane = rp["LANE"]
    bus_of = {lane[b]: b for b in range(1, n_bus)}

    # ---- what "final" means, from the tree alone
    def final_folds(b):   # the folds of b in the order of the lane-group loop: by (level, class)
        order = sorted((height[c] + 1, k) for k, c in enumerate(ch[b]))
        return tuple((lane[ch[b][k]], final_folds(ch[b][k])) for _, k in order)

    def final_step(b):
        return ("step", final_folds(b), (final_step(parent[b]),) if parent[b] > 0 else ())

    n_reads = 0
    # ---- elimination: folds[l] is what Dg / r0 / r1 of lane l have received; every lane rewrites pivot and hand-over
    folds = [() for _ in range(16)]
    handover = [None] * 16                      # Sc, Lr0, Lr1 of the lane: the version they were computed from
    w_pivot = [[] for _ in range(16)]           # the versions written, level by level
    w_handover = [[] for _ in range(16)]
    for h in range(maxh + 1):
        if h > 0:
            assert rp["CH_OFF"][h + 1] > rp["CH_OFF"][h]          # (the kernel static_asserts it: the lead needs a statement)
            for i in range(rp["CH_OFF"][h], rp["CH_OFF"][h + 1]):
                n, m = rp["CH_SRC"][i], rp["CH_BANK"][i]
                assert n in bus_of, "a hand-over names a lane without a bus as its source"
                assert handover[n] == final_folds(bus_of[n]), ("fold read at level %d sees a stale hand-over" % h, bus_of[n])
                n_reads += 1
                for l in _bank_lanes(m):
                    folds[l] = folds[l] + ((n, handover[n]),)
        for l in range(16):                     # EVERY lane: Di = inv(Dg); below the top level also Sc, Lr
            w_pivot[l].append(folds[l])
            if h < maxh:
                handover[l] = folds[l]
                w_handover[l].append(folds[l])
    for b in range(1, n_bus):
        l = lane[b]
        assert folds[l] == final_folds(b), b                       # each child once, in the order of the group loop
        assert w_pivot[l][-1] == w_pivot[l][height[b]] == final_folds(b), b
        if height[b] < maxh:
            assert w_handover[l][-1] == w_handover[l][height[b]] == final_folds(b), b
    # ---- back substitution: got[l] is the parents' steps r0 / r1 of lane l have received; the step d = Di r of EVERY lane is
    # rewritten in front of every depth's hand-over and once more after the last
    got = [() for _ in range(16)]
    step = [None] * 16
    w_step = [[] for _ in range(16)]

    def rewrite_steps():
        for l in range(16):
            step[l] = ("step", w_pivot[l][-1], got[l])
            w_step[l].append(step[l])

    for dd in range(1, maxd + 1):
        rewrite_steps()
        assert rp["PAR_OFF"][dd + 1] > rp["PAR_OFF"][dd]
        for i in range(rp["PAR_OFF"][dd], rp["PAR_OFF"][dd + 1]):
            n, m = rp["PAR_SRC"][i], rp["PAR_BANK"][i]
            assert n in bus_of, "a hand-over names a lane without a bus as its source"
            assert step[n] == final_step(bus_of[n]), ("step read at depth %d is not final" % dd, bus_of[n])
            n_reads += 1
            for l in _bank_lanes(m):
                got[l] = got[l] + (step[n],)
    rewrite_steps()
    for b in range(1, n_bus):
        l = lane[b]
        assert len(w_step[l]) == maxd + 1
        assert w_step[l][-1] == w_step[l][depth[b]] == final_step(b), b   # the parent's step exactly once, the final one
    return n_reads


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_read_sees_a_final_version_and_the_last_write_is_the_one_at_the_own_level(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    rp = codegen.row_plan(n_bus, tt)
    if rp is None:
        return                                                     # counted below
    n_reads = _replay(n_bus, tt, rp)
    n_children = sum(1 for b in range(1, n_bus) if tt["PARENT"][b] > 0)
    assert n_reads >= n_children + (1 if tt["MAXD"] > 0 else 0)   # a fold per child, a step per parent's instruction


def test_enough_of_the_trees_have_a_plan():
    with_plan = [nm for nm, (n_bus, br) in CASES.items() if codegen.row_plan(n_bus, _tables(n_bus, br)) is not None]
    without = sorted(set(CASES) - set(with_plan))
    print("%d trees with a plan, %d without: %s" % (len(with_plan), len(without), without))
    assert len(with_plan) >= MIN_WITH_PLAN
    assert {"anm6", "2bus", "3bus_chain", "3bus_star", "star6"} <= set(with_plan)


def test_the_replay_catches_a_region_that_is_needed():
    """the check has teeth: in the 4-bus chain, swap the two folds -- the child of height 1 is then read at level 1, while
    its hand-over still lacks its own child's fold, and the replay must say so"""
    n_bus, branches = 4, [(0, 1), (1, 2), (2, 3)]
    tt = _tables(n_bus, branches)
    rp = dict(codegen.row_plan(n_bus, tt))
    assert tt["MAXH"] == 2 and rp["CH_OFF"] == [0, 0, 1, 2]
    rp["CH_SRC"], rp["CH_BANK"] = rp["CH_SRC"][::-1], rp["CH_BANK"][::-1]
    with pytest.raises(AssertionError):
        _replay(n_bus, tt, rp)
