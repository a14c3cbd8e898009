"""CPU tier: codegen.row_pair_plan -- the row layout with TWO lanes per bus (csrc/anm_group.hpp: newton_rows<.., PAIRS = true>), each
replica forming one row of Lk = Jpb Di, Sc = Lk Jbp and Lr = Lk r -- checked as DATA: when a pair plan exists, who sits in
the destination banks of every hand-over, and one trip's elimination and back substitution replayed from the tables in
NumPy (row_newbcast emulated with bank masks, every lane running every level, unused lanes seeded with NaN) against the
one-lane-per-bus replay of the same trip from codegen.row_plan: both replicas of every bus must end with the same bits."""
import re

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
    """the cases of tests/test_row_plan.py (the same generator) and two around the leaf rule"""
    topo = lambda net: NetworkModel(net, 0.25, 100).topology()  # noqa: E731
    out = {}
    for name, net in (("anm6", networks.anm6_network()), ("2bus", networks.two_bus_network()),
                      ("radial9_s35", networks.synthetic_radial_network(9, 35)),
                      ("radial12_s42", networks.synthetic_radial_network(12, 42))):
        n_bus, branches, _ = topo(net)
        out[name] = (n_bus, [tuple(b) for b in branches])
    out["3bus_chain"] = (3, [(0, 1), (1, 2)])
    out["3bus_star"] = (3, [(0, 1), (0, 2)])
    out["chain7"] = (7, [(i, i + 1) for i in range(6)])
    out["star6"] = (6, [(0, 1)] + [(1, i) for i in range(2, 6)])
    out["star7"] = (7, [(0, 1)] + [(1, i) for i in range(2, 7)])
    out["three_leaves"] = (5, [(0, 1), (1, 2), (1, 3), (1, 4)])   # a row plan, but no room for three replicas in the leaf bank
    out["two_leaves"] = (4, [(0, 1), (1, 2), (1, 3)])
    for n in (4, 5, 6, 7, 8, 10, 11, 12):
        for seed in (0, 1, 2):
            out["rnd%d_%d" % (n, seed)] = (n, _random_tree(n, np.random.default_rng(97 * n + seed), 0.25 * (seed % 2)))
    return out


CASES = _cases()


def _tree(n_bus, tt):
    maxch = tt["MAXCH"]
    ch = {b: [c for c in tt["CH"][b * maxch:(b + 1) * maxch] if c > 0] for b in range(1, n_bus)}
    return tt["PARENT"], ch, tt["HEIGHT"], tt["DEPTH"]


def _bank_lanes(mask):
    return [l for l in range(16) if (mask >> (l // 4)) & 1]


def _pair_plan_by_the_rules(n_bus, tt):
    """a row plan (at most 4 banks: one per bus with children, one per set of leaves of one parent, at most 4 leaves each), and
    no leaf set of more than 2: its bank holds the leaves and their replicas"""
    parent, ch, _, _ = _tree(n_bus, tt)
    inner = [b for b in range(1, n_bus) if ch[b]]
    leaf_sets = {}
    for b in range(1, n_bus):
        if not ch[b]:
            leaf_sets.setdefault(parent[b], []).append(b)
    return len(inner) + len(leaf_sets) <= 4 and all(len(v) <= 2 for v in leaf_sets.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_plan_exists_exactly_by_the_rules_and_places_the_replicas_by_them(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    rp, pp = codegen.row_plan(n_bus, tt), codegen.row_pair_plan(n_bus, tt)
    assert (pp is not None) == _pair_plan_by_the_rules(n_bus, tt), name
    if pp is None:
        return
    parent, ch, height, depth = _tree(n_bus, tt)
    assert pp["LANE"] == rp["LANE"] and pp["BANKS"] == rp["BANKS"]   # the same banks, replica 0 where the one lane was
    lanes = pp["LANE"][1:] + pp["LANE1"][1:]
    assert pp["LANE1"][0] == -1 and len(set(lanes)) == len(lanes) and all(0 <= l < 16 for l in lanes)
    for b in range(1, n_bus):
        l0, l1 = pp["LANE"][b], pp["LANE1"][b]
        assert l0 // 4 == l1 // 4, "replica 1 of bus %d left the bank" % b
        if ch[b]:
            assert l1 == l0 + 1
        for rep, l in ((0, l0), (1, l1)):
            w = pp["LP"][l]
            assert w & 0x7F == b and ((w >> 7) & 0x7F) - 1 == height[b] and ((w >> 14) & 0x7F) - 1 == depth[b] and (w >> 21) == rep
    assert all(pp["LP"][l] == 0 for l in range(16) if l not in lanes)
    # every value of every hand-over names its lane: rows 1 of Sc and Lr replica 1 of the child, everything else replica 0
    for k in ("PAR_SRC", "PAR_BANK", "PAR_OFF", "CH_BANK", "CH_OFF", "WS_SRC", "WS_BANK"):
        assert pp[k] == rp[k], k
    assert pp["CH_SRC0"] == rp["CH_SRC"]
    rep1 = {pp["LANE"][b]: pp["LANE1"][b] for b in range(1, n_bus)}
    assert pp["CH_SRC1"] == [rep1[l] for l in rp["CH_SRC"]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_destination_banks_hold_consumers_their_replicas_or_unused_lanes(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    pp = codegen.row_pair_plan(n_bus, tt)
    if pp is None:
        return
    parent, _, _, _ = _tree(n_bus, tt)
    bus_of = {l: b for lst in (pp["LANE"], pp["LANE1"]) for b, l in enumerate(lst) if b > 0}
    for n, m in zip(pp["PAR_SRC"], pp["PAR_BANK"]):
        assert 0 < m < 16 and all(parent[bus_of[l]] == bus_of[n] for l in _bank_lanes(m) if l in bus_of)
    for src in ("CH_SRC0", "CH_SRC1"):
        for n, m in zip(pp[src], pp["CH_BANK"]):
            assert 0 < m < 16 and all(bus_of[l] == parent[bus_of[n]] for l in _bank_lanes(m) if l in bus_of)
    for n, m in zip(pp["WS_SRC"], pp["WS_BANK"]):
        assert 0 < m < 16 and all(bus_of[l] == parent[bus_of[n]] for l in _bank_lanes(m) if l in bus_of)


def _bcast(dst, src, n, bank_mask, op):
    """row_newbcast:n with a bank mask: the lanes of the banks named take op(dst, src[n]); the rest keep dst"""
    out = dst.copy()
    ls = _bank_lanes(bank_mask)
    out[ls] = op(dst[ls], src[n])
    return out


def _inv(Dg):
    a, b, c, d = Dg
    r = 1.0 / (a * d - b * c)
    return [d * r, -b * r, -c * r, a * r]


def _replay(tt, plan, seed_of_lane, pairs):
    """One trip's elimination by height and back substitution by depth over one 16-lane row, every lane running every level
    and every depth (the unconditional schedule of newton_rows), from the plan's tables.  seed_of_lane: lane -> the bus whose
    values the lane starts with (unused lanes: NaN).  pairs: each lane forms the row of Lk, Sc and Lr its replica bit names, and
    a fold takes rows 0 from CH_SRC0 and rows 1 from CH_SRC1.  Returns Dg (4), r (2), Di (4) and the step (2), per lane."""
    vals = np.random.default_rng(5).uniform(0.5, 2.0, size=(64, 10)) * np.where(np.random.default_rng(6).uniform(size=(64, 10)) < 0.5, -1, 1)
    lane_vals = np.full((16, 10), np.nan)
    for l, b in seed_of_lane.items():
        lane_vals[l] = vals[b]
    Dg = [lane_vals[:, k].copy() + (8.0 if k in (0, 3) else 0.0) for k in range(4)]    # (diagonally dominant: pivots far from 0)
    r = [lane_vals[:, 4].copy(), lane_vals[:, 5].copy()]
    bpa, bpb = lane_vals[:, 6], lane_vals[:, 7]           # Jbp = {bpa, bpb, -bpb, bpa}
    Jbp = [bpa, bpb, -bpb, bpa]
    wr, nwi = lane_vals[:, 8], lane_vals[:, 9]            # Jpb = {-nwi, wr, -wr, -nwi}
    Jpb = [-nwi, wr, -wr, -nwi]
    rep = np.array([(w >> 21) & 1 for w in plan["LP"]], dtype=bool) if pairs else np.zeros(16, dtype=bool)
    ja, jb = np.where(rep, Jpb[2], Jpb[0]), np.where(rep, Jpb[3], Jpb[1])
    sub = lambda d, s: d - s  # noqa: E731
    Sc, Lr, S0, S1, L = None, None, None, None, None
    with np.errstate(all="ignore"):
        for h in range(tt["MAXH"] + 1):
            for i in range(plan["CH_OFF"][h], plan["CH_OFF"][h + 1]) if h > 0 else ():
                m = plan["CH_BANK"][i]
                if pairs:
                    n0, n1 = plan["CH_SRC0"][i], plan["CH_SRC1"][i]
                    Dg = [_bcast(Dg[0], S0, n0, m, sub), _bcast(Dg[1], S1, n0, m, sub), _bcast(Dg[2], S0, n1, m, sub), _bcast(Dg[3], S1, n1, m, sub)]
                    r = [_bcast(r[0], L, n0, m, sub), _bcast(r[1], L, n1, m, sub)]
                else:
                    n = plan["CH_SRC"][i]
                    Dg = [_bcast(Dg[k], Sc[k], n, m, sub) for k in range(4)]
                    r = [_bcast(r[k], Lr[k], n, m, sub) for k in range(2)]
            Di = _inv(Dg)
            if h < tt["MAXH"]:
                if pairs:
                    ka, kb = ja * Di[0] + jb * Di[2], ja * Di[1] + jb * Di[3]
                    S0, S1 = ka * Jbp[0] + kb * Jbp[2], ka * Jbp[1] + kb * Jbp[3]
                    L = kb * r[1] + ka * r[0]
                else:
                    Lk = [Jpb[0] * Di[0] + Jpb[1] * Di[2], Jpb[0] * Di[1] + Jpb[1] * Di[3],
                          Jpb[2] * Di[0] + Jpb[3] * Di[2], Jpb[2] * Di[1] + Jpb[3] * Di[3]]
                    Sc = [Lk[0] * Jbp[0] + Lk[1] * Jbp[2], Lk[0] * Jbp[1] + Lk[1] * Jbp[3],
                          Lk[2] * Jbp[0] + Lk[3] * Jbp[2], Lk[2] * Jbp[1] + Lk[3] * Jbp[3]]
                    Lr = [Lk[1] * r[1] + Lk[0] * r[0], Lk[3] * r[1] + Lk[2] * r[0]]
        for dd in range(1, tt["MAXD"] + 1):
            d = [Di[0] * r[0] + Di[1] * r[1], Di[2] * r[0] + Di[3] * r[1]]
            for i in range(plan["PAR_OFF"][dd], plan["PAR_OFF"][dd + 1]):
                n, m = plan["PAR_SRC"][i], plan["PAR_BANK"][i]
                ls = _bank_lanes(m)
                r0, r1 = r[0].copy(), r[1].copy()
                r0[ls] = (r[0][ls] - Jbp[0][ls] * d[0][n]) - Jbp[1][ls] * d[1][n]
                r1[ls] = (r[1][ls] - Jbp[2][ls] * d[0][n]) - Jbp[3][ls] * d[1][n]
                r = [r0, r1]
        d = [Di[0] * r[0] + Di[1] * r[1], Di[2] * r[0] + Di[3] * r[1]]
    return np.stack(Dg + r + Di + d)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_trip_on_pairs_gives_both_replicas_the_bits_of_one_lane_per_bus(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    rp, pp = codegen.row_plan(n_bus, tt), codegen.row_pair_plan(n_bus, tt)
    if pp is None:
        return
    one = _replay(tt, rp, {rp["LANE"][b]: b for b in range(1, n_bus)}, pairs=False)
    seed = {pp["LANE"][b]: b for b in range(1, n_bus)}
    seed.update({pp["LANE1"][b]: b for b in range(1, n_bus)})
    two = _replay(tt, pp, seed, pairs=True)
    assert np.isfinite(one[:, rp["LANE"][1:]]).all(), "the one-lane replay itself took something from an unused lane"
    for b in range(1, n_bus):
        want = one[:, rp["LANE"][b]]
        for l in (pp["LANE"][b], pp["LANE1"][b]):
            assert (two[:, l] == want).all(), (name, b, l, two[:, l], want)


def test_three_leaves_under_one_parent_have_no_pair_plan_and_the_stock_feeder_has_this_one():
    n_bus, branches = CASES["three_leaves"]
    tt = _tables(n_bus, branches)
    assert codegen.row_plan(n_bus, tt) is not None and codegen.row_pair_plan(n_bus, tt) is None
    n_bus, branches = CASES["star6"]
    assert codegen.row_pair_plan(n_bus, _tables(n_bus, branches)) is None
    n_bus, branches = CASES["two_leaves"]
    assert codegen.row_pair_plan(n_bus, _tables(n_bus, branches)) is not None
    n_bus, branches = CASES["anm6"]
    tt = _tables(n_bus, branches)
    pp = codegen.row_pair_plan(n_bus, tt)
    _, ch, _, _ = _tree(n_bus, tt)
    used = sorted(pp["LANE"][1:] + pp["LANE1"][1:])
    assert len(used) == 10 and sorted(len(bs) for bs in pp["BANKS"]) == [1, 1, 1, 2]
    for b in range(1, n_bus):
        assert pp["LANE1"][b] == pp["LANE"][b] + (1 if ch[b] else len([bs for bs in pp["BANKS"] if b in bs][0]))


def test_headers_carry_the_pair_plan():
    t = codegen.stock_topologies()
    h6, h30 = codegen.emit_header(t["anm6"]), codegen.emit_header(t["case30"])
    get = lambda h, name: [int(x, 0) for x in re.search(r"%s\[\d+\] = \{([^}]*)\}" % name, h).group(1).replace("u", "").split(",")]  # noqa: E731
    assert "T_ROW2 = 1" in h6 and "T_ROW2 = 0" in h30
    n_bus, branches, _ = t["anm6"]
    pp = codegen.row_pair_plan(n_bus, _tables(n_bus, [tuple(b) for b in branches]))
    for k in ("LANE1", "LP", "CH_SRC0", "CH_SRC1"):
        assert get(h6, "T_ROW2_" + k) == pp[k], k
    assert "T_ROW2 = 1" in codegen.emit_header(t["2bus"]) and "T_ROW2 = 0" in codegen.emit_header(t["3bus"])
