"""CPU tier: codegen.row_plan -- one Newton solve per 16-lane DPP row, one lane per bus, every hand-over a row_newbcast
instruction with a bank mask (csrc/anm_group.hpp: newton_rows) -- checked as DATA: the layout rules, and one trip's hand-overs
replayed from the emitted tables by a NumPy emulation of row_newbcast with distinct tagged values."""
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
    """the stock feeder, the 2-bus network, the 3-bus trees, every tree of tests/golden with <= 12 buses, random small trees"""
    topo = lambda net: NetworkModel(net, 0.25, 100).topology()  # noqa: E731
    out = {}
    for name, net in (("anm6", networks.anm6_network()), ("2bus", networks.two_bus_network()),
                      ("radial9_s35", networks.synthetic_radial_network(9, 35)),
                      ("radial12_s42", networks.synthetic_radial_network(12, 42))):
        n_bus, branches, _ = topo(net)
        out[name] = (n_bus, [tuple(b) for b in branches])
    out["3bus_chain"] = (3, [(0, 1), (1, 2)])
    out["3bus_star"] = (3, [(0, 1), (0, 2)])
    out["chain7"] = (7, [(i, i + 1) for i in range(6)])          # 5 buses with children + a leaf: 6 banks
    out["star6"] = (6, [(0, 1)] + [(1, i) for i in range(2, 6)])  # 4 leaves of one parent: a full bank
    out["star7"] = (7, [(0, 1)] + [(1, i) for i in range(2, 7)])  # 5 leaves of one parent: no plan
    for n in (4, 5, 6, 7, 8, 10, 11, 12):
        for seed in (0, 1, 2):
            out["rnd%d_%d" % (n, seed)] = (n, _random_tree(n, np.random.default_rng(97 * n + seed), 0.25 * (seed % 2)))
    return out


CASES = _cases()


def _tree(n_bus, tt):
    maxch = tt["MAXCH"]
    ch = {b: [c for c in tt["CH"][b * maxch:(b + 1) * maxch] if c > 0] for b in range(1, n_bus)}
    return tt["PARENT"], ch, tt["HEIGHT"], tt["DEPTH"]


def _banks_by_the_rules(n_bus, tt):
    """rules (a) - (c) stated on their own: a bank per bus with children, a bank per set of leaves of one parent (the slack
    included); a plan exists when that is at most 4 banks of at most 4 lanes"""
    parent, ch, _, _ = _tree(n_bus, tt)
    inner = [b for b in range(1, n_bus) if ch[b]]
    leaf_sets = {}
    for b in range(1, n_bus):
        if not ch[b]:
            leaf_sets.setdefault(parent[b], []).append(b)
    ok = len(inner) + len(leaf_sets) <= 4 and all(len(v) <= 4 for v in leaf_sets.values())
    return ok, inner, leaf_sets


def _bank_lanes(mask):
    return [l for l in range(16) if (mask >> (l // 4)) & 1]


def _newbcast(dst, src, n, bank_mask, op):
    """row_newbcast:n with a bank mask over one 16-lane row: lane l of the banks named takes op(dst[l], src[n]); the rest keep dst"""
    out = list(dst)
    for l in _bank_lanes(bank_mask):
        out[l] = op(dst[l], src[n])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_plan_exists_exactly_by_the_rules_and_lays_the_buses_out_by_them(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    assert tt is not None
    ok, inner, leaf_sets = _banks_by_the_rules(n_bus, tt)
    rp = codegen.row_plan(n_bus, tt)
    assert (rp is not None) == ok, (name, inner, leaf_sets)
    if rp is None:
        return
    parent, ch, height, depth = _tree(n_bus, tt)
    lane = rp["LANE"]
    assert lane[0] == -1 and sorted(lane[1:]) == sorted(set(lane[1:])) and all(0 <= l < 16 for l in lane[1:])
    by_bank = {}
    for b in range(1, n_bus):
        by_bank.setdefault(lane[b] // 4, []).append(b)
    for k, bs in by_bank.items():
        if any(ch[b] for b in bs):
            assert len(bs) == 1, "rule (a): a bus with children shares bank %d: %s" % (k, bs)
        else:
            assert len({parent[b] for b in bs}) == 1, "rule (b): leaves of several parents in bank %d: %s" % (k, bs)
    # the packed row of every lane
    for l in range(16):
        w = rp["LP"][l]
        b = w & 0x7F
        assert (b == 0 and w == 0) if l not in lane[1:] else (lane[b] == l)
        if b:
            assert ((w >> 7) & 0x7F) - 1 == height[b] and ((w >> 14) & 0x7F) - 1 == depth[b]


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_trip_replayed_from_the_tables(name):
    n_bus, branches = CASES[name]
    tt = _tables(n_bus, branches)
    rp = codegen.row_plan(n_bus, tt)
    if rp is None:
        return
    parent, ch, height, depth = _tree(n_bus, tt)
    lane = rp["LANE"]
    bus_of = {lane[b]: b for b in range(1, n_bus)}
    maxh, maxd = tt["MAXH"], tt["MAXD"]
    assert len(rp["PAR_OFF"]) == maxd + 2 and len(rp["CH_OFF"]) == maxh + 2
    assert rp["PAR_OFF"][0] == 0 and rp["PAR_OFF"][-1] == len(rp["PAR_SRC"]) and (maxd == 0 or rp["PAR_OFF"][1] == 0)
    assert rp["CH_OFF"][0] == 0 and rp["CH_OFF"][-1] == len(rp["CH_SRC"]) and rp["CH_OFF"][1] == 0
    assert len(rp["WS_SRC"]) == len(rp["CH_SRC"])

    # rule (d), for every instruction: a bus lane inside the destination banks is an intended consumer
    for n, m in zip(rp["PAR_SRC"], rp["PAR_BANK"]):
        assert 0 < m < 16 and all(parent[bus_of[l]] == bus_of[n] for l in _bank_lanes(m) if l in bus_of)
    for n, m in list(zip(rp["CH_SRC"], rp["CH_BANK"])) + list(zip(rp["WS_SRC"], rp["WS_BANK"])):
        assert 0 < m < 16 and all(bus_of[l] == parent[bus_of[n]] for l in _bank_lanes(m) if l in bus_of)

    SLACK = -7.0                                          # "V = 1 + 0j": what a bus attached to the slack keeps
    tag = [float(1000 + 10 * l) for l in range(16)]       # what lane l holds: a distinct value per lane, bus or not
    # ---- the parent's voltage: every PAR pair, a move
    vp = [SLACK] * 16
    for n, m in zip(rp["PAR_SRC"], rp["PAR_BANK"]):
        vp = _newbcast(vp, tag, n, m, lambda d, s: s)
    for b in range(1, n_bus):
        assert vp[lane[b]] == (tag[lane[parent[b]]] if parent[b] > 0 else SLACK), (name, b)
    # ---- the W sums: every WS pair in table order; a bus receives each child once, in class order
    got = [[] for _ in range(16)]
    for n, m in zip(rp["WS_SRC"], rp["WS_BANK"]):
        got = _newbcast(got, tag, n, m, lambda d, s: d + [s])
    for b in range(1, n_bus):
        assert got[lane[b]] == [tag[lane[c]] for c in ch[b]], (name, b)
    # ---- the folds, level by level: each child once, at the level right after its own (where the group loop folds it),
    # a bus's folds in (level, class) order
    got = [[] for _ in range(16)]
    for h in range(1, maxh + 1):
        for i in range(rp["CH_OFF"][h], rp["CH_OFF"][h + 1]):
            got = _newbcast(got, tag, rp["CH_SRC"][i], rp["CH_BANK"][i], lambda d, s, h=h: d + [(h, s)])
    for b in range(1, n_bus):
        want = sorted((height[c] + 1, k) for k, c in enumerate(ch[b]))
        assert got[lane[b]] == [(h, tag[lane[ch[b][k]]]) for h, k in want], (name, b)
        assert all(h <= height[b] for h, _ in want)       # ... which is never after the bus's own pivot
    # ---- the back substitution, depth by depth: a bus receives its parent's step once, at its own depth
    got = [[] for _ in range(16)]
    for dd in range(1, maxd + 1):
        for i in range(rp["PAR_OFF"][dd], rp["PAR_OFF"][dd + 1]):
            got = _newbcast(got, tag, rp["PAR_SRC"][i], rp["PAR_BANK"][i], lambda d, s, dd=dd: d + [(dd, s)])
    for b in range(1, n_bus):
        assert got[lane[b]] == ([(depth[b], tag[lane[parent[b]]])] if parent[b] > 0 else []), (name, b)


def test_five_buses_with_children_have_no_plan_and_the_stock_feeder_has_this_one():
    n_bus, branches = CASES["chain7"]
    assert codegen.row_plan(n_bus, _tables(n_bus, branches)) is None
    n_bus, branches = CASES["star7"]
    assert codegen.row_plan(n_bus, _tables(n_bus, branches)) is None
    n_bus, branches = CASES["anm6"]
    tt = _tables(n_bus, branches)
    rp = codegen.row_plan(n_bus, tt)
    parent, ch, _, _ = _tree(n_bus, tt)
    inner = [b for b in range(1, n_bus) if ch[b]]
    assert len(inner) == 2 and len(rp["BANKS"]) == 4 and rp["BANKS"][:2] == [[b] for b in inner]
    # the root's voltage reaches both of its children's banks in ONE instruction
    assert rp["PAR_SRC"][0] == rp["LANE"][1] and bin(rp["PAR_BANK"][0]).count("1") == 2


def test_headers_carry_the_row_plan():
    t = codegen.stock_topologies()
    h6, h30 = codegen.emit_header(t["anm6"]), codegen.emit_header(t["case30"])
    get = lambda h, name: [int(x, 0) for x in re.search(r"%s\[\d+\] = \{([^}]*)\}" % name, h).group(1).replace("u", "").split(",")]  # noqa: E731
    assert "T_ROW = 1" in h6 and "T_ROW = 0" in h30
    n_bus, branches, _ = t["anm6"]
    rp = codegen.row_plan(n_bus, _tables(n_bus, [tuple(b) for b in branches]))
    for k in ("LANE", "LP", "PAR_SRC", "PAR_BANK", "PAR_OFF", "CH_SRC", "CH_BANK", "CH_OFF", "WS_SRC", "WS_BANK"):
        assert get(h6, "T_ROW_" + k) == rp[k], k
    assert "T_ROW_PAR_N = %d, T_ROW_CH_N = %d" % (len(rp["PAR_SRC"]), len(rp["CH_SRC"])) in h6
    for name in ("2bus", "3bus"):   # a 2-bus tree has a (trivial) plan, a loop has none
        assert ("T_ROW = 1" in codegen.emit_header(t[name])) == (name == "2bus")
