"""Golden vectors of the reference's network front end: tests/golden/reference_constants.npz.

TEST INFRASTRUCTURE ONLY (needs the reference checkout, through oracle/ref_harness.py).  Usage::

    python oracle/make_golden_constants.py

What the UNMODIFIED reference's ``Simulator(network, 0.25, 100)`` (simulator.py:70-181, check_network.py:7-64,
components/*.py) makes of
* the stock networks of tests/test_model.py (keys ``<name>/<field>``), and
* the 400 single-field mutations of the 3-bus basics network that tests/test_model.py draws (``mutations/exception``:
  the class name of what the constructor raised, "" when it accepted the network; the accepted ones' fields one after the
  other in ``mutations/<field>``, each network's first-axis length in ``mutations/<field>_len``).
Fields: ``Y_bus``, ``bus_ids``, ``dev_ids``, ``branch_ids``, ``dev_kind`` (0 other, 1 generator, 2 storage unit), the
device limits, ``tau`` / ``rho`` (generators: columns 0-1; storage units: 0-3), ``soc`` (soc_min, soc_max, eff), the
branches' ``series``, ``shunt``, ``tap``, ``rate``; ``Simulator.state_bounds`` flattened in its own order
(``sb_quantities``; ``sb_ids``: (quantity, repr(id)); ``sb_units``: (quantity, repr(id), unit) with its (lo, hi) in
``sb_lohi``) and the action box of ``get_action_space()`` (``act_lo``, ``act_hi``: P_gen, Q_gen, P_des, Q_des, each
sorted by device id).
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_harness  # noqa: E402

ref_harness.load_reference()
from gym_anm.simulator import Simulator  # noqa: E402
from gym_anm.simulator.components import Generator, StorageUnit  # noqa: E402

import test_model as TM  # noqa: E402  (the networks and the mutation stream of the test)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _id(i):
    """a device / bus id or a branch's (from, to) as a Python literal"""
    return repr(tuple(int(x) for x in i) if isinstance(i, tuple) else int(i))


def constants(ref):
    devs = list(ref.devices.values())
    kind = [2 if isinstance(d, StorageUnit) else 1 if isinstance(d, Generator) else 0 for d in devs]
    tau, rho, soc = np.zeros((len(devs), 4)), np.zeros((len(devs), 4)), np.zeros((len(devs), 3))
    for k, d in enumerate(devs):
        if kind[k]:
            tau[k, :2], rho[k, :2] = (d.tau_1, d.tau_2), (d.rho_1, d.rho_2)
        if kind[k] == 2:
            tau[k, 2:], rho[k, 2:] = (d.tau_3, d.tau_4), (d.rho_3, d.rho_4)
            soc[k] = (d.soc_min, d.soc_max, d.eff)
    brs = list(ref.branches.values())
    out = {
        "Y_bus": ref.Y_bus.toarray(), "bus_ids": np.array(list(ref.buses.keys()), dtype=np.int64),
        "dev_ids": np.array(list(ref.devices.keys()), dtype=np.int64),
        "branch_ids": np.array(list(ref.branches.keys()), dtype=np.int64).reshape(-1, 2), "dev_kind": np.array(kind, dtype=np.int64),
        "dev_p_min": np.array([d.p_min for d in devs], dtype=np.float64), "dev_p_max": np.array([d.p_max for d in devs], dtype=np.float64),
        "dev_q_min": np.array([d.q_min for d in devs], dtype=np.float64), "dev_q_max": np.array([d.q_max for d in devs], dtype=np.float64),
        "tau": tau, "rho": rho, "soc": soc,
        "br_series": np.array([b.series for b in brs], dtype=np.complex128), "br_shunt": np.array([b.shunt for b in brs], dtype=np.complex128),
        "br_tap": np.array([b.tap for b in brs], dtype=np.complex128), "br_rate": np.array([b.rate for b in brs], dtype=np.float64),
    }  # fmt: skip
    rb = ref.state_bounds
    out["sb_quantities"] = np.array(list(rb), dtype=str)
    out["sb_ids"] = np.array([[q, _id(i)] for q in rb for i in rb[q]], dtype=str).reshape(-1, 2)
    units = [(q, i, unit, lo, hi) for q in rb for i in rb[q] for unit, (lo, hi) in rb[q][i].items()]
    assert all(isinstance(x, (float, int, np.floating, np.integer)) for u in units for x in u[3:]), "a bound that is not a number"
    out["sb_units"] = np.array([[q, _id(i), unit] for q, i, unit, _, _ in units], dtype=str).reshape(-1, 3)
    out["sb_lohi"] = np.array([[lo, hi] for _, _, _, lo, hi in units], dtype=np.float64).reshape(-1, 2)
    P_gen, Q_gen, P_des, Q_des = ref.get_action_space()
    out["act_lo"] = np.array([v[0] for x in (P_gen, Q_gen, P_des, Q_des) for _, v in sorted(x.items())], dtype=np.float64)
    out["act_hi"] = np.array([v[1] for x in (P_gen, Q_gen, P_des, Q_des) for _, v in sorted(x.items())], dtype=np.float64)
    # what the arrays hold is what the reference holds (ids are integers, every number survives the conversion)
    assert out["bus_ids"].tolist() == list(ref.buses.keys()) and out["dev_ids"].tolist() == list(ref.devices.keys())
    assert [tuple(b) for b in out["branch_ids"].tolist()] == list(ref.branches.keys())
    return out


def main():
    out = {}
    for which, net in TM.stock_networks().items():
        out.update({"%s/%s" % (which, k): v for k, v in constants(Simulator(net, 0.25, 100)).items()})
    names, packed = [], {}
    for i, net in enumerate(TM._mutations(np.random.default_rng(12), 400)):
        try:
            ref = Simulator(net, 0.25, 100)
        except Exception as ex:  # noqa: BLE001
            names.append(type(ex).__name__)
            continue
        names.append("")
        for k, v in constants(ref).items():
            packed.setdefault(k, []).append(v)
    out["mutations/exception"] = np.array(names, dtype=str)
    for k, vs in packed.items():  # the accepted ones' fields, one after the other (per network: its first-axis length)
        out["mutations/%s" % k] = np.concatenate(vs, axis=0)
        out["mutations/%s_len" % k] = np.array([len(v) for v in vs], dtype=np.int64)
    np.savez_compressed(os.path.join(GOLDEN, "reference_constants.npz"), **out)


if __name__ == "__main__":
    main()
