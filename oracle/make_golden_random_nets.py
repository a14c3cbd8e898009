"""Golden vectors of the reference on random networks: tests/golden/random_nets_{transitions,resets}.npz.

TEST INFRASTRUCTURE ONLY (needs the reference checkout, through oracle/ref_harness.py).  Usage::

    python oracle/make_golden_random_nets.py

``Simulator.transition`` (24 seeded inputs per network, ``make_golden.random_inputs`` with 15 % wild rows) and
``Simulator.reset(init_state)`` (24 seeded initial states, ``make_golden.run_resets``) of the UNMODIFIED reference on
the synthetic meshed and radial networks of tests/test_oracle_golden.py, which compares the oracle against them.  Keys
are ``<case>/<field>`` with ``<case> = <kind><n_bus>_s<seed>``, fields as in ``make_golden.run_transitions`` /
``run_resets``.
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402  (loads the reference)

from gym_anm_amd import networks  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TRANSITION_CASES = [("mesh", 4, 31, 1), ("mesh", 7, 32, 2), ("mesh", 11, 33, 4), ("mesh", 16, 34, 3), ("radial", 9, 35, 0),
                    ("radial", 18, 36, 0), ("mesh", 30, 37, 6)]
RESET_CASES = [("mesh", 6, 41, 2), ("radial", 12, 42, 0), ("mesh", 20, 43, 5)]


def case_id(kind, n_bus, seed):
    return "%s%d_s%d" % (kind, n_bus, seed)


def network(kind, n_bus, seed, n_chords):
    return networks.synthetic_meshed_network(n_bus, seed, n_chords) if kind == "mesh" else networks.synthetic_radial_network(n_bus, seed)


def main():
    out = {}
    for kind, n_bus, seed, n_chords in TRANSITION_CASES:
        net = network(kind, n_bus, seed, n_chords)
        P_load, P_pot, P_set, Q_set, soc0 = MG.random_inputs(net, 0.25, 100, 24, seed, wild_frac=0.15)
        g = MG.run_transitions(net, 0.25, 100, P_load, P_pot, P_set, Q_set, soc0)
        out.update({"%s/%s" % (case_id(kind, n_bus, seed), k): np.asarray(v) for k, v in g.items()})
    np.savez_compressed(os.path.join(GOLDEN, "random_nets_transitions.npz"), **out)
    out = {}
    for kind, n_bus, seed, n_chords in RESET_CASES:
        g = MG.run_resets(network(kind, n_bus, seed, n_chords), 0.25, 100, 24, seed)
        out.update({"%s/%s" % (case_id(kind, n_bus, seed), k): np.asarray(v) for k, v in g.items()})
    np.savez_compressed(os.path.join(GOLDEN, "random_nets_resets.npz"), **out)


if __name__ == "__main__":
    main()
