"""Golden runs of the reference for the differential tests of tests/test_hostsim_parity.py: tests/golden/reference_runs.npz.

TEST INFRASTRUCTURE ONLY (needs the reference checkout, through oracle/ref_harness.py).  Usage::

    python oracle/make_golden_reference_runs.py

Runs each of those tests once with the reference's side live (``_reference_side`` of the test module): what the
UNMODIFIED reference returned -- trajectories (observation, reward, terminated per step), the state layout and the
spaces of an environment -- is recorded under the test's key, and the test's own comparison with this package's side
runs on it at the same time.
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_hostsim_parity as T  # noqa: E402


def main():
    T._RECORDING = {}
    T.test_observation_spaces_of_random_lists_equal_the_reference()
    for seed in [1, 3, 4]:
        T.test_list_observation_episode_equals_the_live_reference(seed)
    T.test_reference_example_simple_env_equals_the_live_reference()
    T.test_reference_example_custom_anm6_equals_the_live_reference()
    T.test_new_env_template_with_callable_observation_and_own_bounds_equals_the_live_reference()
    for case in [("mesh", 5, 51, 2), ("radial", 8, 52, 0), ("mesh", 9, 53, 3)]:
        T.test_random_task_on_a_random_network_equals_the_live_reference(*case)
    for case in [("mesh", 6, 61, 2), ("radial", 10, 62, 0)]:
        T.test_the_whole_state_dictionary_equals_the_live_reference(*case)
    T.test_bad_observation_specs_fail_like_the_live_reference()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reference_runs.npz"), **T._RECORDING)
    print("recorded %d arrays" % len(T._RECORDING))


if __name__ == "__main__":
    main()
