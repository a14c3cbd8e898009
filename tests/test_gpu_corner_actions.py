"""GPU tier: actions on the faces and corners of the action box, the three kernel families against the oracle
(tests/corner_common.py: 729 grid actions of {low, mid, high}^6 on ANM6Easy for 8 steps; the oracle replays every
environment once per module).  Measured on an MI355X: profiles/devmath_probe.txt."""
import pytest

import corner_common as cc

from gym_anm_amd.envs import ANM6EasyVec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ORACLE = {}


def _oracle(run):
    if "replay" not in _ORACLE:
        _ORACLE["replay"] = cc.oracle_replay(run)
    return _ORACLE["replay"]


@pytest.mark.parametrize("impl", ["thread", "radial", "mesh"])
def test_corner_actions_vs_oracle(impl):
    env = ANM6EasyVec(num_envs=cc.E, device=DEV, seed=cc.SEED, impl=impl)
    assert env.simulator.impl == impl and env.simulator.backend.device_type == "cuda"
    run = cc.run_env(env)
    cc.compare(run, _oracle(run), impl)
