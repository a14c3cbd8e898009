"""CPU tier twin of tests/test_gpu_corner_actions.py: the same body (tests/corner_common.py) on the host test double of the
kernel templates -- actions on the faces and corners of the action box against the oracle."""
import corner_common as cc
from hostsim_backend import hostsim_backend

from gym_anm_amd import networks
from gym_anm_amd.envs import ANM6EasyVec
from gym_anm_amd.model import NetworkModel


def test_corner_actions_host_double_vs_oracle():
    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    run = cc.run_env(ANM6EasyVec(num_envs=cc.E, device="cpu", seed=cc.SEED, _backend=be))
    orc = cc.oracle_replay(run)
    cc.compare(run, orc, "host")
