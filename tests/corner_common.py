"""Actions on the faces and corners of the action box (shared by tests/test_gpu_corner_actions.py and its host-double twin
tests/test_corner_actions_spec.py).

Every replay elsewhere in the suite draws ``lo + (hi - lo) * rand``: no action ever lies on the boundary of the box.  A
policy whose output is clipped to the box sits there most of the time, and there project_pq (csrc/anm_device.hpp) works with
violated sets of measure zero, with ``lo == hi`` intervals and with a storage unit whose SoC window has closed.

ANM6EasyVec, 729 environments, reset(seed=3); environment e takes, at every one of 8 steps, the e-th point of
{low, (low + high) / 2, high}^6.  Each environment is replayed by OracleEnv(sparse=False) from its reset state and SoC."""
import itertools

import numpy as np
import numpy.testing as npt
import torch

E = 729
T = 8
SEED = 3


def corner_actions(space):
    lo, hi = np.asarray(space.low, dtype=np.float64), np.asarray(space.high, dtype=np.float64)
    assert lo.size == 6
    pts = np.stack((lo, (lo + hi) / 2, hi))                                             # [3, 6]
    acts = np.array([[pts[c[k], k] for k in range(6)] for c in itertools.product(range(3), repeat=6)])
    assert acts.shape == (E, 6)
    return acts


def run_env(env):
    """reset(seed=3) and 8 steps of the grid actions; everything as NumPy"""
    env.check_actions = False
    dev = env.state.device
    env.reset(seed=SEED)
    out = dict(state0=env.state.cpu().numpy().copy(), soc0=env.simulator.soc.cpu().numpy().copy(),
               acts=corner_actions(env.action_space), obs=[], rew=[], term=[], iters=[])  # fmt: skip
    a = torch.as_tensor(out["acts"], device=dev)
    for t in range(T):
        o, r, term, trunc, _ = env.step(a)
        out["obs"].append(o.cpu().numpy().astype(np.float64))
        out["rew"].append(r.cpu().numpy().astype(np.float64))
        out["term"].append(term.cpu().numpy().astype(bool))
        out["iters"].append(env.simulator.nr_iters.cpu().numpy().copy())
    return out


def oracle_replay(run):
    """The oracle on the same reset states and actions, and the conditions that make the inputs a test: the oracle meets no
    empty feasibility polygon (its projection asserts that; the assertion would surface here), between 20 and 100
    environments collapse, and at least one storage unit reaches SoC exactly 0."""
    import anm_oracle as O
    from gym_anm_amd import networks

    net = networks.anm6_network()
    obs = np.zeros((T, E, run["obs"][0].shape[1]))
    rew, term, iters = np.zeros((T, E)), np.zeros((T, E), dtype=bool), np.zeros((T, E), dtype=np.int64)
    soc_min = np.inf
    for e in range(E):
        orc = O.OracleEnv(net, sparse=False)
        orc.load_state(run["state0"][e], run["soc0"][e])
        for t in range(T):
            obs[t, e], rew[t, e], term[t, e] = orc.step(run["acts"][e])
            if term[t, e]:
                term[t:, e] = True            # absorbing: zero state, zero reward
                break
            iters[t, e] = orc.last["n_iter"]
            soc_min = min(soc_min, float(np.min(orc.soc)))
    n_collapsed = int(term[-1].sum())
    assert 20 <= n_collapsed <= 100, n_collapsed
    assert soc_min == 0.0, soc_min
    for a in (obs, rew, term, iters):
        a.setflags(write=False)
    return dict(obs=obs, rew=rew, term=term, iters=iters, n_collapsed=n_collapsed, state0=run["state0"], soc0=run["soc0"])


def compare(run, orc, tag):
    """the tolerances of test_gpu_parity.py::test_full_batch_vs_oracle_and_properties"""
    # the replay is shared: it started from the reset state of the first run, which every other run must have too -- the
    # SoC exactly, the state (MW) to 1e-10: its slack injection is the output of a solve stopped at the Newton tolerance,
    # which differs between kernel families in the last iterate's rounding (5e-12 measured), and the oracle's next step
    # does not read it
    npt.assert_allclose(run["state0"], orc["state0"], rtol=0, atol=1e-10)
    npt.assert_array_equal(run["soc0"], orc["soc0"])
    w_obs = w_rew = 0.0
    for t in range(T):
        w_obs = max(w_obs, float(np.abs(run["obs"][t] - orc["obs"][t]).max()))
        w_rew = max(w_rew, float(np.abs(run["rew"][t] - orc["rew"][t]).max()))
    print("corner actions: %-8s collapsed %d of %d, worst |obs diff| %.3g, worst |reward diff| %.3g"
          % (tag, int(run["term"][-1].sum()), E, w_obs, w_rew))  # fmt: skip
    for t in range(T):
        npt.assert_array_equal(run["term"][t], orc["term"][t], err_msg="terminated flags, step %d" % t)
        npt.assert_allclose(run["obs"][t], orc["obs"][t], rtol=0, atol=1e-7, err_msg="observations, step %d" % t)
        npt.assert_allclose(run["rew"][t], orc["rew"][t], rtol=1e-9, atol=1e-8, err_msg="rewards, step %d" % t)
        live = ~orc["term"][t]
        npt.assert_array_equal(run["iters"][t][live], orc["iters"][t][live], err_msg="Newton iterations, step %d" % t)
    return w_obs, w_rew
