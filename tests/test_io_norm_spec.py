"""CPU tier: the specification of the running normalisation (gym_anm_amd/io_norm.py) against independent restatements --
the fixed tree against ``math.fsum``, the chunk merge against NumPy's two-pass moments, the return accumulator against
Gymnasium's ``NormalizeReward`` recurrence written out row by row -- and the arguments refused before a device is touched."""
import math

import numpy as np
import pytest

from gym_anm_amd import _lib, errors, io_norm, networks
from gym_anm_amd.envs.anm6 import anm6easy_series
from gym_anm_amd.envs.anm_env import BatchedANMEnv
from gym_anm_amd.model import NetworkModel


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 1000, 1025, 3001, 65536])
def test_tree_sum_against_fsum(n):
    """pairwise summation: |error| <= ceil(log2 n) * u * sum |leaf| to first order; the bound asserted is twice that"""
    g = np.random.default_rng(n)
    x = g.normal(3.0, 10.0, size=n) * 10.0 ** g.integers(-3, 4, size=n)
    got, want = float(io_norm.tree_sum(x)), math.fsum(x)
    bound = 2 * math.ceil(math.log2(n)) * 2.0 ** -53 * math.fsum(np.abs(x))   # (n = 1: the leaf itself, exactly)
    print("n=%d |err|=%.3g bound=%.3g" % (n, abs(got - want), bound))
    assert abs(got - want) <= bound
    # an array of columns is summed column by column, by the same tree
    y = np.stack([x, -x, x * x], axis=1)
    s = io_norm.tree_sum(y)
    assert s[0] == got and s[1] == -got and s[2] == float(io_norm.tree_sum(x * x))


@pytest.mark.parametrize("n", [1, 3, 64])
def test_a_column_of_negative_zeros_sums_to_positive_zero(n):
    y = np.full((n, 2), -0.0)
    y[:, 1] = 1.0
    s = io_norm.tree_sum(y + 0.0)
    assert s[0] == 0.0 and not np.signbit(s[0]) and s[1] == n
    # ... through an update: mean stays +0.0, the bias is never -0.0
    st = io_norm.initial_state(n, 2)
    z = np.zeros(n)
    sc, bi, _ = io_norm.update(st, y, z, z, z, z + 1, (np.ones(2), np.full(2, -0.0)), 1.0, 0.99)
    assert st["mean"][0] == 0.0 and not np.signbit(st["mean"][0]) and bi[0] == 0.0 and not np.signbit(bi[0])
    assert st["mean"][1] > 0 and bi[1] == 0.0 - st["mean"][1] * sc[1]
    assert st["cnt"] == io_norm.COUNT0 + n and st["n_updates"] == 1 and st["n_skipped"] == 0


def two_pass(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.array([math.fsum(c) for c in x.T]) / x.shape[0]
    v = np.array([math.fsum((c - mk) ** 2) for c, mk in zip(x.T, m)]) / x.shape[0]
    return m, v


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_merging_chunks_matches_two_pass_moments(f32):
    """rules 3-6 from identity tables, chunk after chunk, against the two-pass mean / variance of the concatenation.  The
    statistics start EMPTY here (cnt = 0): Gymnasium's prior of 1e-4 pseudo-observations is part of the state, not of the
    rules, and would sit 1e-4 / N above the tolerance."""
    g = np.random.default_rng(7)
    D = 5
    chunks = [g.normal([5.0, -300.0, 0.0, 1e-3, 1e6], [2.0, 0.5, 1.0, 1e-5, 10.0], size=(n, D)) for n in (1000, 37, 4096, 1, 333)]
    if f32:
        chunks = [c.astype(np.float32) for c in chunks]
    st = io_norm.initial_state(1, D)
    st["cnt"] = 0.0
    ident = (np.ones(D), np.full(D, -0.0))
    for c in chunks:
        n = c.shape[0]
        z = np.zeros(n)
        st["G"], st["t_seen"] = np.zeros(n), np.zeros(n, dtype=np.int32)
        io_norm.update(st, c, z, z, z, z, ident, 1.0, 0.99, reward_on=False)
    m, v = two_pass(np.concatenate(chunks).astype(np.float64))
    tol = 1e-5 if f32 else 1e-12
    em = np.abs(st["mean"] - m) / (np.abs(m) + np.sqrt(v))
    ev = np.abs(st["var"] - v) / (m * m + v)
    print("mean err %s\nvar err %s" % (em, ev))
    assert st["cnt"] == sum(c.shape[0] for c in chunks) and st["n_skipped"] == 0
    assert (em <= tol).all() and (ev <= tol).all()


def test_moments_in_the_stored_space_convert_back_to_raw():
    """rule 5 under tables that are not the identity: the same raw statistics, whatever map the rows went through"""
    g = np.random.default_rng(11)
    D, n = 3, 777
    raw = g.normal([50.0, -2.0, 0.25], [3.0, 0.1, 4.0], size=(n, D))
    scale, bias = np.array([0.3, 9.0, 0.25]), np.array([-15.0, 18.0, 0.0])
    st = io_norm.initial_state(n, D)
    st["cnt"] = 0.0
    z = np.zeros(n)
    io_norm.update(st, raw * scale + bias, z, z, z, z, (scale, bias), 1.0, 0.99, reward_on=False)
    m, v = two_pass(raw)
    # (the rounding of the map itself, u (|y| + |b|) / s per entry, is below 1e-14 of |m| + sqrt(v) for these tables)
    assert (np.abs(st["mean"] - m) <= 1e-12 * (np.abs(m) + np.sqrt(v))).all()
    assert (np.abs(st["var"] - v) <= 1e-12 * (m * m + v)).all()


def test_terminated_rows_and_an_empty_batch():
    D = 2
    st = io_norm.initial_state(4, D)
    y = np.array([[1.0, 2.0], [np.nan, 7.0], [3.0, 4.0], [5.0, 6.0]])
    term = np.array([0, 1, 0, 0])
    z = np.zeros(4)
    ident = (np.ones(D), np.full(D, -0.0))
    io_norm.update(st, y, z, term, z, z, ident, 1.0, 0.9, reward_on=False)   # the NaN sits in a row that does not count
    assert st["cnt"] == io_norm.COUNT0 + 3 and st["n_skipped"] == 0 and np.isfinite(st["mean"]).all()
    before = {k: np.array(v, copy=True) for k, v in st.items()}
    sc, bi, _ = io_norm.update(st, y, z, np.ones(4), z, z, ident, 1.0, 0.9, reward_on=False)   # n = 0: nothing changes
    assert all(np.array_equal(before[k], st[k]) for k in ("cnt", "mean", "var")) and st["n_updates"] == 2
    assert np.array_equal(sc, ident[0]) and np.array_equal(bi, ident[1])
    # a counted NaN: that column is skipped, the other updates
    sc, bi, _ = io_norm.update(st, y, z, z, z, z, ident, 1.0, 0.9, reward_on=False)
    assert st["n_skipped"] == 1 and st["mean"][0] == before["mean"][0] and st["mean"][1] != before["mean"][1]
    assert sc[0] == 1.0 and sc[1] != 1.0 and st["cnt"] == io_norm.COUNT0 + 7


def test_return_accumulator_against_the_recurrence_of_normalize_reward():
    """Gymnasium: ``ret = ret * gamma * (1 - done) + reward; rms.update(ret)`` per environment.  The script, one column per
    row: 0 runs on; 1 terminates at call 2, is autoreset at call 3 (timestep 0), runs on; 2 terminates at call 1 and stays
    absorbing (timestep frozen); 3 is truncated at call 2 and stepped past the limit; 4 terminates at call 1, its reset draw
    fails at call 2 (nothing changes), succeeds at call 3."""
    gamma = 0.9
    #            row:   0  1  2  3  4
    steps = [dict(ts=[1, 1, 1, 1, 1], term=[0, 0, 1, 0, 1], trunc=[0, 0, 0, 0, 0]),
             dict(ts=[2, 2, 1, 2, 1], term=[0, 1, 1, 0, 1], trunc=[0, 0, 0, 1, 0]),
             dict(ts=[3, 0, 1, 3, 0], term=[0, 0, 1, 0, 0], trunc=[0, 0, 0, 1, 0]),
             dict(ts=[4, 1, 1, 4, 1], term=[0, 0, 1, 0, 0], trunc=[0, 0, 0, 1, 0])]
    g = np.random.default_rng(3)
    rewards = [g.normal(-1.0, 0.5, size=5) for _ in steps]
    st = io_norm.initial_state(5, 1)
    rs = 1.0
    # the restatement: plain Python per row, Gymnasium's merge in plain arithmetic
    ret, seen = [0.0] * 5, [0] * 5
    mean, var, cnt = 0.0, 1.0, 1e-4
    for k, (s, r) in enumerate(zip(steps, rewards)):
        batch = []
        for e in range(5):
            if s["ts"][e] == seen[e]:
                continue                       # nothing happened to this environment in this call
            if s["ts"][e] == 0:
                ret[e], seen[e] = 0.0, 0       # an autoreset call: no reward was earned
                continue
            ret[e] = ret[e] * gamma + r[e]
            batch.append(ret[e])
            if s["term"][e] or s["trunc"][e]:
                ret[e] = 0.0                   # (ret * (1 - done) of the NEXT step, done here)
            seen[e] = s["ts"][e]
        stored = r * rs                        # what the step stores under the scale it used
        _, _, rs_new = io_norm.update(st, np.zeros((5, 1)), stored, s["term"], s["trunc"], s["ts"], (np.ones(1), np.zeros(1)),
                                      rs, gamma, obs_on=False)
        if batch:
            bm, bv, bn = np.mean(batch), np.var(batch), len(batch)
            d, tot = bm - mean, cnt + bn
            m2 = var * cnt + bv * bn + d * d * cnt * bn / tot
            mean, var, cnt = mean + d * bn / tot, m2 / tot, tot
        assert np.allclose(st["G"], ret, rtol=1e-14, atol=0) and list(st["t_seen"]) == seen, k
        assert st["rcnt"] == cnt, k
        assert abs(st["rmean"] - mean) <= 1e-12 * (abs(mean) + math.sqrt(var)) and abs(st["rvar"] - var) <= 1e-12 * (mean * mean + var), k
        assert abs(rs_new - 1 / math.sqrt(var + 1e-8)) <= 1e-12 * rs_new
        rs = rs_new
    assert st["n_updates"] == 4 and st["n_skipped"] == 0
    assert st["cnt"] == io_norm.COUNT0 and (st["mean"] == 0).all()     # the observation part was off: never touched


def test_tables_and_sizes():
    sc, bi = io_norm.tables(np.array([0.0, 2.0, -3.0]), np.array([1.0, 4.0, 0.0]), 1e-8)
    assert sc[0] == 1 / np.sqrt(1 + 1e-8) and bi[0] == 0.0 and not np.signbit(bi[0])
    assert bi[1] == 0.0 - 2.0 * sc[1] and sc[2] == 1 / np.sqrt(1e-8)
    assert io_norm.slab_doubles(1, 18) == 40 and io_norm.slab_doubles(256, 18) == 40 and io_norm.slab_doubles(1025, 3) == 50
    assert io_norm.slab_doubles(65536, 18) == 256 * 40 and io_norm.slab_doubles(262144, 18) == 1024 * 40
    assert io_norm.slab_doubles(262145, 18) == 257 * 40 and io_norm.slab_doubles(4194304, 3) == 4096 * 10   # (1024 rows a slab)
    assert "anm_model_io_norm_update" in _lib.ABI and "anm_model_io_norm_update" in _lib.GPU_ONLY and "anm_model_io_norm_tables" in _lib.GPU_ONLY


def test_arguments_refused_before_any_backend_is_touched():
    args = (networks.anm6_network(), "state", 1, 0.25, 0.995, 100)
    for kw, exc, word in ((dict(obs_norm="batch"), errors.ArgsError, "obs_norm"), (dict(reward_norm=True), errors.ArgsError, "reward_norm"),
                          (dict(obs_norm="running", obs_map="box"), errors.ArgsError, "obs_norm.*obs_map"),
                          (dict(reward_norm="running", reward_scale=0.5), errors.ArgsError, "reward_norm.*reward_scale"),
                          (dict(obs_norm="running", norm_eps=0.0), errors.ArgsError, "norm_eps"),
                          (dict(obs_norm="running", norm_eps="tiny"), errors.ArgsError, "norm_eps"),
                          (dict(reward_norm="running", norm_eps=float("nan")), errors.ArgsError, "norm_eps"),
                          (dict(obs_norm="running", variants=[networks.anm6_network()]), errors.EnvInitializationError, "obs_norm.*variants"),
                          (dict(reward_norm="running", track_full=True), errors.EnvInitializationError, "reward_norm.*track_full"),
                          (dict(obs_norm="running", fuse_observation=False, observation=[("dev_p", "all", "MW")]),
                           errors.EnvInitializationError, "obs_norm.*fuse_observation=False"),
                          (dict(obs_norm="running", observation=lambda s: s), errors.EnvInitializationError, "obs_norm.*callable")):
        kw = dict(kw)
        a = list(args)
        if "observation" in kw:
            a[1] = kw.pop("observation")
        with pytest.raises(exc, match=word):        # (device="cpu": building the simulator would raise HipExtensionError instead)
            BatchedANMEnv(*a, device="cpu", **kw)


def test_the_host_backend_and_the_mixed_environment_refuse_the_mode():
    from hostsim_backend import hostsim_backend

    from gym_anm_amd.envs import MixedBatchedANMEnv

    net = networks.anm6_network()
    be = hostsim_backend(NetworkModel(net, 0.25, 100).topology())
    assert be.device_type == "cpu" and not hasattr(be.lib, "anm_model_io_norm_update")
    kw = dict(aux_bounds=np.array([[0, 95]]), costs_clipping=(1, 100), num_envs=4, device="cpu", series=anm6easy_series(), _backend=be)
    for mode in (dict(obs_norm="running"), dict(reward_norm="running")):
        with pytest.raises(errors.EnvInitializationError, match="GPU library"):
            BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **mode, **kw)
        with pytest.raises(errors.EnvInitializationError, match="batch views"):
            MixedBatchedANMEnv([dict(network=net, series=anm6easy_series())], [0, 0], **mode)
        with pytest.raises(errors.EnvInitializationError, match="batch views"):
            MixedBatchedANMEnv([dict(network=net, series=anm6easy_series(), **mode)], [0, 0])
    env = BatchedANMEnv(net, "state", 1, 0.25, 0.995, 100, **kw)    # the default is today's interface
    assert env.obs_rms is None and env.ret_rms is None and env.io_map is None and env.norm_training
    with pytest.raises(errors.ArgsError, match="obs_norm or reward_norm"):
        env.norm_state()
