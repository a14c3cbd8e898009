"""CPU tier: the specification of the in-kernel episode time limit, truncation flag and episode statistics
(gym_anm_amd/episode.py) against hand-worked sequences, what the constructors refuse, and the register budgets of the kernel
the feature adds.  The GPU tier (tests/test_gpu_episode.py) holds the kernels to this specification."""
import os

import numpy as np
import pytest

from gym_anm_amd import codegen, episode, errors, networks, rng
from gym_anm_amd.envs import ANM6EasyVec
from gym_anm_amd.model import NetworkModel

from hostsim_backend import hostsim_backend

G = 0.5        # a discount whose powers are exact: the hand-worked numbers below are exact too


def run(tr, calls, autoreset):
    """calls: (reward, terminated_out[, reset_converged]) per step call; returns the events"""
    term, events = False, []
    for c in calls:
        ev, term = tr.call(term, autoreset, c[0], c[1], *(c[2:]))
        events.append(ev)
    return events


def test_limit_reached_with_autoreset():
    tr = episode.EpisodeTracker(G, 3)
    ev = run(tr, [(-1.0, False), (-2.0, False), (-4.0, False)], True)
    assert ev == ["step"] * 3
    assert tr.truncated and tr.timestep == 3 and tr.n_done == 1
    assert (tr.last_ret, tr.last_disc_ret, tr.last_len) == (-7.0, -1.0 - 1.0 - 1.0, 3)
    assert (tr.ret, tr.disc_ret, tr.discount) == (-7.0, -3.0, 0.125)          # running values: cleared by the reset, not here
    ev = run(tr, [(-99.0, False)], True)                                       # the call after: re-initialised, action ignored
    assert ev == ["reset"] and not tr.truncated and tr.timestep == 0
    assert (tr.ret, tr.disc_ret, tr.discount) == (0.0, 0.0, 1.0)
    assert (tr.last_ret, tr.last_disc_ret, tr.last_len, tr.n_done) == (-7.0, -3.0, 3, 1)
    ev = run(tr, [(-8.0, False)], True)
    assert ev == ["step"] and (tr.ret, tr.disc_ret, tr.discount, tr.timestep) == (-8.0, -8.0, 0.5, 1) and tr.n_done == 1


def test_collapse_before_the_limit():
    tr = episode.EpisodeTracker(G, 5)
    term, evs = False, []
    for r, t_out in [(-1.0, False), (-200.0, True)]:
        ev, term = tr.call(term, True, r, t_out)
        evs.append(ev)
    assert evs == ["step", "step"] and term and not tr.truncated
    assert (tr.last_ret, tr.last_disc_ret, tr.last_len, tr.n_done) == (-201.0, -101.0, 2, 1)
    ev, term = tr.call(term, True, -1.0, False)
    assert ev == "reset" and not term and tr.timestep == 0 and tr.n_done == 1


def test_collapse_exactly_at_the_limit_sets_both_flags_and_counts_one_episode():
    tr = episode.EpisodeTracker(G, 2)
    term = False
    _, term = tr.call(term, True, -1.0, False)
    _, term = tr.call(term, True, -200.0, True)
    assert term and tr.truncated and tr.n_done == 1 and tr.last_len == 2 and tr.last_ret == -201.0
    ev, term = tr.call(term, True, 0.0, False)
    assert ev == "reset" and tr.n_done == 1 and not tr.truncated


def test_stepping_past_the_limit_without_autoreset_counts_one_episode():
    tr = episode.EpisodeTracker(G, 2)
    ev = run(tr, [(-1.0, False)] * 6, False)
    assert ev == ["step"] * 6                                # keeps being stepped: TimeLimit
    assert tr.truncated and tr.timestep == 6 and tr.n_done == 1
    assert (tr.last_ret, tr.last_disc_ret, tr.last_len) == (-2.0, -1.5, 2)
    assert tr.ret == -6.0 and tr.disc_ret == -(1 + .5 + .25 + .125 + .0625 + .03125)
    # ... and a collapse later on is a second end event; the absorbing steps after it are none
    ev, term = tr.call(False, False, -200.0, True)
    assert ev == "step" and term and tr.n_done == 2 and tr.last_len == 7
    for _ in range(3):
        ev, term = tr.call(term, False, -1.0, False)
        assert ev == "noop" and term
    assert tr.n_done == 2 and tr.timestep == 7 and tr.truncated and tr.ret == -206.0


def test_a_failed_reset_draw_counts_no_episode_and_is_retried():
    tr = episode.EpisodeTracker(G, 2)
    term = False
    for _ in range(2):
        _, term = tr.call(term, True, -1.0, False)
    assert tr.n_done == 1 and tr.truncated and not term
    ev, term = tr.call(term, True, -1.0, False, False)       # the draw does not converge: looks absorbing
    assert ev == "reset" and term and not tr.truncated and tr.timestep == 0 and tr.n_done == 1
    ev, term = tr.call(term, True, -1.0, False, True)        # drawn again at the next call
    assert ev == "reset" and not term and tr.n_done == 1
    assert (tr.ret, tr.disc_ret, tr.discount) == (0.0, 0.0, 1.0)
    ev, term = tr.call(term, True, -3.0, False)
    assert ev == "step" and tr.ret == -3.0 and tr.timestep == 1


def test_without_a_limit_only_collapses_end_episodes_and_nothing_truncates():
    tr = episode.EpisodeTracker(0.995)
    ev = run(tr, [(-0.1, False)] * 50, True)
    assert ev == ["step"] * 50 and not tr.truncated and tr.n_done == 0 and tr.timestep == 50
    # the discounted return is the fused recurrence, one rounding per step
    d, g = 0.0, 1.0
    for _ in range(50):
        d, g = rng.fma(g, -0.1, d), g * 0.995
    assert tr.disc_ret == d and tr.discount == g
    assert not episode.ended_on_entry(False, 10**6, None) and episode.ended_on_entry(True, 0, None)
    assert episode.ended_on_entry(False, 5, 5) and not episode.ended_on_entry(False, 4, 5)


@pytest.mark.parametrize("bad", [0, -1, 2.5, "7", True, 2**31])
def test_a_bad_limit_is_an_args_error(bad):
    with pytest.raises(errors.ArgsError, match="max_episode_steps"):
        episode.check_limit(bad)
    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    with pytest.raises(errors.ArgsError, match="max_episode_steps"):
        ANM6EasyVec(num_envs=4, device="cpu", _backend=be, max_episode_steps=bad)


def test_env_config_with_the_episode_fields():
    """anm_env_config: `tail` in the padding behind K, the episode fields behind exo_high; the struct that ends at exo_high
    (tests/test_exo_uniform_spec.py pins it) is a prefix of it and says tail = 0"""
    import ctypes as C

    from gym_anm_amd import _lib

    base, ext = _lib.EnvConfig, _lib.EnvConfigEpisode
    assert _lib.ENV_TAIL_NONE == 0 and _lib.ENV_TAIL_EPISODE == 1
    assert base.gamma.offset == 8 and base.K.offset == 0 and base.K.size == 4          # four bytes of padding: `tail`
    assert ext.max_episode_steps.offset == C.sizeof(base) == base.exo_high.offset + 8
    assert ext.episode.offset == ext.max_episode_steps.offset + 8 and C.sizeof(ext) == ext.episode.offset + 8
    for name, _ in base._fields_:
        assert getattr(ext, name).offset == getattr(base, name).offset, name

    def tail_of(cfg):
        return C.c_int32.from_address(C.addressof(cfg) + 4).value

    old = base(K=1, gamma=0.9)
    assert tail_of(old) == 0
    new = ext(K=1, gamma=0.9, max_episode_steps=7)
    assert tail_of(new) == 1 and new.K == 1 and new.gamma == 0.9 and new.max_episode_steps == 7 and not new.episode
    assert isinstance(new, base)                    # goes where anm_model_set_env's argtypes ask for an EnvConfig
    # the header declares the same layout
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "anm_mi355x.h")).read()
    body = text[text.index("typedef struct anm_env_config {"):text.index("} anm_env_config;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"(\w+)\s*;", body)
    assert members == ["K", "tail"] + [n for n, _ in base._fields_][1:] + ["max_episode_steps", "episode"]


def test_good_limits():
    assert episode.check_limit(None) is None and episode.check_limit(1) == 1 and episode.check_limit(np.int64(3000)) == 3000


def test_the_host_double_refuses_the_feature_instead_of_ignoring_it():
    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    with pytest.raises(errors.EnvInitializationError, match="GPU library"):
        ANM6EasyVec(num_envs=4, device="cpu", _backend=be, max_episode_steps=10)
    with pytest.raises(errors.EnvInitializationError, match="GPU library"):
        ANM6EasyVec(num_envs=4, device="cpu", _backend=be, episode_stats=True)
    env = ANM6EasyVec(num_envs=4, device="cpu", _backend=be)       # off by default: as before
    assert env.max_episode_steps is None and not env.episode_stats and not bool(env.truncated.any())
    assert env.episode_length is env.timestep


def test_the_mixed_batch_refuses_the_feature():
    from gym_anm_amd.envs import MixedBatchedANMEnv
    from gym_anm_amd.envs.anm6 import anm6easy_series

    tasks = [dict(network=networks.anm6_network(), series=anm6easy_series())]
    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv(tasks, [0, 0], max_episode_steps=5)
    with pytest.raises(errors.EnvInitializationError, match="batch views"):
        MixedBatchedANMEnv(tasks, [0, 0], episode_stats=True)


def test_budgets_of_the_episode_aware_fast_path_kernel():
    """k_step_rows_ep (the sibling of k_step_rows that anm_step_f64 picks when a limit or statistics are set): at most 256
    VGPRs and no scratch, like the kernel it stands in for, read from the built anm6 library"""
    import importlib.util

    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf in this image")
    lib = codegen.lib_path(codegen.topology_name(codegen.stock_topologies()["anm6"]))
    if not os.path.exists(lib):
        pytest.skip("library of anm6 not built here")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_stats", os.path.join(root, "scripts", "kernel_stats.py"))
    ks = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ks)
    have = ks.kernel_stats(lib)
    hits = {n: s for n, s in have.items() if "k_step_rows_ep<" in n}
    assert len(hits) == 2, sorted(hits)                       # the f64 and the f32 solve
    for n, s in hits.items():
        assert s["vgpr"] <= 256 and s["scratch_insts"] == 0 and s["vgpr_spill"] == 0, (n[:80], s)
    # the kernels that must not carry the feature keep their names (and with them their budgets in tests/test_abi.py)
    assert any("k_step_rows<double, false>" in n for n in have) and any("k_step_stragglers<double, true>" in n for n in have)
