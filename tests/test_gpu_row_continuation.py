"""GPU tier: the handed-over Newton solves of a wavefront continue one per 16-lane DPP row (group::newton_rows, four a pass,
every hand-over one 64-bit row_newbcast instruction) or one per lane group (group::newton_groups, eight a pass for ANM6).
The contract is bit-identity: a solve gives the same iterate, iteration count and flags on either.  Checked here on every
solve of a stepped batch, on each branch of the policy that chooses between the two (group::continue_collective), for the
isolation of the four rows of a wavefront, and -- what localises a failure of the others -- for the two instructions
themselves.

The inputs are drawn on the host (CPU generators), so that the solve counts the tests assert -- solves that run to the cap,
slow converging ones, solves still running at iteration 6 and 12 -- are properties of the reference algorithm that the host
test double reproduces without a GPU (test_the_stepped_batch_holds_the_solves_the_gpu_test_asserts below does)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_common as pc  # noqa: E402

from gym_anm_amd import networks  # noqa: E402

DEV = "cuda"
CAP = 100
STEP_SEED, STEP_ENVS, STEP_T = 105, 200, 20   # seed chosen on the host test double: 23 solves at the cap, 8 slow converging ones
POOL_SEED, POOL_E = 11, 8192                  # random transitions: 59 at the cap, 7 that fail with NaN, 6 slow, on the host


def _host_actions(env, gen):
    """parity_common.uniform_actions drawn on the host (the same numbers wherever the batch runs)"""
    shim = types.SimpleNamespace(device="cpu", action_space=env.action_space, num_envs=env.num_envs)
    return pc.uniform_actions(shim, gen)


def _stepped(device, **kw):
    """every output of every step of the seeded batch, and the iteration counts of its solves"""
    from gym_anm_amd.envs import ANM6EasyVec

    env = ANM6EasyVec(num_envs=STEP_ENVS, device=device, seed=STEP_SEED, tol=1e-6, max_iter=CAP, autoreset=True, **kw)
    env.reset(seed=STEP_SEED)
    g = torch.Generator(device="cpu").manual_seed(STEP_SEED)
    out, n_cap, n_slow = [], 0, 0
    for _ in range(STEP_T):
        obs, reward, term, _, _ = env.step(_host_actions(env, g).to(device))
        it = env.simulator.nr_iters
        n_cap += int((it == CAP).sum())
        n_slow += int(((it > 6) & (it < CAP) & ~term).sum())
        out.append([x.clone() for x in (obs, env.state, reward, env.e_loss, env.penalty, term, env.simulator.soc, env.timestep, it,
                                        env._reset_count)])
    return out, n_cap, n_slow


def test_the_stepped_batch_holds_the_solves_the_gpu_test_asserts():
    """CPU tier (host test double): the seed of the rows-equal-groups test gives >= 8 solves at the cap and >= 8 that converge
    after iteration 6 -- for the reference algorithm, whatever continues them"""
    from gym_anm_amd.model import NetworkModel
    from hostsim_backend import hostsim_backend

    be = hostsim_backend(NetworkModel(networks.anm6_network(), 0.25, 100).topology())
    _, n_cap, n_slow = _stepped("cpu", _backend=be)
    assert n_cap >= 8 and n_slow >= 8, (n_cap, n_slow)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_rows_equal_groups_on_every_solve(precision):
    """Every solve of 200 environments (three full wavefronts and a ragged one) x 20 steps handed over before its first
    iteration: 16 passes of 4 on rows against 8 passes of 8 on groups, every output of every step bit for bit."""
    rows, n_cap, n_slow = _stepped(DEV, handoff_after=0, row_continuation=1, precision=precision)
    grps, n_cap_g, n_slow_g = _stepped(DEV, handoff_after=0, row_continuation=-1, precision=precision)
    names = ("obs", "state", "reward", "e_loss", "penalty", "terminated", "soc", "timestep", "nr_iters", "reset_count")
    for t, (a, b) in enumerate(zip(rows, grps)):
        for name, x, y in zip(names, a, b):
            assert torch.equal(x, y), (t, name, int((x != y).sum()))
    print("solves at the cap %d, slow converging %d" % (n_cap, n_slow))
    assert (n_cap, n_slow) == (n_cap_g, n_slow_g)
    if precision == "f64":
        assert n_cap >= 8 and n_slow >= 8, (n_cap, n_slow)


# ---------------------------------------------------------------------------------------------------
# transitions assembled from a pool of random inputs (as bench.transition_figure draws them)
# ---------------------------------------------------------------------------------------------------
def _sim(E, **kw):
    from gym_anm_amd.simulator import BatchedSimulator

    return BatchedSimulator(networks.anm6_network(), 0.25, 100, num_envs=E, device=DEV, tol=1e-6, max_iter=CAP, **kw)


def _run(inp, **kw):
    E = inp[0].shape[0]
    sim = _sim(E, **kw)
    pl, pp, ps, qs, soc = (x.to(DEV).contiguous() for x in inp)
    sim.soc.copy_(soc)
    sim.transition(pl, pp, ps, qs)
    torch.cuda.synchronize()
    return sim.full.clone(), sim.pfe_converged.clone(), sim.nr_iters.clone()


_POOL = {}


def _pool():
    """Random inputs, uniform over the devices' ranges, and what becomes of each on lane groups.  (The x 40 load trick of
    bench.transition_figure makes no ANM6 row hopeless -- the transition clips a load to its device's range -- so the
    hopeless rows of the tests below are the pool's own: the ~0.7 % of uniform inputs whose solve runs to the cap.)"""
    if not _POOL:
        m = _sim(1).model
        b = m.baseMVA
        g = torch.Generator(device="cpu").manual_seed(POOL_SEED)

        def U(lo, hi):
            lo, hi = torch.as_tensor(lo), torch.as_tensor(hi)
            return lo + (hi - lo) * torch.rand((POOL_E, lo.numel()), generator=g, dtype=torch.float64)

        inp = (U(m.dev_p_min[m.load_idx] * b, 0 * m.dev_p_min[m.load_idx]), U(0 * m.dev_p_max[m.gen_idx], m.dev_p_max[m.gen_idx] * b),
               U(m.dev_p_min[m.setp_idx] * b, m.dev_p_max[m.setp_idx] * b), U(m.dev_q_min[m.setp_idx] * b, m.dev_q_max[m.setp_idx] * b),
               U(m.dev_soc_min[m.des_idx], m.dev_soc_max[m.des_idx]))
        _, conv, it = _run(inp, row_continuation=-1)
        conv, it = conv.cpu(), it.cpu()
        pick = lambda mask: mask.nonzero().flatten()  # noqa: E731
        _POOL.update(inp=inp, hopeless=pick(it == CAP), blown=pick(~conv & (it > 6) & (it < CAP)), slow=pick(conv & (it > 6)),
                     benign=pick(conv & (it <= 5)))
        assert len(_POOL["hopeless"]) >= 9 and len(_POOL["blown"]) >= 1 and len(_POOL["benign"]) >= 256
    return _POOL


def _batch(E, placed):
    """E benign rows of the pool, with the pool rows of `placed` {row of the batch: row of the pool} in their places"""
    p = _pool()
    src = p["benign"][:E].clone()
    for row, k in placed.items():
        src[row] = k
    return tuple(x[src] for x in p["inp"])


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)


@pytest.mark.gpu
def test_the_branches_of_the_policy():
    """The policy (row_continuation = 0) against groups only (-1): `full` dump, converged and nr_iters bit for bit, on
    wavefronts that take each branch -- decided by how many solves are running at the hand-over (iteration 6) and at the
    intermediate limit (iteration 12), which the test reads from the groups-only run."""
    h = _pool()["hopeless"]
    W0, W1 = [5, 23, 60], [64, 77, 85, 98, 111, 127]
    # wavefront 0: 3 hopeless rows (n <= 4: rows);  wavefront 1: 6, spread over its lanes (n > 4, 6 survivors: groups to the cap)
    inp = _batch(128, {r: int(h[k]) for k, r in enumerate(W0 + W1)})
    ref = _run(inp, row_continuation=-1)
    it = ref[2].cpu()
    for rows, lo in ((W0, 0), (W1, 64)):
        w = it[lo:lo + 64]
        assert (w == CAP).nonzero().flatten().tolist() == [r - lo for r in rows]
        assert int((w > 6).sum()) == len(rows) and int((w > 12).sum()) == len(rows)
    _same(ref, _run(inp, row_continuation=0))
    _same(ref, _run(inp, row_continuation=1))
    # every solve handed over before its first iteration: 64 > 4 on groups up to iteration 12, then the 3 survivors on rows
    # (wavefront 1: nobody survives)
    inp = _batch(128, {r: int(h[k]) for k, r in enumerate(W0)})
    ref = _run(inp, row_continuation=-1, handoff_after=0)
    it = ref[2].cpu()
    assert (it == CAP).nonzero().flatten().tolist() == W0 and int((it > 12).sum()) == 3 and int((it[64:] > 12).sum()) == 0
    _same(ref, _run(inp, row_continuation=0, handoff_after=0))


@pytest.mark.gpu
def test_a_solve_that_blows_up_stays_in_its_row():
    """One wavefront, four handed-over solves in its four rows, one of which overflows to Inf / NaN: the other three -- two
    that run to the cap and a slow converging one where the pool has one -- are bit for bit what they are without it (and
    one row further up: the ranks of the solves behind it change)."""
    p = _pool()
    others = [int(p["hopeless"][0]), int(p["hopeless"][1]), int(p["slow"][0]) if len(p["slow"]) else int(p["hopeless"][2])]
    placed = {20: others[0], 30: others[1], 40: others[2]}
    with_it = _run(_batch(64, {**placed, 10: int(p["blown"][0])}), row_continuation=1)
    without = _run(_batch(64, placed), row_continuation=1)
    it = with_it[2].cpu()
    assert int((it > 6).sum()) == 4 and not bool(with_it[1][10]) and 6 < int(it[10]) < CAP
    keep = torch.ones(64, dtype=torch.bool, device=DEV)
    keep[10] = False
    _same([x[keep] for x in with_it], [x[keep] for x in without])


@pytest.mark.gpu
def test_the_two_row_newbcast_instructions_do_what_the_mapping_assumes():
    """anm_test_row_dpp: v_fmac_f64_dpp with -src / +src and a register of 1.0, and v_mov_b64_dpp, under bank masks, on one
    wavefront -- bitwise acc -/+ x[lane N of my row] on the banks named, acc untouched elsewhere; x and acc random with +-0,
    denormals, Inf and NaN among them (a NaN result is checked for being one: its payload is the hardware's choice)."""
    sim = _sim(1)
    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 5e-324, -2.5e-310, np.inf, -np.inf, np.nan, 1.0, -1.0, 1.7e308, -1.7e308, 2.2250738585072014e-308])

    def draw():
        v = rng.standard_normal(64) * 10.0 ** rng.integers(-300, 300, 64)
        k = rng.permutation(64)[:24]
        v[k] = special[rng.integers(0, len(special), 24)]
        return v

    lane = np.arange(64)
    row0, bank = lane - lane % 16, (lane % 16) // 4
    for trial in range(8):
        acc, x = draw(), draw()
        if trial == 0:
            x[[5, 21, 37, 53]] = [np.nan, np.inf, -0.0, 5e-324]   # the broadcast lane itself holds the special values
        d_acc, d_x = torch.as_tensor(acc, device=DEV), torch.as_tensor(x, device=DEV)
        out = torch.zeros(10, 64, dtype=torch.float64, device=DEV)
        sim.backend.check(sim.backend.lib.anm_test_row_dpp(d_acc.data_ptr(), d_x.data_ptr(), out.data_ptr(), None), "anm_test_row_dpp")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        src = lambda n: x[row0 + n]                                # noqa: E731  x of lane n of my row
        on = lambda mask: ((mask >> bank) & 1) == 1                # noqa: E731  my bank is named
        with np.errstate(all="ignore"):
            want = [
                np.where(on(0x5), acc + src(5), acc),
                np.where(on(0x5), acc - src(5), acc),
                np.where(on(0x1), acc - src(0), np.where(on(0x2), acc - src(7), acc - src(15))),
                np.where(on(0xA), src(12), acc), np.where(on(0xA), src(12), acc),
                np.where(on(0x8), acc - src(3), acc), np.where(on(0x8), acc - src(3), acc), np.where(on(0x8), acc - src(3), acc),
                np.where(on(0x3), (acc - 2.0 * src(9)) - 4.0 * src(9), acc),
                np.where(on(0x3), (acc - 16.0 * src(9)) - 8.0 * src(9), acc),
            ]
        for r, w in enumerate(want):
            w = np.asarray(w, dtype=np.float64)
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(got[r]), nan), (trial, r)
            assert np.array_equal(got[r][~nan].view(np.int64), w[~nan].view(np.int64)), (trial, r, np.nonzero(got[r] != w)[0][:8])
