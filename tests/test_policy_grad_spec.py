"""CPU tier: the specification of the PPO gradient (gym_anm_amd/policy_grad.py) needs no device.
  1. ``backward`` against torch float64 autograd of the same loss (exact tanh and exp): the relative L2 error of the whole
     gradient vector is at most 4 x that of torch float32 autograd of the ``pi.evaluate`` formulation -- the margin
     test_evaluate_is_consistent_with_act grants the kernel's tanh32 and summation order over torch's;
  2. hand-built cases: one live row, n = 0, NaN padding, a row exactly at ratio = 1 + c, the partial boundaries;
  3. the limits and the refusals."""
import math

import numpy as np
import pytest
import torch

from gym_anm_amd import errors, policy, policy_grad as PG

F32, F64 = np.float32, np.float64


def bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x.view(np.int32)


def make_mb(B, D, A, seed, dead=()):
    g = np.random.default_rng(seed)
    mb = dict(obs=g.standard_normal((B, D)).astype(F32), actions=g.standard_normal((B, A)).astype(F32),
              logp=np.zeros(B, dtype=F32), values=(0.3 * g.standard_normal(B)).astype(F32),
              returns=g.standard_normal(B).astype(F32), adv=g.standard_normal(B).astype(F32), weight=np.ones(B, dtype=F32))
    for i in dead:
        mb["weight"][i] = 0
    return mb


def params_of(D, A, hidden, seed, scale=None):
    flat = policy.init_flat(D, A, hidden, -0.5, seed)
    g = np.random.default_rng(seed + 1)
    if scale is not None:
        flat = (scale * g.standard_normal(flat.shape[0])).astype(F32)
    flat[-A:] = np.linspace(-0.8, 0.1, A).astype(F32)
    # biases away from zero, so that they matter
    for net, i, kind, at, shape in policy.layout(D, A, hidden)[0]:
        if kind == "bias":
            flat[at:at + shape[0]] = (0.1 * g.standard_normal(shape[0])).astype(F32)
    return flat


def torch_loss_grad(flat, mb, D, A, hidden, activation, dtype, clip, vf_coef, ent_coef, vf_clip):
    """autograd of the loss of the issue in ``dtype`` on the CPU: ``(grad, clipped-branch-active mask, ratio)``"""
    fl = torch.tensor(np.asarray(flat, dtype=F64), dtype=dtype, requires_grad=True)
    fn = torch.tanh if activation == "tanh" else torch.relu
    at = {(net, i, kind): (o, shape) for net, i, kind, o, shape in policy.layout(D, A, hidden)[0]}

    def view(net, i, kind):
        o, shape = at[(net, i, kind)]
        return fl[o:o + int(np.prod(shape))].view(shape)

    def net_of(name, x):
        n = len(hidden) + 1
        for i in range(n):
            x = x @ view(name, i, "weight") + view(name, i, "bias")
            if i + 1 < n:
                x = fn(x)
        return x

    t = lambda k: torch.tensor(np.nan_to_num(np.asarray(mb[k], dtype=F64)), dtype=dtype)  # noqa: E731
    w = t("weight")
    live = w != 0
    x = t("obs")
    mean, v = net_of("actor", x), net_of("critic", x)[:, 0]
    ls = view("log_std", 0, "log_std")
    z = (t("actions") - mean) * torch.exp(-ls)
    half = 0.5 * math.log(2.0 * math.pi)
    logp = (-0.5 * z * z - ls - half).sum(dim=1)
    ratio = torch.exp(logp - t("logp"))
    adv, ret = t("adv"), t("returns")
    pg = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv)
    vi = (v - ret) ** 2
    if vf_clip is not None:
        vcl = t("values") + torch.clamp(v - t("values"), -vf_clip, vf_clip)
        vi = torch.max(vi, (vcl - ret) ** 2)
    vi = 0.5 * vi
    H = (ls + (0.5 + half)).sum()
    n = live.sum()
    loss = (torch.where(live, w * (pg + vf_coef * vi), torch.zeros_like(pg))).sum() / n - ent_coef * H
    loss.backward()
    r = ratio.detach()
    active = ((adv >= 0) & (r > 1 + clip)) | ((adv < 0) & (r < 1 - clip))
    return fl.grad.numpy().astype(F64), (active & live).numpy(), r.numpy(), float(loss.detach())


def rel_l2(x, ref):
    return float(np.linalg.norm(np.asarray(x, dtype=F64) - ref) / np.linalg.norm(ref))


# ---- 1. against float64 autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vf_clip", [None, 0.2], ids=["vfclip-off", "vfclip-on"])
@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_backward_against_float64_autograd(activation, vf_clip, capsys):
    B, D, A, hidden = 130, 18, 6, (64, 64)
    clip, vf_coef, ent_coef = 0.2, 0.5, 0.01
    dead = (7, 126, 127, 128, 129)
    flat = params_of(D, A, hidden, 3)
    par = policy.unpack(flat, D, A, hidden)
    mb = make_mb(B, D, A, 11, dead)
    for i in dead:                                          # what a dead row holds is never read
        mb["obs"][i], mb["adv"][i], mb["logp"][i] = np.nan, np.nan, np.nan
    ist = PG.inv_std_of(par["log_std"])
    logp_now = PG.backward(par, mb, np.ones(B, dtype=F32), ist, activation)["logp"]
    delta = np.array([0.5, 0.5, -0.5, -0.5, 0.5, -0.5, 0.05, -0.05], dtype=F32)[np.arange(B) % 8]
    sign = np.array([1, -1, -1, 1, 1, -1, 1, -1], dtype=F32)[np.arange(B) % 8]
    live = mb["weight"] != 0
    mb["logp"] = np.where(live, logp_now - delta, np.nan).astype(F32)
    mb["adv"] = np.where(live, sign * (0.2 + np.abs(mb["adv"])), np.nan).astype(F32)
    ratio = PG.ratio_of(PG.log_ratio(par, mb, ist, activation))
    got = PG.backward(par, mb, ratio, ist, activation, clip, vf_coef, ent_coef, vf_clip)
    ref, active64, r64, loss64 = torch_loss_grad(flat, mb, D, A, hidden, activation, torch.float64, clip, vf_coef, ent_coef, vf_clip)
    g32, _, _, _ = torch_loss_grad(flat, mb, D, A, hidden, activation, torch.float32, clip, vf_coef, ent_coef, vf_clip)
    lo, hi = F32(1) - F32(clip), F32(1) + F32(clip)
    active = live & (((mb["adv"] >= 0) & (ratio > hi)) | ((mb["adv"] < 0) & (ratio < lo)))
    for a in (active, active64):                            # at least a quarter of the rows clip, at least a quarter do not
        assert a.sum() >= B / 4 and (live & ~a).sum() >= B / 4
    assert np.array_equal(active, active64)
    e_spec, e_torch = rel_l2(got["grad"], ref), rel_l2(g32, ref)
    with capsys.disabled():
        print("\n  %s, vf_clip=%s: gradient against float64 autograd, relative L2: specification %.3g, torch float32 %.3g"
              % (activation, vf_clip, e_spec, e_torch))
    assert e_spec <= 4 * e_torch
    if vf_clip is not None:                                 # the clipped value branch is taken somewhere: it changes the gradient
        off = PG.backward(par, mb, ratio, ist, activation, clip, vf_coef, ent_coef, None)
        assert rel_l2(off["grad"], ref) > 1e-3 and off["stats"][2] < got["stats"][2]
    st = got["stats"]
    assert abs(st[0] - loss64) <= 1e-5 * max(1.0, abs(loss64)) and st[6] == B - len(dead) and st[7] == 0
    assert abs(st[5] - np.mean((np.abs(r64[live] - 1) > clip))) < 1e-6
    assert got["grad"].dtype == F32 and got["logp"].dtype == F32 and got["values"].dtype == F32
    assert not got["values"][list(dead)].any() and not got["logp"][list(dead)].any()
    critic = policy.forward(par, np.nan_to_num(mb["obs"]), np.zeros((B, A), F32), np.ones(A, F32), activation)["values"]
    assert np.array_equal(bits(got["values"][live]), bits(critic[live]))          # rule 1: the chains of act


# ---- 2. hand-built cases --------------------------------------------------------------------------------------------------------------
SMALL = dict(D=3, A=2, hidden=(32,))


def small(B, seed=5, dead=(), activation="tanh", **kw):
    D, A, hidden = SMALL["D"], SMALL["A"], SMALL["hidden"]
    par = policy.unpack(params_of(D, A, hidden, seed, scale=0.7), D, A, hidden)
    mb = make_mb(B, D, A, seed + 100, dead)
    ist = PG.inv_std_of(par["log_std"])
    mb["logp"] = (PG.backward(par, mb, np.ones(B, dtype=F32), ist, activation)["logp"] - F32(0.1)).astype(F32)
    return par, mb, ist


def run(par, mb, ist, ratio=None, **kw):
    ratio = PG.ratio_of(PG.log_ratio(par, mb, ist)) if ratio is None else ratio
    return PG.backward(par, mb, ratio, ist, **kw)


def rows(mb, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in mb.items()}


def test_exactly_one_live_row():
    par, mb, ist = small(40, dead=[i for i in range(40) if i != 17])
    got = run(par, mb, ist, vf_clip=0.3)
    alone = run(par, rows(mb, [17]), ist, vf_clip=0.3)
    assert got["stats"][6] == 1 and got["grad"].any()
    assert np.array_equal(bits(got["grad"]), bits(alone["grad"])) and np.array_equal(bits(got["stats"]), bits(alone["stats"]))
    assert np.array_equal(bits(got["logp"][17]), bits(alone["logp"][0])) and not np.delete(got["logp"], 17).any()


def test_empty_minibatch_is_all_plus_zero():
    par, mb, ist = small(33, dead=range(33))
    for k in ("obs", "actions", "logp", "values", "returns", "adv"):
        mb[k][:] = np.nan
    got = run(par, mb, ist, ratio=np.full(33, np.nan, dtype=F32), ent_coef=0.01, vf_clip=0.2)
    for k in ("grad", "stats", "logp", "values"):
        assert not bits(got[k]).any(), k                    # every word +0.0: nothing NaN, nothing -0.0


def test_nan_padding_rows_change_no_bit():
    dead = (0, 20, 31, 32, 38, 39)
    par, mb, ist = small(40, dead=dead)
    ratio = PG.ratio_of(PG.log_ratio(par, mb, ist))
    clean = run(par, mb, ist, ratio=ratio, ent_coef=0.01)
    for k in ("obs", "actions", "logp", "values", "returns", "adv"):
        mb[k][list(dead)] = np.nan
    ratio[list(dead)] = np.nan
    dirty = run(par, mb, ist, ratio=ratio, ent_coef=0.01)
    for k in ("grad", "stats", "logp", "values", "partials"):
        assert np.array_equal(bits(clean[k]), bits(dirty[k])), k
    mb["weight"][20] = 1                                    # a NaN row that counts poisons, as in torch
    assert np.isnan(run(par, mb, ist, ratio=ratio)["grad"]).all()


def test_a_row_exactly_at_the_clip_boundary_passes_its_gradient():
    par, mb, ist = small(1)
    hi, lo = F32(1) + F32(0.2), F32(1) - F32(0.2)
    actor = slice(0, policy.layout(**SMALL)[0][4][3])       # the actor's words: up to the critic's first weight
    for adv, edge, beyond in ((0.7, hi, np.nextafter(hi, F32(2))), (-0.7, lo, np.nextafter(lo, F32(0)))):
        mb["adv"][0] = adv
        at = run(par, mb, ist, ratio=np.array([edge], dtype=F32))
        past = run(par, mb, ist, ratio=np.array([beyond], dtype=F32))
        assert at["grad"][actor].any() and at["stats"][5] == 0
        assert not past["grad"][actor].any() and past["stats"][5] == 1
        assert np.array_equal(bits(at["grad"][actor.stop:-2]), bits(past["grad"][actor.stop:-2]))      # the critic does not care


def test_partial_boundaries_follow_the_documented_order():
    assert [PG.rows_per_partial(B) for B in (1, 32, 33, 16384, 16385, 32769, 65536, 65537, 1 << 24)] == [32, 32, 32, 32, 64, 128, 128, 256, 32768]
    par, mb, ist = small(65)
    R = 64
    ratio = PG.ratio_of(PG.log_ratio(par, mb, ist))
    full = {B: run(par, rows(mb, slice(0, B)), ist, ratio=ratio[:B], R=R) for B in (R - 1, R, R + 1)}
    assert [full[B]["partials"].shape[0] for B in (R - 1, R, R + 1)] == [1, 1, 2]
    # R + 1: the first partial is the chain over the first R rows, the second the last row alone; grad is their ordered sum
    last = run(par, rows(mb, [R]), ist, ratio=ratio[R:R + 1], R=R)
    assert np.array_equal(bits(full[R + 1]["partials"][0]), bits(full[R]["partials"][0]))
    assert np.array_equal(bits(full[R + 1]["partials"][1]), bits(last["partials"][0]))
    P = full[R]["grad"].shape[0]
    want, _ = PG.reduce_partials(full[R + 1]["partials"], par["log_std"], P, 0.5, 0.0)
    assert np.array_equal(bits(full[R + 1]["grad"]), bits(want))
    # R - 1 against R: one row more at the END of the chain; the chain over R - 1 rows is a prefix
    a, b = full[R - 1]["partials"][0], run(par, rows(mb, slice(0, R)), ist, ratio=ratio[:R], R=R)["partials"][0]
    assert not np.array_equal(bits(a), bits(b))
    split = run(par, rows(mb, slice(0, R + 1)), ist, ratio=ratio[:R + 1], R=32)       # another R: another order, the same mathematics
    assert split["partials"].shape[0] == 3
    assert np.allclose(split["grad"], full[R + 1]["grad"], rtol=1e-4, atol=1e-6)
    assert np.array_equal(bits(split["logp"]), bits(full[R + 1]["logp"]))


# ---- 3. limits and refusals -------------------------------------------------------------------------------------------------------------
def test_lds_plan_and_refusals():
    P = policy.layout(18, 6, (64, 64))[1]
    T = 64 * 64 + 6 * 64 + 64 * 64 + 2 * 64
    assert PG.grad_lds_floats(18, 6, (64, 64), 2) == P + T + 128 + 64 * (4 * 65 + 15) == 37645
    assert PG.grad_lds_floats(18, 6, (64, 64), 4) > policy.LDS_FLOATS >= PG.grad_lds_floats(18, 6, (64, 64), 2)
    assert PG.grad_lds_floats(18, 6, (32,), 4) <= policy.LDS_FLOATS and PG.grad_lds_floats(18, 6, (32, 96, 32), 1) == 42669
    assert PG.grad_lds_floats(18, 6, (128,), 2) <= policy.LDS_FLOATS and PG.grad_lds_floats(18, 6, (256,), 1) <= policy.LDS_FLOATS
    with pytest.raises(errors.ArgsError, match="backward pass"):
        PG.check_args(18, 6, (32, 96, 32), 64)
    ok = PG.check_args(18, 6, (64, 64), 65536, 0.2, 0.5, 0.0, None)
    assert ok == (65536, 0.2, 0.5, 0.0, None) and PG.check_args(18, 6, (64, 64), 1, vf_clip=0.0)[4] == 0.0
    assert PG.grad_lds_floats(18, 6, (96, 96), 1) > policy.LDS_FLOATS
    with pytest.raises(errors.ArgsError, match="backward pass"):
        PG.check_args(18, 6, (96, 96), 64)
    for kw, msg in ((dict(batch_size=0), "batch_size"), (dict(batch_size=(1 << 24) + 1), "batch_size"), (dict(batch_size=2.5), "batch_size"),
                    (dict(clip=0.0), "clip"), (dict(clip=float("nan")), "clip"), (dict(clip="x"), "clip"),
                    (dict(vf_coef=float("inf")), "vf_coef"), (dict(ent_coef=None), "ent_coef"), (dict(vf_clip=-0.1), "vf_clip"),
                    (dict(vf_clip=float("nan")), "vf_clip")):
        args = dict(batch_size=64, clip=0.2, vf_coef=0.5, ent_coef=0.0, vf_clip=None)
        args.update(kw)
        with pytest.raises(errors.ArgsError, match=msg):
            PG.check_args(18, 6, (64, 64), **args)
    with pytest.raises(errors.ArgsError):                   # the shape's own limits are policy.py's
        PG.check_args(18, 6, (48,), 64)
    par, mb, ist = small(4)
    for R in (0, 31, 48):
        with pytest.raises(errors.ArgsError, match="multiple of 32"):
            run(par, mb, ist, R=R)
