"""CPU: the yardstick of the two-headed policy-gradient learners (tests/sigma_pg_reference.py) pinned with torch float64 autograd -- the four losses written out as the
reference writes them (ppo.jl:4-21, a2c.jl:4-15, reinforce.jl:4-13, bc.jl:10-18; entropy: policies.jl:348 without `dims`, :398 per column) and differentiated by autograd --
and the conditions under which the GPU comparison of tests/test_gpu_sigma_pg.py means something, asserted with the yardstick alone: the share of parameters an Adam-step
comparison leaves out, the clipped columns of the ppo cases, the clamp variants' rows. No GPU.
"""
import numpy as np
import pytest
import torch

import sigma_head_reference as SR
import sigma_pg_reference as PR


def _torch_loss(c, kind, flat, entropy_over_everything=True):
    """the loss from its definition; flat: a float64 leaf tensor"""
    dims, acts, ad, sc, B = c["dims"], c["acts"], c["ad"], c["ascale"], c["B"]
    h = torch.tensor(np.asarray(c["s"], np.float64)); off = 0
    for l in range(len(dims) - 1):
        n = dims[l + 1] * dims[l]
        W = flat[off:off + n].reshape(dims[l], dims[l + 1]).T; off += n      # column-major (out x in)
        b = flat[off:off + dims[l + 1]]; off += dims[l + 1]
        h = W @ h + b[:, None]
        h = torch.relu(h) if acts[l] == "relu" else torch.tanh(h) if acts[l] == "tanh" else h
    mu, ls = h[:ad], h[ad:]
    a = torch.tensor(np.asarray(c["a"], np.float64))
    if sc > 0:
        sg = torch.exp(torch.clamp(ls, -5.0, 2.0)); u = torch.atanh(torch.clamp(a / sc, float(np.float32(-1.0) + np.float32(1e-5)), float(np.float32(1.0) - np.float32(1e-5))))
    else:
        sg = torch.exp(ls); u = a
    lp = (-(u - mu) ** 2 / (2 * sg ** 2) - SR.C0 - ls)
    if sc > 0:
        lp = lp - 2 * (np.log(2.0) - u - torch.nn.functional.softplus(-2 * u))
    lp = lp.sum(0)
    A, old = (torch.tensor(x) for x in PR.columns(c, kind))
    le = float(np.float32(c["lambda_e"])) if kind != "reinforce" else 0.0
    if kind == "ppo":
        eps = np.float32(c["eps_clip"]); lo, hi = float(np.float32(1.0) - eps), float(np.float32(1.0) + eps)
        r = torch.exp(lp - old); p_loss = -torch.mean(torch.minimum(r * A, torch.clamp(r, lo, hi) * A))
    else:
        p_loss = -torch.mean(lp * A)
    if sc > 0:
        ent = torch.mean(SR.ENT0 + ls.sum(0))                           # [1 x B], then the mean
    else:
        ent = SR.ENT0 + (ls.sum() if entropy_over_everything else ls.sum() / B)      # one scalar over everything; its mean is itself
    return p_loss - le * ent


def _autograd(c, kind, **kw):
    flat = torch.tensor(np.asarray(c["p"], np.float64), requires_grad=True)
    loss = _torch_loss(c, kind, flat, **kw); loss.backward()
    return float(loss.detach()), flat.grad.numpy()


CASES = PR.STEP_CASES
IDS = ["%s-B%d-a%g%s" % (n, B, sc, "" if k is None else "-clamp%d" % k) for n, B, sc, k in CASES]


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_yardstick_equals_autograd(case, kind):
    name, B, sc, clamp = case; c = PR.batch(name, B, sc, kind, clamp)
    loss, info, g, _ = PR.pg_loss(c, kind); tl, tg = _autograd(c, kind)
    e_g = np.abs(g - tg).max() / np.abs(tg).max()
    print("%s %s: loss %.12g / %.12g, gradient error / scale %.2e" % (IDS[CASES.index(case)], kind, loss, tl, e_g))
    assert abs(loss - tl) <= 1e-9 * max(1.0, abs(tl)) and e_g <= 1e-9
    assert abs(info["grad_norm"] - np.sqrt(tg @ tg)) <= 1e-9 * np.sqrt(tg @ tg)


def test_the_scalar_entropy_of_the_plain_policy_is_a_sum_over_the_minibatch():
    """policies.jl:348: with lambda_e > 0 the plain policy's logSigma seed carries -lambda_e per column, not -lambda_e / B; the per-column reading is a different loss"""
    c = PR.batch("5-100-100-2x3", 37, 0.0, "ppo"); c["lambda_e"] = 0.1
    _, info, g, dz = PR.pg_loss(c, "ppo"); _, tg = _autograd(c, "ppo"); _, tg_mean = _autograd(c, "ppo", entropy_over_everything=False)
    l = info["l"]
    assert abs(info["entropy"] - (SR.ENT0 + l.sum())) < 1e-12 and abs(info["entropy"] - float(SR.entropy(c, c["s"]))) < 1e-9
    assert np.abs(g - tg).max() <= 1e-9 * np.abs(tg).max() and np.abs(g - tg_mean).max() > 1e-2 * np.abs(tg).max()
    c0 = dict(c); c0["lambda_e"] = 0.0; dz0 = PR.pg_loss(c0, "ppo")[3]
    assert np.allclose(dz[:3], dz0[:3], atol=0, rtol=0) and np.allclose(dz[3:] - dz0[3:], -float(np.float32(0.1)), rtol=0, atol=1e-15)
    cs = PR.batch("5-100-100-2x3", 37, 2.0, "ppo"); dzs = PR.pg_loss(cs, "ppo")[3]; cs0 = dict(cs); cs0["lambda_e"] = 0.0
    assert np.allclose(dzs[3:] - PR.pg_loss(cs0, "ppo")[3][3:], -float(np.float32(0.1)) / 37, rtol=0, atol=1e-15)      # squashed: the mean over the columns


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_cases_leave_out_at_most_a_quarter(case):
    name, B, sc, clamp = case; worst = 0.0
    for kind in PR.KINDS:
        c = PR.batch(name, B, sc, kind, clamp); share = PR.skipped_share(PR.pg_loss(c, kind)[2]); worst = max(worst, share)
        print("%s %s: left out %.4f" % (IDS[CASES.index(case)], kind, share))
        assert share <= 0.25, (kind, share)


def test_why_the_plain_cases_take_a_small_lambda_e_and_the_lone_relu_column_is_no_step_case():
    c = PR.batch("4-256-256-2x2", 37, 0.0, "ppo"); c["lambda_e"] = 0.1
    share = PR.skipped_share(PR.pg_loss(c, "ppo")[2]); print("plain 4-256-256-2x2 B=37 at lambda_e = 0.1: left out %.4f" % share)
    assert share > 0.25
    lone = PR.skipped_share(PR.pg_loss(PR.batch("3-64-64-2x1", 1, 2.0, "ppo"), "ppo")[2]); print("lone column on the relu 3-64-64-2x1: left out %.4f" % lone)
    assert lone > 0.25


@pytest.mark.parametrize("case", [x for x in CASES if x[1] > 1], ids=[i for x, i in zip(CASES, IDS) if x[1] > 1])      # (a lone column has no clip fraction to speak of)
def test_ppo_cases_clip_on_both_sides(case):
    name, B, sc, clamp = case
    c = PR.batch(name, B, sc, "ppo", clamp); info = PR.pg_loss(c, "ppo")[1]
    r, A = info["ratio"], info["weight"]; clipped = (r > 1.2) | (r < 0.8)
    print("%s: clip fraction %.3f, clipped columns with A > 0: %d, A < 0: %d" % (IDS[CASES.index(case)], info["clip_fraction"], (A[clipped] > 0).sum(), (A[clipped] < 0).sum()))
    assert 0.2 <= info["clip_fraction"] <= 0.8 and (A[clipped] > 0).any() and (A[clipped] < 0).any()


@pytest.mark.parametrize("k", (0, 1, 2))
def test_clamp_variants_have_rows_on_both_sides(k):
    c = PR.batch("5-100-100-2x3", 37, 2.0, "ppo", k); l = PR.pg_loss(c, "ppo")[1]["l"]
    assert (l < -5.0).any() and (l > 2.0).any() and np.abs(l + 5.0).min() > 1e-3 and np.abs(l - 2.0).min() > 1e-3


def test_chain_stops_at_the_first_kl_above_the_target():
    c = PR.batch("3-64-64-2x1", 257, 2.0, "ppo"); mbs = [np.arange(0, 128), np.arange(128, 256), np.arange(256, 257)]
    p, infos, _ = PR.pg_chain(c, "ppo", mbs); assert len(infos) == 3 and not np.array_equal(p, c["p"])
    kls = [i["kl"] for i in infos]; tk = 0.5 * (kls[0] + kls[1]) if kls[1] > kls[0] else kls[0] - 1e-6
    assert len(PR.pg_chain(c, "ppo", mbs, target_kl=tk)[1]) == (2 if kls[1] > kls[0] else 1)
