"""CPU: the float64 yardstick of MixtureNetwork (tests/mixture_reference.py) against torch float64 autograd and against itself.

Largest share of parameters left out of the Adam comparison over the step cases (test_adam_comparison_leaves_out_at_most_a_quarter): see its output; the cap is a
quarter per handle."""
import numpy as np
import pytest
import torch

import ensemble_reference as ER
import mixture_reference as MR

GRID = [(n, K, B) for n in MR.SHAPES for K in MR.KS for B in MR.BS]


def _torch_chain(flat, dims, acts, x):
    h, off = x, 0
    for l, a in enumerate(acts):
        n = dims[l + 1] * dims[l]
        W = flat[off:off + n].reshape(dims[l], dims[l + 1]).T; off += n      # column-major (out x in)
        b = flat[off:off + dims[l + 1]]; off += dims[l + 1]
        h = W @ h + b[:, None]
        h = torch.relu(h) if a == "relu" else torch.tanh(h) if a == "tanh" else h
    return h


def _torch_loss(c, w):
    """-mean(w * logsumexp(log alpha + l)) with autograd leaves for every handle"""
    f64 = torch.float64; nd = c["nd"]
    ps = [torch.tensor(np.asarray(p, np.float64), requires_grad=True) for p in c["ps"]]; wp = torch.tensor(np.asarray(c["wp"], np.float64), requires_grad=True)
    s, a = torch.tensor(np.asarray(c["s"], np.float64)), torch.tensor(np.asarray(c["a"], np.float64)); B = a.shape[1]
    w = torch.ones(B, dtype=f64) if w is None else torch.tensor(np.asarray(w, np.float64).reshape(-1))
    ls = []
    for p in ps:
        mu = _torch_chain(p[:-nd], c["dims"], c["acts"], s); lsg = p[-nd:][:, None]
        ls.append((-(a - mu) ** 2 / (2 * torch.exp(2 * lsg)) - MR.HALF_LOG_2PI - lsg).sum(0))
    la = torch.log(wp)[:, None].expand(-1, B) if c["wdims"] is None else torch.log_softmax(_torch_chain(wp, c["wdims"], c["wacts"], s), 0)
    lp = torch.logsumexp(la + torch.stack(ls), 0)
    loss = -(w * lp).mean(); loss.backward()
    return lp.detach().numpy(), float(loss.detach()), [p.grad.numpy() for p in ps], wp.grad.numpy()


@pytest.mark.parametrize("name,K,B", GRID + [("2-32-1", 16, 37)])
@pytest.mark.parametrize("weighted", [False, True])
def test_lp_and_gradients_match_torch_autograd(name, K, B, weighted):
    c = MR.case(name, K, B); w = c["w"] if weighted else None
    lp_t, loss_t, gs_t, gw_t = _torch_loss(c, w)
    loss, gs, gw, resp = MR.loss_and_grads(c, w=w)
    assert np.abs(MR.logpdf(c) - lp_t).max() <= 1e-10 and abs(loss - loss_t) <= 1e-10
    for g, gt in zip(gs + [gw], gs_t + [gw_t]):
        assert g.shape == gt.shape and np.abs(g - gt).max() <= 1e-10
    assert abs(resp.sum() - 1) < 1e-12 and resp.min() >= MR.MIN_RESPONSIBILITY


@pytest.mark.parametrize("name", list(MR.SHAPES))
def test_one_component_is_the_plain_gaussian(name):
    c = MR.case(name, 1, 37); nd = c["nd"]; p = c["ps"][0]
    mu = ER.forward(p[:-nd], c["dims"], c["acts"], c["s"])[0]; ls = np.asarray(p[-nd:], np.float64)[:, None]
    gauss = (-(c["a"] - mu) ** 2 / (2 * np.exp(2 * ls)) - 0.5 * np.log(2 * np.pi) - ls).sum(0)
    shift = np.log(np.float64(c["wp"][0])) if c["wdims"] is None else 0.0      # the constant weight is used raw: log alpha is added; a softmax over one row is 1
    assert np.abs(MR.logpdf(c) - (gauss + shift)).max() <= 1e-12


@pytest.mark.parametrize("name,K,B", GRID)
def test_naive_form_equals_the_stable_one_where_finite(name, K, B):
    c = MR.case(name, K, B); naive = MR.naive_logpdf(c); ok = np.isfinite(naive)
    assert ok.all() and np.abs(naive - MR.logpdf(c)).max() <= 1e-9
    n32 = MR.naive_logpdf(c, dtype=np.float32); ok = np.isfinite(n32)      # and in float32, where the reference evaluates it
    assert np.abs(n32[ok] - MR.logpdf(c)[ok]).max() <= 1e-3


def test_naive_form_underflows_where_the_stable_one_does_not():
    c = MR.case("2-32-1", 2, 37); far = MR.far_actions(c)
    l, _ = MR.component_logpdfs(c, c["s"], far)
    assert (l < -200).all()
    with np.errstate(divide="ignore"):
        assert np.isneginf(MR.naive_logpdf(c, a=far, dtype=np.float32)).all()      # every exp(l_k) is 0 in Float32
    lp = MR.logpdf(c, a=far); assert np.isfinite(lp).all() and (lp < -200).all()
    lp32 = MR.density(c, a=far, dtype=np.float32)[0]
    assert np.isfinite(lp32).all() and np.abs(lp32 - lp).max() <= 1e-5 * np.abs(lp).max()
    info, gs, new = MR.step(dict(c, a=far), MR.optimisers(c))
    assert np.isfinite(info["grad_norm"]) and all(np.isfinite(p).all() for p in new)


def test_float32_restatement_error_is_small():
    for name in MR.SHAPES:
        e = MR.float32_error(name); print("%s: float32 lp error %.3g -> tolerance %.3g" % (name, e, 4 * e))
        assert 0 < e < 1e-4


def test_adam_comparison_leaves_out_at_most_a_quarter():
    worst = (0.0, None)
    for name, K, B, weighted in MR.STEP_CASES:
        c = MR.case(name, K, B); _, gs, gw, _ = MR.loss_and_grads(c, w=c["w"] if weighted else None)
        for h, g in enumerate(gs + [gw]):
            sh = MR.skipped_share(g); worst = max(worst, (sh, (name, K, B, weighted, h)))
            assert sh <= 0.25, (name, K, B, weighted, h, sh)
    print("largest share left out: %.1f %% %s" % (100 * worst[0], worst[1]))


def test_fit_is_its_steps_and_max_batches_ends_it():
    c = MR.case("2-32-1", 3, 300); N = 300
    perms = [np.random.default_rng(40 + k).permutation(N) for k in range(2)]
    ps, rows = MR.fit(c, c["s"], c["a"], c["w"], 128, 2, perms)
    assert len(rows) == 2 and len(ps) == 4
    opts = MR.optimisers(c); cur = dict(c)
    for ep, idx in ER.minibatches(N, 128, 2, perms):
        _, _, new = MR.step(cur, opts, c["s"][:, idx], c["a"][:, idx], c["w"][:, idx]); cur = dict(cur, ps=new[:3], wp=new[3])
    assert all(np.array_equal(a, b) for a, b in zip(ps, cur["ps"] + [cur["wp"]]))
    ps3, rows3 = MR.fit(c, c["s"], c["a"], c["w"], 128, 2, perms, max_batches=3)
    assert len(rows3) == 1 and rows3[0]["loss"] == rows[0]["loss"]
    bad = dict(c, a=np.where(np.arange(N) == 5, np.nan, c["a"]))
    info, _, new = MR.step(bad, MR.optimisers(c))
    assert np.isnan(info["grad_norm"]) and all(np.array_equal(p, np.asarray(q, np.float64)) for p, q in zip(new, c["ps"] + [c["wp"]]))
