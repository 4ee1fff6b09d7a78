"""The yardstick of the two-headed Gaussian actors (tests/sigma_head_reference.py) against torch float64 autograd of the reference's formulas, written with TWO head layers over
one shared trunk object (policies.jl:333-398, sac.jl:34-52): the hand gradient of sac_actor_loss, exploration / logpdf consistency (policy_tests.jl:305-316), the clamp, the
entropy shapes, and the share of parameters the GPU test leaves out of its Adam comparison. No GPU."""
import numpy as np
import pytest
import torch

import ensemble_reference as ER
import sigma_head_reference as SR

GRAD_CASES = [(n, 37, sc, None) for n in SR.SHAPES for sc in SR.ASCALES] + [(n, 37, sc, k) for n in ("2-32-2x1", "5-100-100-2x3") for sc in (1.0, 2.0) for k in (0, 1, 2)]


def _t(x):
    return torch.tensor(np.asarray(x, np.float64))


def _act(a, h):
    return torch.relu(h) if a == "relu" else torch.tanh(h) if a == "tanh" else h


def _chain(layers, acts, x):
    for (W, b), a in zip(layers, acts):
        x = _act(a, W @ x + b[:, None])
    return x


def _leaf_layers(flat, dims):
    Ws, bs = ER.unflatten(flat, dims)
    return [(_t(W).requires_grad_(True), _t(b).requires_grad_(True)) for W, b in zip(Ws, bs)]


def torch_actor_loss(c, eps):
    """sac_actor_loss with mu = Chain(base..., head_mu), logSigma = Chain(base..., head_ls) over the SAME base tensors: (loss, entropy, flat gradient in the one-chain layout)"""
    ad, sc = c["ad"], c["ascale"]; layers = _leaf_layers(c["p"], c["dims"]); base = layers[:-1]; W, b = layers[-1]
    Wm, bm, Wl, bl = (W[:ad].detach().clone().requires_grad_(True), b[:ad].detach().clone().requires_grad_(True),
                      W[ad:].detach().clone().requires_grad_(True), b[ad:].detach().clone().requires_grad_(True))
    s = _t(c["s"]); acts = c["acts"]
    mu = _chain(base + [(Wm, bm)], acts, s); l = _chain(base + [(Wl, bl)], acts, s)      # two networks, one trunk object: autograd adds the two paths
    e = _t(eps)
    sg = torch.exp(torch.clamp(l, -5, 2)) if sc > 0 else torch.exp(l)
    u = e * sg + mu
    lp = -((u - mu) ** 2) / (2 * sg ** 2) - SR.C0 - l
    if sc > 0:
        lp = lp - 2 * (np.log(2.0) - u - torch.nn.functional.softplus(-2 * u)); a = sc * torch.tanh(u)
    else:
        a = u
    lp = lp.sum(0)
    x = torch.cat([s, a], 0)
    q = [_chain([(_t(W_), _t(b_)) for W_, b_ in zip(*ER.unflatten(c[k], c["qdims"]))], c["qacts"], x)[0] for k in ("q1", "q2")]
    loss = (np.exp(np.float64(c["log_alpha"])) * lp - torch.minimum(q[0], q[1])).mean()
    loss.backward()
    g = [np.concatenate([W_.grad.numpy().reshape(-1, order="F"), b_.grad.numpy()]) for W_, b_ in base]
    g.append(np.concatenate([np.vstack([Wm.grad.numpy(), Wl.grad.numpy()]).reshape(-1, order="F"), bm.grad.numpy(), bl.grad.numpy()]))
    return float(loss.detach()), float(-lp.detach().mean()), np.concatenate(g)


@pytest.mark.parametrize("name,B,sc,clamp", GRAD_CASES)
def test_hand_gradient_matches_autograd(name, B, sc, clamp):
    c = SR.case(name, B, sc, clamp)
    loss, ent, g, _ = SR.sac_actor_loss(c)
    tl, te, tg = torch_actor_loss(c, c["eps"][2])
    assert abs(loss - tl) <= 1e-10 * max(1.0, abs(tl)) and abs(ent - te) <= 1e-10 * max(1.0, abs(te))
    assert np.abs(g - tg).max() <= 1e-9 * np.abs(tg).max(), (np.abs(g - tg).max(), np.abs(tg).max())
    # the trunk's gradient is the SUM of both heads' paths: it differs from what the mu path alone would give
    if len(c["dims"]) > 2:
        _, _, _, dz = SR.sac_actor_loss(c); hs = SR.forward(c, c["s"])[2]; dz_mu = dz.copy(); dz_mu[c["ad"]:] = 0.0
        g_mu = ER.backward(c["p"], c["dims"], c["acts"], hs, dz_mu); n0 = c["dims"][0] * c["dims"][1]
        assert np.abs(g[:n0] - g_mu[:n0]).max() > 1e-6 * np.abs(g[:n0]).max()


@pytest.mark.parametrize("name", list(SR.SHAPES))
@pytest.mark.parametrize("sc", SR.ASCALES)
def test_exploration_logpdf_consistency(name, sc):
    """logpdf(pi, s, exploration(pi, s)[1]) == the exploration's own logprob (policy_tests.jl:305-316); squashed: where the stored action is inside the atanh clamp"""
    c = SR.case(name, 257, sc)
    a, lp, u = SR.explore(c, c["s"], c["eps"][2])
    assert a.shape == (c["ad"], 257) and lp.shape == (257,)
    if sc > 0:
        assert np.abs(a).max() <= sc
        ok = (np.abs(a / sc) < 1.0 - 2e-5).all(0); assert ok.mean() > 0.9
    else:
        ok = np.ones(257, bool)
    assert np.abs(SR.logpdf(c, c["s"], a)[ok] - lp[ok]).max() <= 1e-6 * max(1.0, np.abs(lp[ok]).max())
    # the stored actions of the case come from the policy itself
    assert np.isfinite(SR.logpdf(c, c["s"], c["a"])).all()


@pytest.mark.parametrize("name", ["2-32-2x1", "5-100-100-2x3"])
@pytest.mark.parametrize("sc", [1.0, 2.0])
def test_clamp_cases(name, sc):
    """the logSigma head's biases at -6 / 0 / 3 put l below -5, inside and above 2; none within 1e-3 of an edge; sigma is the clamped one, and a clamped l's gradient is -c"""
    seen = set()
    for k in (0, 1, 2):
        c = SR.case(name, 37, sc, clamp=k); mu, l, _ = SR.forward(c, c["s"]); B = c["B"]
        assert np.abs(l + 5).min() > 1e-3 and np.abs(l - 2).min() > 1e-3
        seen |= {"lo"} if (l < -5).any() else set(); seen |= {"in"} if ((l > -5) & (l < 2)).any() else set(); seen |= {"hi"} if (l > 2).any() else set()
        _, _, u = SR.explore(c, c["s"], c["eps"][2])
        np.testing.assert_allclose(u - mu, c["eps"][2] * np.exp(np.clip(l, -5, 2)), rtol=1e-12, atol=1e-12)
        dz = SR.sac_actor_loss(c)[3]; out = (l < -5) | (l > 2)
        assert np.allclose(dz[c["ad"]:][out], -np.exp(np.float64(c["log_alpha"])) / B, rtol=1e-12)      # (ad = 1: the k = 1 case has only the inside row)
        # the Gaussian head does not clamp
        g = SR.case(name, 37, 0.0, clamp=k); mug, lg, _ = SR.forward(g, g["s"]); _, _, ug = SR.explore(g, g["s"], g["eps"][2])
        np.testing.assert_allclose(ug - mug, g["eps"][2] * np.exp(lg), rtol=1e-12, atol=1e-12)
    assert seen == {"lo", "in", "hi"}


def test_entropy_shapes():
    c = SR.case("5-100-100-2x3", 37, 2.0); g = SR.case("5-100-100-2x3", 37, 0.0)
    e = SR.entropy(c, c["s"]); assert e.shape == (1, 37)
    np.testing.assert_allclose(e[0], SR.ENT0 + SR.forward(c, c["s"])[1].sum(0))
    eg = SR.entropy(g, g["s"]); assert np.ndim(eg) == 0      # policies.jl:348: `sum` over everything
    np.testing.assert_allclose(eg, SR.ENT0 + SR.forward(g, g["s"])[1].sum())
    assert SR.action(c, c["s"]).shape == (3, 37) and np.abs(SR.action(c, c["s"])).max() <= 2.0


def test_temperature_and_target():
    c = SR.case("4-256-256-2x2", 37, 1.0)
    v, g = SR.sac_temp_loss(c); la = torch.tensor(float(c["log_alpha"]), dtype=torch.float64, requires_grad=True)
    lp = _t(SR.explore(c, c["s"], c["eps"][1])[1]); L = -(torch.exp(la) * (lp + float(c["H"]))).mean(); L.backward()
    assert abs(v - float(L.detach())) <= 1e-12 * abs(v) and abs(g - float(la.grad)) <= 1e-12 * abs(g)
    y = SR.sac_target(c); assert y.shape == (37,) and np.isfinite(y).all()
    d = c["done"]; np.testing.assert_allclose(y[d], c["r"][d].astype(np.float64))      # (1 - done) removes the bootstrap term


def test_skipped_share_of_step_cases():
    """Parameters whose float64 gradient lies within 1e-3 of the gradient scale of zero are left out of the GPU test's Adam comparison: at most a quarter per handle, on every
    step case, with the yardstick alone, from the very normals of the GPU comparison (the device's Philox draws, restated on the host). The largest share is printed (and
    recorded in tests/test_gpu_sigma_head.py's docstring)."""
    worst = 0.0; assert all((n, 1, 2.0) in SR.STEP_CASES for n in SR.GRID_SHAPES)      # the lone column of every grid shape takes the Adam comparison too
    for name, B, sc in SR.STEP_CASES:
        _, g, p = SR.actor_step(SR.case(name, B, sc), SR.philox_normals(SR.ACTOR_CTR, B, SR.SHAPES[name][2])); sh = SR.skipped_share(g); worst = max(worst, sh)
        print("skipped share %-16s B=%-5d ascale=%g: %.4f" % (name, B, sc, sh))
        assert sh <= 0.25, (name, B, sc, sh)
        keep = np.abs(g) > 1e-3 * np.abs(g).max(); c = SR.case(name, B, sc)
        np.testing.assert_allclose((np.asarray(c["p"], np.float64) - p)[keep], 1e-3 * np.sign(g[keep]), rtol=1e-3)      # Adam's first step: lr sign(g)
    print("largest skipped share: %.4f" % worst)


@pytest.mark.parametrize("name", SR.GRID_SHAPES)
def test_float32_error_and_tolerance(name):
    elp, ey = SR.float32_error(name); tlp, ty = SR.tolerance(name)
    print("float32 error %-16s lp %.3e  y %.3e  -> tolerances %.3e %.3e" % (name, elp, ey, tlp, ty))
    assert 0 < elp < 1e-2 and 0 < ey < 1e-2 and tlp == 4 * elp and ty == 4 * ey
