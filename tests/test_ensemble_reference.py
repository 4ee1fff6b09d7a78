"""No GPU: pins the float64 yardstick of the ensemble tests (tests/ensemble_reference.py) -- against torch float64 autograd of training_loss on every test shape, hand
values, the ignored weights of the classification loss -- and derives what the GPU tests take from it: the tolerance of var* and of the ensemble logpdf (four times
the error of a float32 restatement in the reference's operand order, `ER.mixture_tolerance`) and the share of parameters an Adam-step comparison leaves out.
Run with -s to see the measured figures (they are quoted in tests/test_gpu_ensemble.py's docstring).
"""
import numpy as np
import pytest

import ensemble_reference as ER

GRID = [(n, M, B) for n in ER.SHAPES for M in ER.MS for B in ER.BS]


def _torch_loss_grads(c, weighted):
    import torch
    dims, acts, kind = c["dims"], c["acts"], c["kind"]
    x = torch.tensor(c["x"], dtype=torch.float64); y = torch.tensor(c["y"], dtype=torch.float64); w = torch.tensor(c["w"], dtype=torch.float64) if weighted else torch.ones_like(y)
    ps = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in c["ps"]]; losses = []
    for p in ps:
        h, off = x, 0
        for l, a in enumerate(acts):
            i, o = dims[l], dims[l + 1]
            W = p[off:off + i * o].reshape(i, o).T; off += i * o; b = p[off:off + o]; off += o      # column-major (out x in)
            h = W @ h + b[:, None]
            h = torch.relu(h) if a == "relu" else torch.tanh(h) if a == "tanh" else h
        if kind == ER.GAUSS:
            nd = dims[-1] // 2; mu, var = h[:nd], torch.nn.functional.softplus(h[nd:]) + 1e-3
            losses.append(-(w * (-torch.log(var) / 2 - (y - mu) ** 2 / (2 * var))).mean())
        else:
            pr = torch.softmax(h, 0); losses.append((-torch.xlogy(y, pr + ER.EPS32).sum(0)).mean())
    L = torch.stack(losses).mean(); L.backward()
    return float(L.detach()), [float(l.detach()) for l in losses], [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name,M,B", GRID)
def test_loss_and_gradients_match_torch_autograd(name, M, B, weighted):
    c = ER.case(name, M, B)
    loss, lm, gs = ER.loss_and_grads(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], c["w"] if weighted else None)
    tl, tlm, tg = _torch_loss_grads(c, weighted)
    assert abs(loss - tl) <= 1e-12 * max(1.0, abs(tl)) and np.allclose(lm, tlm, rtol=1e-12, atol=0)
    for g, t in zip(gs, tg):
        assert np.abs(g - t).max() <= 1e-9 * np.abs(t).max(), (name, M, B, np.abs(g - t).max(), np.abs(t).max())


def test_hand_values():
    # M = 1, nd = 1, o = (0, 0), y = 0: var = log 2 + 1e-3 and loss = log(var) / 2
    o = np.zeros((2, 1)); y = np.zeros((1, 1)); var = np.log(2.0) + 1e-3
    mu_, var_ = ER.members(ER.GAUSS, [o])
    assert mu_[0][0, 0] == 0 and abs(var_[0][0, 0] - var) < 1e-15
    assert abs(ER.training_loss(ER.GAUSS, [o], y) - np.log(var) / 2) < 1e-15
    # two members with mu = +-1 and equal var = s: mu* = 0 and var* = s + 1
    z = 0.3; s = ER.softplus(np.array(z)) + 1e-3
    mean, evar = ER.mixture(ER.GAUSS, [np.array([[1.0], [z]]), np.array([[-1.0], [z]])])
    assert mean[0, 0] == 0 and abs(evar[0, 0] - (s + 1)) < 1e-15
    # uniform logits over C classes: loss = -log(1 / C + eps)
    for C in (2, 3, 7):
        y = np.zeros((C, 4)); y[np.arange(4) % C, np.arange(4)] = 1
        assert abs(ER.training_loss(ER.CLASS, [np.full((C, 4), 0.7)], y) + np.log(1.0 / C + ER.EPS32)) < 1e-15
        assert abs(ER.logpdf(ER.CLASS, [np.full((C, 4), 0.7)] * 2, y)[0, 0] - np.log(1.0 / C + 1e-10)) < 1e-15


def test_seeds_carry_every_factor():
    """a 1 / M, a 1 / (nd B), a swapped half or a missing logistic factor in the seeds changes the gradient by far more than the GPU test's 1e-4"""
    c = ER.case("5-100-100-4", 3, 37); os = [ER.forward(p, c["dims"], c["acts"], c["x"])[0] for p in c["ps"]]
    sd = ER.seeds(ER.GAUSS, os, c["y"], c["w"])[0]; nd = 2; sc = np.abs(sd).max()
    wrong = [sd * 3, sd * (nd * 37), np.concatenate([sd[nd:], sd[:nd]], 0), np.concatenate([sd[:nd], sd[nd:] / ER.logistic(os[0][nd:])], 0)]
    assert all(np.abs(wg - sd).max() > 1e-2 * sc for wg in wrong)


def test_classification_loss_ignores_the_weights():
    c = ER.case("4-100-100-3", 3, 37)
    a = ER.loss_and_grads(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], None)
    b = ER.loss_and_grads(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], 5.0 * c["w"])
    assert a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    g = ER.case("3-12-2", 3, 37)      # the regression loss does not
    assert ER.training_loss(ER.GAUSS, [ER.forward(p, g["dims"], g["acts"], g["x"])[0] for p in g["ps"]], g["y"], g["w"]) != \
        ER.training_loss(ER.GAUSS, [ER.forward(p, g["dims"], g["acts"], g["x"])[0] for p in g["ps"]], g["y"], None)


def test_adam_step_and_nan_gate():
    c = ER.case("3-12-2", 3, 37); opts = [ER.Adam64(len(p)) for p in c["ps"]]
    info, gs, new = ER.step(c["ps"], opts, c["dims"], c["acts"], c["kind"], c["x"], c["y"], c["w"])
    for p, g, q in zip(c["ps"], gs, new):      # the first Adam step moves every parameter by lr sign(g) (up to eps)
        nz = np.abs(g) > 1e-6
        assert np.allclose((q - p)[nz], -1e-3 * np.sign(g[nz]), rtol=1e-3, atol=0)
    assert abs(info["loss"] - np.mean(info["losses"])) < 1e-15 and abs(info["grad_norm"] ** 2 - sum(n * n for n in info["norms"])) < 1e-12
    y = c["y"].copy(); y[0, 5] = np.nan
    info, _, same = ER.step(c["ps"], [ER.Adam64(len(p)) for p in c["ps"]], c["dims"], c["acts"], c["kind"], c["x"], y, None)
    assert np.isnan(info["grad_norm"]) and all(np.array_equal(a, b) for a, b in zip(same, c["ps"]))


def test_fit_walks_the_injected_permutations():
    rng = np.random.default_rng(3); N = 300
    perms = [rng.permutation(N) for _ in range(2)]
    mb = ER.minibatches(N, 128, 2, perms)
    assert [len(i) for _, i in mb] == [128, 128, 44] * 2 and [e for e, _ in mb] == [0, 0, 0, 1, 1, 1]
    assert np.array_equal(np.concatenate([i for e, i in mb if e == 1]), perms[1])
    assert len(ER.minibatches(N, 128, 2, perms, max_batches=3)) == 3 and len(ER.minibatches(N, 128, 2, perms, max_batches=4)) == 4
    c = ER.case("3-12-2", 3, N)
    ps, rows = ER.fit(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], c["w"], 128, 2, perms)
    opts = [ER.Adam64(len(p)) for p in c["ps"]]; qs = c["ps"]
    for _, idx in mb:
        info, _, qs = ER.step(qs, opts, c["dims"], c["acts"], c["kind"], c["x"][:, idx], c["y"][:, idx], c["w"][:, idx])
    assert all(np.array_equal(a, b) for a, b in zip(ps, qs)) and len(rows) == 2 and rows[1]["loss"] == info["loss"]


@pytest.mark.parametrize("name", list(ER.SHAPES))
def test_float32_tolerance_of_the_mixture(name):
    """what the GPU test allows in var* and in the ensemble logpdf: four times float32's own error, and the inputs keep it meaningful (|mu*| of order one, var* >= 0.05)"""
    ev, el = ER.float32_error(name); tv, tl = ER.mixture_tolerance(name)
    print("%s: float32 error var* %.3g logpdf %.3g -> tolerance %.3g / %.3g" % (name, ev, el, tv, tl))
    assert tl == 4 * el and tv == 4 * ev and 0 < el < 1e-4 and ev < 1e-4
    for M in ER.MS:
        for B in ER.BS:
            mean, evar, _ = ER.mixture64(ER.case(name, M, B))
            assert np.abs(mean).max() < 10
            if evar is not None:
                assert ev > 0 and evar.min() >= 0.05, (name, M, B, evar.min())


def test_adam_comparison_leaves_out_at_most_a_quarter():
    """the share of parameters whose gradient is within 1e-3 of the gradient scale of zero, per member of every step case of the GPU test"""
    import test_gpu_ensemble as TG
    worst = (-1.0, ())
    for name, M, B, weighted in TG.STEP_CASES:
        c = ER.case(name, M, B)
        _, _, gs = ER.loss_and_grads(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], c["w"] if weighted else None)
        sh = max(ER.skipped_share(g) for g in gs); worst = max(worst, (sh, (name, M, B, weighted)))
        assert sh <= TG.STEP_SKIPPED_MAX, (name, M, B, weighted, sh)
    print("largest share left out: %.1f %% %s" % (100 * worst[0], worst[1]))
