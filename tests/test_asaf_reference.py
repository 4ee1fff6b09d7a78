"""No GPU: known answers for the float64 yardstick of ASAF (tests/asaf_reference.py), so that what tests/test_gpu_asaf.py compares the device against is itself pinned.

With pi == piG every difference of log-densities is zero: both softplus terms are ln 2 and every sigmoid weight is 1/2, whatever the data."""
import numpy as np
import pytest
import torch

import asaf_reference as R

DIMS, ACTS = [3, 16, 16, 2], ["tanh", "tanh", "identity"]


def _case(seed, ascale, n=24, nE=19, logsigma=(-0.7, 0.3)):
    rng = np.random.default_rng(seed)
    p = []
    for i, o in zip(DIMS[:-1], DIMS[1:]):
        p += [rng.normal(0, 0.4, i * o), rng.normal(0, 0.1, o)]
    p = np.concatenate(p + [np.asarray(logsigma, np.float64)]).astype(np.float32)
    lim = 0.9 * ascale if ascale > 0 else 1.5
    d = {"s": rng.normal(0, 1, (3, n)).astype(np.float32), "a": rng.uniform(-lim, lim, (2, n)).astype(np.float32),
         "sE": rng.normal(0, 1, (3, nE)).astype(np.float32), "aE": rng.uniform(-lim, lim, (2, nE)).astype(np.float32)}
    return p, d


@pytest.mark.parametrize("ascale", [0.0, 2.0], ids=["gaussian", "squashed"])
def test_loss_is_two_ln2_minus_entropy_share_when_pi_is_its_frozen_copy(ascale):
    p, d = _case(1, ascale)
    gG, gE = R.frozen(p, DIMS, ACTS, d["s"], d["a"], ascale), R.frozen(p, DIMS, ACTS, d["sE"], d["aE"], ascale)
    layers, ls = R.params(p, DIMS)
    loss, parts = R.asaf_loss(layers, ACTS, ls, d["s"], d["a"], gG, d["sE"], d["aE"], gE, ascale)
    H = float(np.float32(1.4189385332046727)) + float(np.float64(p[-2]) + np.float64(p[-1]))
    assert abs(parts["entropy"] - H) < 1e-12
    assert abs(parts["expert"] - np.log(2.0)) < 1e-12 and abs(parts["policy"] - np.log(2.0)) < 1e-12
    assert abs(loss.item() - (2 * np.log(2.0) - 0.1 * H)) < 1e-12


@pytest.mark.parametrize("ascale", [0.0, 2.0], ids=["gaussian", "squashed"])
def test_gradient_is_half_the_difference_of_mean_score_functions_when_pi_is_its_frozen_copy(ascale):
    p, d = _case(2, ascale)
    gG, gE = R.frozen(p, DIMS, ACTS, d["s"], d["a"], ascale), R.frozen(p, DIMS, ACTS, d["sE"], d["aE"], ascale)
    layers, ls = R.params(p, DIMS)
    loss, _ = R.asaf_loss(layers, ACTS, ls, d["s"], d["a"], gG, d["sE"], d["aE"], gE, ascale)
    loss.backward(); g = R.flat(layers, ls)
    layers2, ls2 = R.params(p, DIMS)
    lin = 0.5 * (R.logpdf(layers2, ACTS, ls2, d["s"], d["a"], ascale).mean() - R.logpdf(layers2, ACTS, ls2, d["sE"], d["aE"], ascale).mean()) - 0.1 * R.entropy(ls2)
    lin.backward(); want = R.flat(layers2, ls2)
    assert np.abs(g).max() > 1e-3
    assert np.abs(g - want).max() < 1e-12 * max(1.0, np.abs(want).max())


def test_gaussian_logpdf_is_the_closed_form():
    mu, ls, a = torch.tensor([[0.5], [-1.0]], dtype=torch.float64), torch.tensor([0.2, -0.4], dtype=torch.float64), torch.tensor([[1.0], [0.0]], dtype=torch.float64)
    c = float(np.float32(0.9189385332046727))
    want = (-(0.5 ** 2) / (2 * np.exp(0.2) ** 2) - c - 0.2) + (-(1.0 ** 2) / (2 * np.exp(-0.4) ** 2) - c + 0.4)
    assert abs(R.gaussian_logpdf(mu, ls, a).item() - want) < 1e-12


def test_squashed_logpdf_at_a_stored_action_of_exactly_ascale_uses_the_clamp():
    ascale = 2.0
    hi = float(np.float32(1.0) - np.float32(1.0e-5))
    u = R.untanh(np.array([[ascale, -ascale, 2.5 * ascale]], np.float32), ascale).numpy()[0]
    assert np.isfinite(u).all() and u[0] == np.arctanh(hi) and u[1] == -np.arctanh(hi) and u[2] == u[0]
    assert abs(u[0] - np.arctanh(1 - 1e-5)) > 1e-4          # the float32 bound is not the float64 one: atanh is steep there
    p, d = _case(3, ascale, n=4)
    d["a"][:, 0] = ascale; d["a"][:, 1] = -ascale
    layers, ls = R.params(p, DIMS)
    lp = R.logpdf(layers, ACTS, ls, d["s"], d["a"], ascale)
    assert torch.isfinite(lp).all()
    mu = R.mlp(layers, ACTS, torch.as_tensor(d["s"].astype(np.float64)))[:, 0]
    uu = torch.full((2,), float(np.arctanh(hi)), dtype=torch.float64)
    c = float(np.float32(0.9189385332046727))
    want = (-((uu - mu) ** 2) / (2 * torch.exp(ls) ** 2) - c - ls - 2 * (float(np.log(np.float32(2.0))) - uu - torch.log1p(torch.exp(-2 * uu)))).sum()
    assert abs(lp[0].item() - want.item()) < 1e-10
    lp.sum().backward()
    assert all(torch.isfinite(W.grad).all() and torch.isfinite(b.grad).all() for W, b in layers)


@pytest.mark.parametrize("logsigma,inside", [((-0.7, 0.3), (True, True)), ((2.5, -0.2), (False, True)), ((-5.5, 3.0), (False, False))])
def test_squashed_logsigma_gradient_loses_its_first_term_outside_the_clamp(logsigma, inside):
    ascale = 2.0
    p, d = _case(4, ascale, logsigma=logsigma)
    layers, ls = R.params(p, DIMS)
    R.logpdf(layers, ACTS, ls, d["s"], d["a"], ascale).sum().backward()
    B = d["s"].shape[1]
    with torch.no_grad():
        mu = R.mlp(layers, ACTS, torch.as_tensor(d["s"].astype(np.float64))); u = R.untanh(d["a"], ascale)
        s2 = torch.exp(torch.clamp(ls, -5.0, 2.0))[:, None] ** 2
        first = (((u - mu) ** 2) / s2).sum(1).numpy()
    for k in range(2):
        want = (first[k] if inside[k] else 0.0) - B
        assert abs(ls.grad[k].item() - want) < 1e-9 * max(1.0, abs(want)), (k, ls.grad[k].item(), want)
    # the Gaussian head has no clamp: the first term is there whatever logSigma is
    layers, ls = R.params(p, DIMS)
    R.logpdf(layers, ACTS, ls, d["s"], d["a"], 0.0).sum().backward()
    with torch.no_grad():
        mu = R.mlp(layers, ACTS, torch.as_tensor(d["s"].astype(np.float64)))
        first = (((torch.as_tensor(d["a"].astype(np.float64)) - mu) ** 2) / (torch.exp(ls)[:, None] ** 2)).sum(1).numpy()
    assert np.abs(ls.grad.numpy() - (first - B)).max() < 1e-9 * max(1.0, np.abs(first).max())


def test_clip_value_and_adam_first_step():
    g = np.array([-3.0, 0.5, 2.0, 1e-9])
    assert np.array_equal(R.clip_value(g, 1.0), [-1.0, 0.5, 1.0, 1e-9]) and R.clip_value(g, None) is g and R.clip_value(g, np.inf) is g and R.clip_value(g, 0.0) is g
    p = R.adam_first_step(np.zeros(3), np.array([2.0, -0.1, 5.0]), lr=1e-3)
    assert np.abs(p - np.array([-1e-3, 1e-3, -1e-3])).max() < 1e-9
