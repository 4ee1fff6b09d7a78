"""The float64 yardstick of the spectrally normalised layers (tests/sn_reference.py) against independent evidence: torch autograd for the analytic gradient,
numpy's SVD for the power iteration, and the fixed-point property that makes the one-call and two-call BCE discriminator steps agree."""
import numpy as np
import pytest
import torch

import sn_reference as SR


def _chain(rng, dims, scale=0.6):
    return SR.flatten([rng.standard_normal((dims[l + 1], dims[l])) * scale for l in range(len(dims) - 1)], [rng.standard_normal(dims[l + 1]) * 0.1 for l in range(len(dims) - 1)])


def _us(rng, dims, sn):
    return [rng.standard_normal(dims[l + 1]) for l in range(len(sn)) if sn[l]]


@pytest.mark.parametrize("dims,acts,sn", [
    ((3, 12, 1), ("relu", "identity"), (1, 1)),
    ((4, 10, 10, 2), ("tanh", "tanh", "identity"), (1, 3, 1)),
    ((3, 8, 8, 2, 1), ("relu", "tanh", "relu", "identity"), (1, 2, 1, 0)),
    ((5, 7, 3), ("tanh", "relu"), (0, 2)),
])
def test_analytic_gradient_matches_autograd(dims, acts, sn):
    rng = np.random.default_rng(11); B = 9
    flat, us, x = _chain(rng, dims), _us(rng, dims, sn), rng.standard_normal((dims[0], B))
    R = rng.standard_normal((dims[-1], B))
    y, c = SR.forward(flat, dims, acts, sn, us, x)
    g, dx = SR.backward(c, R)
    # autograd of act((W / (u'W v)) x + b) with u and v detached (the constants the forward call produced)
    Ws, bs = SR.unflatten(flat, dims)
    tW = [torch.tensor(W.copy(), dtype=torch.float64, requires_grad=True) for W in Ws]; tb = [torch.tensor(b.copy(), dtype=torch.float64, requires_grad=True) for b in bs]
    h = torch.tensor(x, dtype=torch.float64, requires_grad=True); h0 = h; k = 0
    for l in range(len(Ws)):
        W = tW[l]
        if sn[l]:
            u, v = torch.tensor(c["us"][k]), torch.tensor(c["vs"][k]); k += 1
            W = W / (u @ W @ v)
        z = W @ h + tb[l][:, None]
        h = torch.relu(z) if acts[l] == "relu" else torch.tanh(z) if acts[l] == "tanh" else z
    np.testing.assert_allclose(h.detach().numpy(), y, rtol=1e-12, atol=1e-14)
    (h * torch.tensor(R)).sum().backward()
    ref = SR.flatten([w.grad.numpy() for w in tW], [b.grad.numpy() for b in tb])
    scale = np.abs(ref).max()
    assert np.abs(g - ref).max() <= 1e-9 * scale
    assert np.abs(dx - h0.grad.numpy()).max() <= 1e-9 * np.abs(h0.grad.numpy()).max()


def test_power_iteration_converges_to_top_singular_value():
    """200 iterations on a random 12 x 3 matrix against numpy's SVD to 1e-8 relative. The iteration's own eps terms leave |u| = |s| / (|s| + eps) and
    |v| = |t| / (|t| + eps) just under 1, so u'W v sits 2 eps = 2.4e-7 (absolute) under the singular value whatever the iteration count: the bound of 1e-8
    relative is reachable only for sigma > 2 eps / 1e-8 = 24, hence entries of standard deviation 32 (sigma ~ 110). At unit scale (sigma = 3.5, where the
    eps terms alone are 6.8e-8 relative) the same bound is asked of the estimate with the two known norms divided out."""
    rng = np.random.default_rng(5); W1 = rng.standard_normal((12, 3)); u0 = rng.standard_normal(12)
    W = 32.0 * W1
    u, v = SR.power_iteration(W, u0, 200)
    top = np.linalg.svd(W, compute_uv=False)[0]
    assert abs(SR.msv(W, u, v) - top) <= 1e-8 * top
    u, v = SR.power_iteration(W1, u0, 200)
    top = np.linalg.svd(W1, compute_uv=False)[0]
    assert abs(SR.msv(W1, u, v) / (np.linalg.norm(u) * np.linalg.norm(v)) - top) <= 1e-8 * top
    assert abs(SR.msv(W1, u, v) - (top - 2 * SR.EPS)) <= 1e-8 * top


def test_one_call_and_two_call_bce_agree_at_the_fixed_point():
    rng = np.random.default_rng(7); dims, acts, sn = (3, 12, 1), ("relu", "identity"), (1, 1)
    flat = _chain(rng, dims); Ws, _ = SR.unflatten(flat, dims)
    us = [SR.power_iteration(Ws[l], rng.standard_normal(dims[l + 1]), 200)[0] for l in range(2)]
    x_ex, x_pi = rng.standard_normal((3, 16)), rng.standard_normal((3, 16))
    l1, g1, _, _ = SR.bce_step(flat, dims, acts, sn, us, x_ex, x_pi, two_call=False)
    l2, g2, _, _ = SR.bce_step(flat, dims, acts, sn, us, x_ex, x_pi, two_call=True)
    assert abs(l1 - l2) <= 1e-6 * abs(l1)
    assert np.abs(g1 - g2).max() <= 1e-6 * np.abs(g1).max()
    # away from the fixed point the two forms differ: the property is not vacuous
    far = [rng.standard_normal(12), rng.standard_normal(1)]
    la, ga, _, _ = SR.bce_step(flat, dims, acts, sn, far, x_ex, x_pi, two_call=False)
    lb, gb, _, _ = SR.bce_step(flat, dims, acts, sn, far, x_ex, x_pi, two_call=True)
    assert np.abs(ga - gb).max() > 1e-6 * np.abs(ga).max()


def test_single_output_layer():
    rng = np.random.default_rng(9); W = rng.standard_normal((1, 12))
    for u0 in (np.array([0.3]), np.array([-2.0])):
        u, v = SR.power_iteration(W, u0, 1)
        nrm = np.sqrt((W * W).sum())
        assert abs(abs(u[0]) - 1.0) <= 4 * SR.EPS / nrm + 1e-12 and np.sign(u[0]) == np.sign(u0[0])
        assert abs(SR.msv(W, u, v) - nrm) <= 4 * SR.EPS * (1.0 + nrm)
