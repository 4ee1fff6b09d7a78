"""Known-answer checks of tests/advil_reference.py, the float64 yardstick of the AdVIL tests (no GPU)."""
import numpy as np
import torch

import advil_reference as A
import iq_reference as R


def _layer(W):
    W = torch.tensor(np.asarray(W, np.float64), requires_grad=True)
    return [(W, torch.zeros(W.shape[0], dtype=torch.float64, requires_grad=True))]


def test_orth_reg_of_orthonormal_columns_is_zero():
    q, _ = np.linalg.qr(np.random.default_rng(0).normal(size=(64, 17)))
    assert abs(A.orth_reg(_layer(q), 1.0).item()) < 1e-24


def test_orth_reg_of_ones():
    """W = ones(2, 2): W'W = [[2, 2], [2, 2]], the two off-diagonal entries squared give 8"""
    assert np.isclose(A.orth_reg(_layer(np.ones((2, 2))), 0.25).item(), 0.25 * 8, rtol=1e-14)      # (norm(.)^2 goes through a square root)


def test_orth_reg_sums_over_layers_and_ignores_biases():
    rng = np.random.default_rng(1)
    W1, W2 = rng.normal(size=(5, 3)), rng.normal(size=(2, 5))
    l1, l2 = _layer(W1), _layer(W2)
    both = [(l1[0][0], torch.full((5,), 7.0, dtype=torch.float64)), (l2[0][0], torch.full((2,), -3.0, dtype=torch.float64))]
    assert np.isclose(A.orth_reg(both, 2.0).item(), A.orth_reg(l1, 2.0).item() + A.orth_reg(l2, 2.0).item(), rtol=1e-14)


def test_orth_reg_gradient_is_4_beta_W_R():
    rng = np.random.default_rng(2)
    for shape, beta in (((64, 17), 1e-4), ((6, 64), 1.0)):
        W = rng.normal(0, 0.3, shape)
        lay = _layer(W)
        A.orth_reg(lay, beta).backward()
        Rm = W.T @ W; np.fill_diagonal(Rm, 0.0)
        want = 4 * beta * W @ Rm
        assert np.abs(lay[0][0].grad.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert lay[0][1].grad is None or not lay[0][1].grad.any()


def test_advil_d_loss_closed_form_for_a_linear_discriminator():
    """D(x) = w'x + c: mean D(expert) - mean D(pi) = w_a' (mean a - mean pi(s)); the input gradient is w everywhere, so the penalty is (|w| - 0.4)^2"""
    rng = np.random.default_rng(3); od, ad, B = 4, 2, 37
    s, a = rng.normal(size=(od, B)).astype(np.float32), rng.normal(size=(ad, B)).astype(np.float32)
    a_dims, a_acts = [od, 8, ad], ["tanh", "identity"]
    pa = rng.normal(0, 0.5, od * 8 + 8 + 8 * ad + ad)
    pd = rng.normal(0, 0.5, od + ad + 1)
    al, dl = A.mlp_params(pa, a_dims), A.mlp_params(pd, [od + ad, 1])
    loss, info = A.advil_d_loss(al, a_acts, dl, ["identity"], s, a, lambda_gp=10.0, seed=5, counter=13)
    w = pd[:od + ad]
    pi = A.mlp(al, a_acts, torch.as_tensor(s.astype(np.float64))).detach().numpy()
    want = w[od:] @ (a.astype(np.float64).mean(1) - pi.mean(1)) + 10.0 * (np.linalg.norm(w) - 0.4) ** 2
    assert np.isclose(loss.item(), want, rtol=1e-12, atol=1e-12)
    assert np.isclose(info["grad_pen"], (np.linalg.norm(w) - 0.4) ** 2, rtol=1e-12)
    assert np.isclose(info["D_expert"] - info["D_policy"] + info["gp_loss"], loss.item(), rtol=1e-13)


def test_advil_penalty_is_the_iq_penalty_at_target_04():
    rng = np.random.default_rng(4); od, ad, B, seed, ctr = 3, 2, 20, 9, 21
    s, a = rng.normal(size=(od, B)).astype(np.float32), rng.normal(size=(ad, B)).astype(np.float32)
    a_dims, a_acts, d_dims, d_acts = [od, 6, ad], ["relu", "identity"], [od + ad, 7, 1], ["tanh", "identity"]
    pa, pd = rng.normal(0, 0.5, od * 6 + 6 + 6 * ad + ad), rng.normal(0, 0.5, (od + ad) * 7 + 7 + 7 + 1)
    al, dl = A.mlp_params(pa, a_dims), A.mlp_params(pd, d_dims)
    _, info = A.advil_d_loss(al, a_acts, dl, d_acts, s, a, seed=seed, counter=ctr)
    xh = R.xhat(np.concatenate([s, a], 0), A.policy_sa(al, a_acts, s), R.eps(seed, ctr, B))
    assert np.isclose(info["grad_pen"], R.gradient_penalty(dl, d_acts, xh, target=0.4).item(), rtol=1e-14)
    assert not np.isclose(info["grad_pen"], R.gradient_penalty(dl, d_acts, xh, target=1.0).item(), rtol=1e-3)


def test_advil_pi_loss_pieces():
    """with D(x) = the sum of the action entries the loss is mean(sum pi(s)) + lambda mse, and only the actor receives a gradient that matters"""
    rng = np.random.default_rng(5); od, ad, B = 3, 2, 11
    s, a = rng.normal(size=(od, B)).astype(np.float32), rng.normal(size=(ad, B)).astype(np.float32)
    a_dims, a_acts = [od, ad], ["identity"]
    pa = rng.normal(0, 0.5, od * ad + ad)
    pd = np.concatenate([np.zeros(od), np.ones(ad), [0.0]])
    al, dl = A.mlp_params(pa, a_dims), A.mlp_params(pd, [od + ad, 1])
    loss, info = A.advil_pi_loss(al, a_acts, dl, ["identity"], s, a, lambda_bc=0.2)
    W, b = pa[:od * ad].reshape((ad, od), order="F"), pa[od * ad:]
    pi = W @ s.astype(np.float64) + b[:, None]
    assert np.isclose(loss.item(), pi.sum(0).mean() + 0.2 * ((pi - a) ** 2).mean(), rtol=1e-12)
    assert np.isclose(info["bc_mse"], ((pi - a) ** 2).mean(), rtol=1e-12)


def test_loop_runs_and_lowers_the_bc_error():
    rng = np.random.default_rng(6); od, ad, n = 2, 1, 96
    s = rng.normal(size=(od, n)).astype(np.float32); a = np.tanh(s[:1] - 0.5 * s[1:]).astype(np.float32)
    a_dims, a_acts, d_dims, d_acts = [od, 16, ad], ["tanh", "identity"], [od + ad, 16, 1], ["tanh", "identity"]
    pa, pd = rng.normal(0, 0.3, od * 16 + 16 + 16 * ad + ad), rng.normal(0, 0.3, (od + ad) * 16 + 16 + 16 + 1)
    before = A.bc_mse(pa, a_dims, a_acts, s, a)
    pa2, pd2, hist = A.advil_loop(pa, pd, a_dims, a_acts, d_dims, d_acts, s, a, epochs=3, batch_size=40, lr=3e-3)
    assert len(hist) == 4 and all(np.isfinite(v) for h in hist for v in h.values())
    assert not np.array_equal(pd2, pd) and A.bc_mse(pa2, a_dims, a_acts, s, a) < before
