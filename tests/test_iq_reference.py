"""CPU checks of the float64 IQ-Learn yardstick (tests/iq_reference.py): the reference's own gradient_penalty test, the closed-form seeds and the two-sweep
parameter gradient of the penalty (csrc/iq.hip) against autograd, central finite differences on the whole loss, and the eps draws against the oracle's Philox."""
import numpy as np
import pytest
import torch

import cql_reference as CR
import iq_reference as R


def _net(dims, seed=0, scale=0.5):
    rng = np.random.default_rng(seed)
    n = sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1))
    return rng.normal(0, scale, n)


def _split(flat, dims):
    Ws, bs, off = [], [], 0
    for l in range(len(dims) - 1):
        i, o = dims[l], dims[l + 1]
        Ws.append(np.asarray(flat[off:off + i * o]).reshape((o, i), order="F")); off += i * o
        bs.append(np.asarray(flat[off:off + o])); off += o
    return Ws, bs


def test_reference_penalty_of_a_dense_layer_of_ones():
    # test/extras_tests.jl:9: gradient_penalty(Dense(2, 1, init=ones, bias=false), ones(2, 100)) ≈ (sqrt(2) - 1)^2
    layers = [(torch.ones((1, 2), dtype=torch.float64, requires_grad=True), torch.zeros(1, dtype=torch.float64, requires_grad=True))]
    P = R.gradient_penalty(layers, ["identity"], np.ones((2, 100)))
    assert abs(float(P) - (np.sqrt(2) - 1) ** 2) < 1e-12
    P2, _, _ = R.np_penalty_grad([np.ones((1, 2))], [np.zeros(1)], ["identity"], np.ones((2, 100)))
    assert abs(P2 - (np.sqrt(2) - 1) ** 2) < 1e-12


@pytest.mark.parametrize("act", ["identity", "relu", "tanh"])
def test_two_sweep_penalty_gradient_matches_autograd(act):
    dims = [3, 7, 5, 2]; acts = [act, act, "identity" if act != "tanh" else "tanh"]
    flat = _net(dims, seed=1); x = np.random.default_rng(2).normal(0, 1, (3, 9))
    layers = R.mlp_params(flat, dims)
    P = 4.0 * R.gradient_penalty(layers, acts, x, target=1.0)
    P.backward()
    g_ref = R.flat_grad(layers)
    Ws, bs = _split(flat, dims)
    P2, dW, db = R.np_penalty_grad(Ws, bs, acts, x, target=1.0, lam=4.0)
    g = np.concatenate([np.concatenate([W.reshape(-1, order="F"), b]) for W, b in zip(dW, db)])
    assert abs(4.0 * P2 - float(P)) < 1e-12
    assert np.allclose(g, g_ref, rtol=1e-10, atol=1e-12), np.abs(g - g_ref).max()


@pytest.mark.parametrize("reg", [False, True])
def test_closed_form_seeds_match_autograd(reg):
    rng = np.random.default_rng(4); A, B, Bp = 3, 10, 5
    Q, Qp = rng.normal(0, 1, (A, B)), rng.normal(0, 1, (A, B))
    a = np.eye(A)[rng.integers(0, A, B)].T; done = rng.random(B) < 0.3
    Qt, Qpt = torch.tensor(Q, requires_grad=True), torch.tensor(Qp, requires_grad=True)
    gd = 0.9 * (1 - torch.tensor(done, dtype=torch.float64))
    y = gd * torch.logsumexp(Qpt, 0); Rv = (Qt * torch.tensor(a)).sum(0) - y
    L = (-Rv[Bp:]).mean() + (torch.logsumexp(Qt, 0) - y).mean() + ((Rv ** 2).mean() / (4 * 0.5) if reg else 0)
    L.backward()
    s, sp = R.np_iq_seeds(Q, Qp, a, done, Bp, reg=reg)
    assert np.allclose(s, Qt.grad.numpy(), atol=1e-12) and np.allclose(sp, Qpt.grad.numpy(), atol=1e-12)


def test_iq_loss_matches_finite_differences():
    rng = np.random.default_rng(7); dims = [4, 6, 6, 3]; acts = ["tanh", "relu", "identity"]; B, Bp = 8, 4
    flat = _net(dims, seed=3)
    s, sp = rng.normal(0, 1, (4, B)), rng.normal(0, 1, (4, B))
    a = np.eye(3)[rng.integers(0, 3, B)].T; done = rng.random(B) < 0.25
    xh = R.xhat(s[:, Bp:], s[:, :Bp], R.eps(5, 9, Bp)).astype(np.float64)

    def value(f):
        return float(R.iq_loss(R.mlp_params(f, dims), acts, s, a, sp, done, Bp, xh=xh)[0])
    layers = R.mlp_params(flat, dims)
    loss, info = R.iq_loss(layers, acts, s, a, sp, done, Bp, xh=xh)
    loss.backward()
    g = R.flat_grad(layers)
    assert abs(info["softQloss"] + info["avg_R_expert_IQ"]) < 1e-15 and info["grad_pen"] > 0 and info["reg_loss"] > 0
    h = 1e-6
    for idx in np.random.default_rng(1).choice(flat.size, 15, replace=False):
        e = np.zeros_like(flat); e[idx] = h
        fd = (value(flat + e) - value(flat - e)) / (2 * h)
        assert abs(fd - g[idx]) <= 1e-6 * max(1.0, abs(fd)), (idx, fd, g[idx])


def test_eps_draws_follow_the_spec():
    e = R.eps(123, 456, 64)
    assert e.dtype == np.float32 and (e >= 0).all() and (e < 1).all() and len(set(e.tolist())) == 64
    for j in (0, 1, 63):
        x = CR.philox_oracle(123, 456, j, R.RNG_IQ_GP)
        want = np.float32(float(CR.u53(np.array([x[0]]), np.array([x[1]]))[0]))
        assert e[j] == want
