"""Float64 restatement of OnlineIQLearn's critic loss and of gradient_penalty (src/model_free/il/iqlearn.jl:49-95, src/extras/gradient_penalty.jl) with torch
autograd (create_graph=True for the penalty's input gradient): the yardstick of tests/test_gpu_iq.py. Alongside it, the closed-form seeds and the two-sweep
parameter gradient of the penalty that csrc/iq.hip implements, written out in numpy.

Draws: eps_j = (float)u53(Philox(seed, counter, j, IQ_GP)) for penalty column j (include/crux_rng.h), Philox from tests/cql_reference.py.
"""
import numpy as np
import torch

import cql_reference as CR

RNG_IQ_GP = 11
mlp_params, mlp, adam_first_step = CR.mlp_params, CR.mlp, CR.adam_first_step


def flat_grad(layers):
    """the flat parameter gradient; a leaf the loss does not reach (the biases under the penalty of a linear network) counts as zero"""
    z = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))
    return np.concatenate([np.concatenate([z(W).reshape(-1, order="F"), z(b)]) for W, b in layers])


def eps(seed, counter, H):
    x = CR.philox(seed, counter, np.arange(H), RNG_IQ_GP)
    return CR.u53(x[0], x[1]).astype(np.float32)


def xhat(x, xtilde, e):
    """eps xtilde + (1 - eps) x in float32, as the reference's broadcast computes it"""
    x, xt, e = np.asarray(x, np.float32), np.asarray(xtilde, np.float32), np.asarray(e, np.float32)[None, :]
    return (e * xt + (np.float32(1) - e) * x).astype(np.float32)


def gradient_penalty(layers, acts, x, target=1.0):
    """gradient_penalty(D, x; target) with the graph kept: mean_j (|d sum(D(x)) / dx_j| - target)^2"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    out = mlp(layers, acts, xt)
    g, = torch.autograd.grad(out.sum(), xt, create_graph=True)
    return ((torch.sqrt((g * g).sum(0)) - target) ** 2).mean()


def iq_loss(layers, acts, s, a, sp, done, n_policy, gamma=0.9, reg=True, alpha_reg=0.5, gp=True, lambda_gp=10.0, xh=None):
    """iq_loss (iqlearn.jl:49-95) over a minibatch whose columns [0, n_policy) are buffer rows and the rest demo rows; xh: the interpolated penalty states.
    Returns (loss, dict of the six info values)."""
    s, sp = torch.as_tensor(np.asarray(s, np.float64)), torch.as_tensor(np.asarray(sp, np.float64))
    a = torch.as_tensor(np.asarray(a, np.float64)); d = torch.as_tensor(np.asarray(done, np.float64).reshape(-1))
    Q, Qp = mlp(layers, acts, s), mlp(layers, acts, sp)
    V, Vp = torch.logsumexp(Q, 0), torch.logsumexp(Qp, 0)
    y = gamma * (1 - d) * Vp
    R = (Q * a).sum(0) - y
    ex = torch.arange(R.numel()) >= n_policy
    p1 = (-R[ex]).mean(); p2 = (V - y).mean()
    loss = p1 + p2
    info = {"softQloss": p1, "valueloss": p2, "avg_R_expert_IQ": -p1, "avg_R_demo_IQ": R[~ex].mean(), "grad_pen": torch.zeros((), dtype=torch.float64),
            "reg_loss": torch.zeros((), dtype=torch.float64)}
    if gp:
        info["grad_pen"] = lambda_gp * gradient_penalty(layers, acts, xh)
        loss = loss + info["grad_pen"]
    if reg:
        info["reg_loss"] = 1 / (4 * alpha_reg) * (R ** 2).mean()
        loss = loss + info["reg_loss"]
    return loss, {k: float(v) for k, v in info.items()}


# ---- the closed forms of csrc/iq.hip in numpy (float64) -----------------------------------------------------------------------------------------------------------
def _act(act, z):
    return np.maximum(z, 0) if act == "relu" else np.tanh(z) if act == "tanh" else z


def _d1(act, h):
    return (h > 0).astype(np.float64) if act == "relu" else 1 - h * h if act == "tanh" else np.ones_like(h)


def _d2(act, h):
    return -2 * h * (1 - h * h) if act == "tanh" else np.zeros_like(h)


def np_forward(Ws, bs, acts, x):
    hs = [np.asarray(x, np.float64)]
    for W, b, act in zip(Ws, bs, acts):
        hs.append(_act(act, W @ hs[-1] + b[:, None]))
    return hs


def np_penalty_grad(Ws, bs, acts, x, target=1.0, lam=1.0):
    """lambda dP/dtheta by the two sweeps of iq.hip's header: returns (P, [dW_l], [db_l])"""
    L, H = len(Ws), x.shape[1]
    hs = np_forward(Ws, bs, acts, x)
    delta, g = [None] * (L + 1), [None] * (L + 1)
    g[L] = np.ones_like(hs[L])
    delta[L] = _d1(acts[L - 1], hs[L]) * g[L]
    for l in range(L, 0, -1):
        g[l - 1] = Ws[l - 1].T @ delta[l]
        if l > 1:
            delta[l - 1] = _d1(acts[l - 2], hs[l - 1]) * g[l - 1]
    n = np.sqrt((g[0] ** 2).sum(0))
    P = ((n - target) ** 2).mean()
    gbar = lam * 2 * (n - target) * g[0] / n / H
    dW = [np.zeros_like(W) for W in Ws]; db = [np.zeros_like(b) for b in bs]; z2 = [None] * (L + 1)
    for l in range(1, L + 1):
        dW[l - 1] += delta[l] @ gbar.T
        dbar = Ws[l - 1] @ gbar
        z2[l] = dbar * g[l] * _d2(acts[l - 1], hs[l])
        gbar = _d1(acts[l - 1], hs[l]) * dbar
    hb = np.zeros_like(hs[L])
    for l in range(L, 0, -1):
        zb = z2[l] + _d1(acts[l - 1], hs[l]) * hb
        dW[l - 1] += zb @ hs[l - 1].T
        db[l - 1] += zb.sum(1)
        hb = Ws[l - 1].T @ zb
    return P, dW, db


def np_iq_seeds(Q, Qp, a, done, n_policy, gamma=0.9, reg=True, alpha_reg=0.5):
    """dL/dQ(s) and dL/dQ(s') of iq_loss without the penalty (the seeds of k_iq_head)"""
    B = Q.shape[1]; Be = B - n_policy
    def lse(v):
        m = v.max(0); return m + np.log(np.exp(v - m).sum(0))
    p, pp = np.exp(Q - lse(Q)), np.exp(Qp - lse(Qp))
    gd = gamma * (1 - np.asarray(done, np.float64).reshape(-1))
    R = (Q * a).sum(0) - gd * lse(Qp)
    dR = -(np.arange(B) >= n_policy).astype(np.float64) / Be + (R / (2 * alpha_reg * B) if reg else 0)
    return dR[None, :] * a + p / B, ((-dR - 1 / B) * gd)[None, :] * pp
