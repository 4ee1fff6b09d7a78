"""Float64 restatement of AdVIL's two losses and of OrthogonalRegularizer (src/model_free/il/AdVIL.jl:1-10, src/extras/orthogonal_regularization.jl) with torch
autograd: the yardstick of tests/test_gpu_advil.py. Everything here is written as the reference writes it -- W' * W masked by ones - I and norm(.)^2, the losses as
sums of means, the penalty through iq_reference.gradient_penalty (create_graph=True) -- and differentiated by autograd; none of the closed forms of csrc/advil.hip
(4 beta W R, the +-1/B seeds, the BC seed) appears, so that those are checked as well.

Draws: the penalty's eps_j = (float)u53(Philox(seed, counter, j, IQ_GP)) (iq_reference.eps); the batch loop's counter of minibatch g is 8g + 5.
"""
import numpy as np
import torch

import iq_reference as R

mlp_params, mlp, eps, xhat, gradient_penalty, flat_grad, adam_first_step = R.mlp_params, R.mlp, R.eps, R.xhat, R.gradient_penalty, R.flat_grad, R.adam_first_step

GP_TARGET = 0.4      # gradient_penalty(critic(pi), expert_sa, pi_sa, target=0.4f0) (AdVIL.jl:9)


def orth_reg(layers, beta=1.0):
    """OrthogonalRegularizer(beta)(pi) (orthogonal_regularization.jl:5-15) over [(W, b)]: beta sum_l norm((W' W) .* (ones - I))^2; biases have no `weight`"""
    reg = torch.zeros((), dtype=torch.float64)
    for W, _b in layers:
        prod = W.T @ W
        mat = torch.ones_like(prod) - torch.eye(prod.shape[0], dtype=prod.dtype)
        reg = reg + torch.linalg.norm(prod * mat) ** 2
    return beta * reg


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def policy_sa(a_layers, a_acts, s):
    """pi_sa = vcat(s, action(pi, s)) as float32 columns (what the interpolation of the penalty is formed from)"""
    with torch.no_grad():
        return np.concatenate([np.asarray(s, np.float32), mlp(a_layers, a_acts, _t(s)).numpy().astype(np.float32)], 0)


def advil_d_loss(a_layers, a_acts, d_layers, d_acts, s, a, lambda_gp=10.0, seed=0, counter=0, target=GP_TARGET):
    """advil_d_loss (AdVIL.jl:6-10): mean(value(pi, expert_sa)) - mean(value(pi, pi_sa)) + lambda_GP gradient_penalty(critic(pi), expert_sa, pi_sa, target=0.4).
    Returns (loss, {D_expert, D_policy, grad_pen, gp_loss}); the gradient of interest is the discriminator's."""
    s64, a64 = _t(s), _t(a)
    pi_sa = torch.cat([s64, mlp(a_layers, a_acts, s64)], 0)
    expert_sa = torch.cat([s64, a64], 0)
    xh = xhat(np.concatenate([np.asarray(s, np.float32), np.asarray(a, np.float32)], 0), policy_sa(a_layers, a_acts, s), eps(seed, counter, np.shape(s)[1]))
    de, dp = mlp(d_layers, d_acts, expert_sa).mean(), mlp(d_layers, d_acts, pi_sa).mean()
    P = gradient_penalty(d_layers, d_acts, xh, target=target)
    loss = de - dp + lambda_gp * P
    return loss, {"D_expert": de.item(), "D_policy": dp.item(), "grad_pen": P.item(), "gp_loss": (lambda_gp * P).item()}


def advil_pi_loss(a_layers, a_acts, d_layers, d_acts, s, a, lambda_bc=0.2):
    """advil_pi_loss (AdVIL.jl:1-4): mean(value(pi, s, pi_a)) + lambda_BC Flux.mse(pi_a, a). Returns (loss, {D_policy, bc_mse}); the gradient of interest is the actor's."""
    s64, a64 = _t(s), _t(a)
    pi_a = mlp(a_layers, a_acts, s64)
    dv = mlp(d_layers, d_acts, torch.cat([s64, pi_a], 0)).mean()
    mse = ((pi_a - a64) ** 2).mean()
    return dv + lambda_bc * mse, {"D_policy": dv.item(), "bc_mse": mse.item()}


class Adam64:
    """Flux's Adam in float64 over one flat vector"""

    def __init__(self, n, lr=3e-4, b1=0.9, b2=0.999, eps_=1e-8):
        self.m, self.v, self.bp, self.lr, self.b1, self.b2, self.eps = np.zeros(n), np.zeros(n), [b1, b2], lr, b1, b2, eps_

    def step(self, p, g):
        self.m = self.b1 * self.m + (1 - self.b1) * g; self.v = self.b2 * self.v + (1 - self.b2) * g * g
        out = p - self.lr * (self.m / (1 - self.bp[0])) / (np.sqrt(self.v / (1 - self.bp[1])) + self.eps)
        self.bp = [self.bp[0] * self.b1, self.bp[1] * self.b2]
        return out


def advil_loop(pa, pd, a_dims, a_acts, d_dims, d_acts, s, a, epochs, batch_size, lambda_gp=10.0, lambda_bc=0.2, beta=1e-4, lr=3e-4, seed=0, perm_seed=0):
    """solve(AdVIL) (batch.jl:38-85) as a plain loop in float64: epochs + 1 epochs, a fresh permutation per epoch, partition into minibatches (the last may be short),
    critic step, then the actor step on the same minibatch with the updated critic. Returns the two flat parameter vectors and the per-epoch mean infos."""
    pa, pd = np.asarray(pa, np.float64).copy(), np.asarray(pd, np.float64).copy()
    oa, od_ = Adam64(pa.size, lr), Adam64(pd.size, lr)
    rng = np.random.default_rng(perm_seed); n = np.shape(s)[1]; g = 0; hist = []
    for _ep in range(epochs + 1):
        order = rng.permutation(n); infos = []
        for k0 in range(0, n, batch_size):
            ids = order[k0:k0 + batch_size]; sb, ab = s[:, ids], a[:, ids]
            al, dl = mlp_params(pa, a_dims), mlp_params(pd, d_dims)
            ld, di = advil_d_loss(al, a_acts, dl, d_acts, sb, ab, lambda_gp, seed, 8 * g + 5)
            ld.backward(); pd = od_.step(pd, flat_grad(dl))
            al, dl = mlp_params(pa, a_dims), mlp_params(pd, d_dims)
            lp, pi_ = advil_pi_loss(al, a_acts, dl, d_acts, sb, ab, lambda_bc)
            tot = lp + orth_reg(al, beta)
            tot.backward(); pa = oa.step(pa, flat_grad(al))
            infos.append({"discriminator_loss": ld.item(), "actor_loss": tot.item(), "bc_mse": pi_["bc_mse"], "grad_pen": di["grad_pen"]})
            g += 1
        hist.append({k: float(np.mean([i[k] for i in infos])) for k in infos[0]})
    return pa, pd, hist


def bc_mse(pa, a_dims, a_acts, s, a):
    """mean((pi(s) - a)^2) over a held-out set"""
    with torch.no_grad():
        return float(((mlp(mlp_params(pa, a_dims), a_acts, _t(s)) - _t(a)) ** 2).mean())
