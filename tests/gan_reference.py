"""Float64 restatement of the five discriminator losses Lᴰ of src/extras/gans.jl as gail_d_loss calls them (on_policy_gail.jl:1-5: x = a, yD = (s,), wD = 1f0), differentiated
by torch autograd: the yardstick of tests/test_gpu_gan_losses.py. With z = D(vcat(a, s)), each mean over its own half:

  BCE    gans.jl:9      logitbinarycrossentropy(z_E, 1) + logitbinarycrossentropy(z_pi, 0)
  LS     gans.jl:14     mse(sigmoid(z_E), 1) + mse(sigmoid(z_pi), 0)
  Hinge  gans.jl:19     mean(relu(1 + (-2 wD + 1) z_E)) + mean(relu(1 + z_pi)) = mean(relu(1 - z_E)) + mean(relu(1 + z_pi))
  W      gans.jl:24     mean(z_pi) - mean((2 wD - 1) z_E) = mean(z_pi) - mean(z_E)
  WGP    gans.jl:34-40  W + lambda gradient_penalty(D, x_E, x_pi) (src/extras/gradient_penalty.jl, target = 1f0): iq_reference.gradient_penalty (create_graph=True) on
                        xhat = eps x_pi + (1 - eps) x_E with iq_reference's draw eps_j = (float)u53(Philox(seed, counter, j, IQ_GP))

Nothing here is written as a derivative: every gradient comes from autograd (torch's relu has derivative 0 at 0, the rule the device takes as Zygote's). The sigmoid of
LS is the one the loss names, it is not a seed.
"""
import numpy as np
import torch

import iq_reference as IQ
import nda_gail_reference as NR

KINDS = {"BCE": 0, "LS": 1, "Hinge": 2, "W": 3, "WGP": 4}      # CRUX_GAN_* of include/cruxhip.h
mlp_params, mlp, flat_grad, adam_first_step, vcat_as = IQ.mlp_params, IQ.mlp, IQ.flat_grad, IQ.adam_first_step, NR.vcat_as


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def loss_of_z(kind, ze, zp):
    """Lᴰ without a penalty from the two halves of the discriminator's output (torch tensors of any shape): a torch scalar"""
    if kind == "BCE":
        bce = torch.nn.functional.binary_cross_entropy_with_logits
        return bce(ze, torch.ones_like(ze)) + bce(zp, torch.zeros_like(zp))
    if kind == "LS":
        return ((torch.sigmoid(ze) - 1.0) ** 2).mean() + (torch.sigmoid(zp) ** 2).mean()
    if kind == "Hinge":
        return torch.relu(1.0 - ze).mean() + torch.relu(1.0 + zp).mean()
    if kind in ("W", "WGP"):
        return zp.mean() - ze.mean()
    raise KeyError(kind)


def wgp_xhat(x_ex, x_pi, seed, counter):
    """the penalty's columns: iq_reference's draw and its float32 interpolation (x = the expert half, xtilde = the policy half)"""
    x_ex, x_pi = np.asarray(x_ex, np.float32), np.asarray(x_pi, np.float32)
    if x_ex.shape != x_pi.shape:
        raise ValueError("DimensionMismatch: gradient_penalty broadcasts %r against %r" % (x_ex.shape, x_pi.shape))
    return IQ.xhat(x_ex, x_pi, IQ.eps(seed, counter, x_ex.shape[1]))


def d_loss(kind, layers, acts, x_ex, x_pi, lam=10.0, seed=0, counter=0):
    """Lᴰ(gan_loss, D, a_E, a_pi, yD = (s_E,), yG = (s_pi,)) on x = vcat(a, s) of both halves: a torch scalar"""
    ze, zp = mlp(layers, acts, _t(x_ex))[0], mlp(layers, acts, _t(x_pi))[0]
    loss = loss_of_z(kind, ze, zp)
    if kind == "WGP":
        loss = loss + float(np.float32(lam)) * IQ.gradient_penalty(layers, acts, wgp_xhat(x_ex, x_pi, seed, counter))
    return loss


def d_step(kind, p, dims, acts, x_ex, x_pi, lam=10.0, seed=0, counter=0):
    """loss and the flat float64 gradient of one discriminator step"""
    layers = mlp_params(p, dims)
    loss = d_loss(kind, layers, acts, x_ex, x_pi, lam, seed, counter)
    loss.backward()
    return loss.item(), flat_grad(layers)


def dz(kind, z, n_ex):
    """d Lᴰ / d z by autograd for a given output row z [n_ex + n_pi] (no penalty): what a head's seeds must equal"""
    zt = torch.tensor(np.asarray(z, np.float64).reshape(-1), requires_grad=True)
    loss_of_z(kind, zt[:n_ex], zt[n_ex:]).backward()
    return zt.grad.numpy()


def abs_seed_grad(kind, p, dims, acts, x_ex, x_pi):
    """the flat gradient of sum_j |dL/dz_j| z_j: the loss's own pull on every column (autograd's, held constant), with both halves pulling the same way. An entry where
    the loss's gradient is exactly zero and this one is not is a CANCELLATION between columns (under W: a relu unit that is on in every column, the output bias), not a
    dead unit. Float32 arithmetic leaves a rounding residue there in any summation order -- the Float32 reference does too -- and float64 lands on zero only as far as
    its own summation order happens to; so tests that compare exact zeros ask their inputs to hold none (tests/test_gan_reference.py)."""
    layers = mlp_params(p, dims); n_ex = np.asarray(x_ex).shape[1]
    z = mlp(layers, acts, _t(np.concatenate([np.asarray(x_ex, np.float64), np.asarray(x_pi, np.float64)], 1)))[0]
    w = np.abs(dz("W" if kind == "WGP" else kind, z.detach().numpy(), n_ex))
    (z * _t(w)).sum().backward()
    return flat_grad(layers)
