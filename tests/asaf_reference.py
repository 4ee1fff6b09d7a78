"""Float64 restatement of ASAF's actor loss (src/model_free/il/asaf.jl:1-21) and of the two log-densities it reads (src/policies.jl:333-336, :383-396) with torch
autograd: the yardstick of tests/test_gpu_asaf.py. Everything here is written from the reference's formulas -- the densities as sums over the action, the loss as
two means of log(1 + exp(.)) minus 0.1 times the entropy -- and differentiated by autograd; none of the closed forms of csrc/asaf.hip (the sigmoid weights, the seed
(a - mu) / sigma^2, the logSigma gradient with its clamp mask, the -0.1 per logSigma slot) appears, so that those are checked as well.

The frozen copy piG enters as numbers: gG = logpdf(piG, s, a) over the minibatch, gE = logpdf(piG, s_E, a_E) over all demonstrations (no gradient reaches them).
The Float32 constants of the reference stay Float32 constants: the clamp bounds -1f0 + 1f-5 and 1f0 - 1f-5 are formed in float32, and a / ascale is a float32
quotient (atanh is steep there: the float64 value of 1 - 1e-5 would move atanh by 7e-4).
"""
import numpy as np
import torch

import iq_reference as R

mlp_params, mlp, flat_grad, adam_first_step = R.mlp_params, R.mlp, R.flat_grad, R.adam_first_step

LOG_SQRT_2PI = float(np.float32(0.9189385332046727))       # the reference's 0.9189385332046727f0
ENTROPY_CONST = float(np.float32(1.4189385332046727))      # 1.4189385332046727f0
CLAMP_LO = float(np.float32(-1.0) + np.float32(1.0e-5))
CLAMP_HI = float(np.float32(1.0) - np.float32(1.0e-5))
LOG2 = float(np.log(np.float32(2.0)))                      # log(2.0f0)


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def params(p, dims):
    """the flat Flux vector of a (Squashed)GaussianPolicy: the mean network's layers, then logSigma; returns ([(W, b)], logSigma) as float64 leaves"""
    ad = dims[-1]
    p = np.asarray(p)
    layers = mlp_params(p[:p.size - ad], dims)
    ls = torch.tensor(np.asarray(p[p.size - ad:], np.float64), requires_grad=True)
    return layers, ls


def flat(layers, ls):
    g = ls.grad.numpy() if ls.grad is not None else np.zeros(ls.shape[0])
    return np.concatenate([flat_grad(layers), g])


def gaussian_logpdf(mu, ls, a):
    """gaussian_logpdf(mu, logSigma, a) (policies.jl:333-336): [B]"""
    s2 = torch.exp(ls)[:, None] ** 2
    return (-((a - mu) ** 2) / (2 * s2) - LOG_SQRT_2PI - ls[:, None]).sum(0)


def untanh(a, ascale):
    """atanh.(clamp.(a ./ ascale, -1f0 + 1f-5, 1f0 - 1f-5)) (policies.jl:396); the quotient and the bounds in float32"""
    t = (np.asarray(a, np.float32) / np.float32(ascale)).astype(np.float64)
    return torch.atanh(torch.clamp(_t(t), CLAMP_LO, CLAMP_HI))


def squashed_logprob(mu, ls, u):
    """squashed_gaussian_logprob(mu, logSigma, u) (policies.jl:383-386) of the un-tanh'd action u: sigma = exp(clamp(logSigma, -5, 2)), - logSigma unclamped"""
    s2 = torch.exp(torch.clamp(ls, -5.0, 2.0))[:, None] ** 2
    corr = 2 * (LOG2 - u - torch.nn.functional.softplus(-2 * u))
    return (-((u - mu) ** 2) / (2 * s2) - LOG_SQRT_2PI - ls[:, None] - corr).sum(0)


def logpdf(layers, acts, ls, s, a, ascale=0.0):
    """logpdf(pi, s, a) for a GaussianPolicy (ascale = 0) or a SquashedGaussianPolicy (ascale > 0): [B]"""
    mu = mlp(layers, acts, _t(s))
    if ascale > 0:
        return squashed_logprob(mu, ls, untanh(a, ascale))
    return gaussian_logpdf(mu, ls, _t(a))


def entropy(ls):
    """entropy(pi, s) of both policies (policies.jl:348, :398): 1.4189385 + sum(logSigma), independent of s"""
    return ENTROPY_CONST + ls.sum()


def asaf_loss(layers, acts, ls, s, a, gG, sE, aE, gE, ascale=0.0):
    """asaf_actor_loss (asaf.jl:3-13): mean(log(1 + exp(piG_E - pi_E))) + mean(log(exp(pi_G - piG_G) + 1)) - 0.1 mean(entropy(pi, s)).
    Returns (loss, {entropy, expert, policy})."""
    l_g = logpdf(layers, acts, ls, s, a, ascale)
    l_e = logpdf(layers, acts, ls, sE, aE, ascale)
    e = entropy(ls)
    expert = torch.log1p(torch.exp(_t(gE) - l_e)).mean()
    policy = torch.log1p(torch.exp(l_g - _t(gG))).mean()
    loss = expert + policy - 0.1 * e
    return loss, {"entropy": e.item(), "expert": expert.item(), "policy": policy.item()}


def frozen(p, dims, acts, s, a, ascale=0.0):
    """logpdf(piG, s, a) as plain numbers"""
    layers, ls = params(p, dims)
    with torch.no_grad():
        return logpdf(layers, acts, ls, s, a, ascale).numpy()


def clip_value(g, c):
    """Optimiser(ClipValue(c), ...): element-wise clamp; c None / <= 0 / inf = off"""
    if c is None or not (0 < c < np.inf):
        return g
    return np.clip(g, -c, c)
