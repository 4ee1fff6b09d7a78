"""Float64 yardstick of ASAF's actor loss (src/model_free/il/asaf.jl:3-13) for a two-headed policy -- a GaussianPolicy / SquashedGaussianPolicy whose logSigma is a network on
mu's trunk -- for tests/test_asaf_sigma_reference.py and tests/test_gpu_asaf_sigma.py. The policy and its cases are tests/sigma_head_reference.py's (SR), the constants and
atanh(clamp(a / ascale)) are tests/asaf_reference.py's (AR). The loss is written from the reference's formulas with the per-column logSigma(s) and differentiated by torch
autograd: none of the closed forms of csrc/asaf.hip (the sigmoid weights, the seed [dmu; dl], the clamp mask, the entropy's share of dl) appears, so that those are checked.

    z = pi(s) [2 ad x B], mu = z[:ad], l = z[ad:]
    logpdf(pi, s, a)_j = sum_d [-(u - mu)^2 / (2 sigma^2) - 0.9189385 - l (- 2 (log 2 - u - softplus(-2 u)))],  sigma = exp(l) or exp(clamp(l, -5, 2)),  u = a or atanh(clamp(a / ascale))
    entropy(pi, s)     = 1.4189385 + sum(l)        GaussianPolicy: over the WHOLE matrix, one scalar (policies.jl:348), so mean(entropy) is that scalar
                       = 1.4189385 + sum_d l_j     SquashedGaussianPolicy: per column (:398)
    L = mean_E log(1 + exp(gE - logpdf(pi, s_E, a_E))) + mean_G log(exp(logpdf(pi, s, a) - gG) + 1) - 0.1 mean(entropy(pi, s))      (entropy over the rollout minibatch only)

A case (shape, n, ascale, N_E): the rollout minibatch is SR.case's own (s, a) (actions drawn from the policy itself); piG is the policy's parameters perturbed by N(0, 0.02);
the N_E demonstrations are actions of the policy at 1.5 times its noise on fresh states. gG and gE enter as float32 numbers, as the device columns they become.
"""
import functools

import numpy as np
import torch

import asaf_reference as AR
import cql_reference as CR
import ensemble_reference as ER
import sigma_head_reference as SR

LR = 1e-3
# (shape, n, ascale, N_E): n = 1 / 37 / 257 = a lone column, a ragged block, one past a block; N_E = 16400 reaches the second grid-stride sweep of the 64 head blocks
CASES = [("2-32-2x1", 37, 0.0, 21), ("2-32-2x1", 1, 2.0, 5), ("2-32-2x1", 37, 1.0, 16400), ("5-100-100-2x3", 37, 2.0, 75), ("5-100-100-2x3", 257, 0.0, 21),
         ("4-256-256-2x2", 257, 2.0, 21), ("4-256-256-2x2", 1, 2.0, 21), ("17-256-256-2x6", 37, 2.0, 75)]
CLAMP_CASE = ("5-100-100-2x3", 37, 1.0, 21)      # SR.case(..., clamp=0): logSigma head biases -6 / 0 / 3, below, inside and above the squashed head's clamp


@functools.lru_cache(maxsize=None)
def case(name, n, sc, NE, clamp=None):
    c = dict(SR.case(name, n, sc, clamp)); od, ad = c["od"], c["ad"]
    rng = np.random.default_rng(SR.CASE_SEED[name] * 100000 + n * 7 + int(10 * sc) + 31 * (NE % 9973) + (0 if clamp is None else 500 + clamp))
    c["NE"] = NE; c["pG"] = (c["p"].astype(np.float64) + rng.normal(0, 0.02, c["p"].size)).astype(np.float32)
    c["sE"] = np.asfortranarray(rng.normal(0, 1, (od, NE)).astype(np.float32))
    c["aE"] = np.asfortranarray(SR.explore(c, c["sE"], 1.5 * rng.normal(0, 1, (ad, NE)))[0].astype(np.float32))
    c["gG"] = _logpdf_np(c, c["pG"], c["s"], c["a"]).astype(np.float32)
    c["gE"] = _logpdf_np(c, c["pG"], c["sE"], c["aE"]).astype(np.float32)
    return c


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def logpdf_t(layers, c, s, a):
    """(logpdf(pi, s, a) [B], l [ad x B]) as torch float64"""
    ad, sc = c["ad"], c["ascale"]
    z = CR.mlp(layers, list(c["acts"]), _t(s)); mu, l = z[:ad], z[ad:]
    if sc > 0:
        u = AR.untanh(a, sc); s2 = torch.exp(torch.clamp(l, -5.0, 2.0)) ** 2
        corr = 2 * (AR.LOG2 - u - torch.nn.functional.softplus(-2 * u))
        return (-((u - mu) ** 2) / (2 * s2) - AR.LOG_SQRT_2PI - l - corr).sum(0), l
    s2 = torch.exp(l) ** 2
    return (-((_t(a) - mu) ** 2) / (2 * s2) - AR.LOG_SQRT_2PI - l).sum(0), l


def _logpdf_np(c, p, s, a):
    with torch.no_grad():
        return logpdf_t(CR.mlp_params(p, c["dims"]), c, s, a)[0].numpy()


def entropy_t(c, l):
    """entropy(pi, s): a scalar for the GaussianPolicy (the sum runs over everything), [B] for the squashed one"""
    return AR.ENTROPY_CONST + (l.sum(0) if c["ascale"] > 0 else l.sum())


def loss(c, layers):
    """asaf_actor_loss (asaf.jl:3-13): (loss, {entropy, expert, policy}) as torch float64"""
    l_g, l = logpdf_t(layers, c, c["s"], c["a"]); l_e, _ = logpdf_t(layers, c, c["sE"], c["aE"])
    expert = torch.log1p(torch.exp(_t(c["gE"]) - l_e)).mean()
    policy = torch.log1p(torch.exp(l_g - _t(c["gG"]))).mean()
    ent = entropy_t(c, l).mean()
    return expert + policy - 0.1 * ent, {"entropy": ent, "expert": expert, "policy": policy}


def step(c, clip=None, lr=LR):
    """one train!(pi, asaf_actor_loss): (info, flat gradient, parameters after Adam's first step); the norm is taken before ClipValue, the clamp before Adam"""
    layers = CR.mlp_params(c["p"], c["dims"]); L, parts = loss(c, layers); L.backward()
    g = CR.flat_grad(layers); gn = float(np.sqrt(g @ g))
    info = {"loss": float(L.detach()), "grad_norm": gn}; info.update({k: float(v.detach()) for k, v in parts.items()})
    p = ER.Adam64(g.size, lr=lr).step(np.asarray(c["p"], np.float64), AR.clip_value(g, clip))
    return info, g, p


def logpdf32_error(c):
    """the largest absolute error of the float32 restatement of logpdf(pi, s, a) against float64 over the case's own columns (the rollout rows and the demonstrations)"""
    e = 0.0
    for s, a in ((c["s"], c["a"]), (c["sE"], c["aE"])):
        e = max(e, float(np.abs(SR.logpdf(c, s, a, np.float32) - SR.logpdf(c, s, a)).max()))
    return e


def logpdf_tolerance(c):
    """absolute tolerance of the device's logpdf: SR.tolerance's rule (four times float32's own error) over the case's own columns"""
    return 4.0 * logpdf32_error(c)
