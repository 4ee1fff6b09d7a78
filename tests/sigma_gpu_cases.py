"""Device objects of a tests/sigma_head_reference.py case (SR.case): the two-headed actor in the reference's idiom, the critics, the minibatch. Shared by
tests/test_gpu_cql_sigma.py and tests/test_gpu_asaf_sigma.py."""
import numpy as np

import parity
from parity import crux


def policy(dims, acts, ad, sc, ctx, **kw):
    """base = [Dense...]; mu = Chain(base..., Dense(h, ad)); logSigma = Chain(base..., Dense(h, ad))"""
    base = [crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(dims) - 2)]
    mu, ls = crux.Chain(*base, crux.Dense(dims[-2], ad)), crux.Chain(*base, crux.Dense(dims[-2], ad))
    return crux.SquashedGaussianPolicy(mu, ls, sc, ctx=ctx, **kw) if sc > 0 else crux.GaussianPolicy(mu, ls, ctx=ctx, **kw)


def actor(c, ctx, p=None):
    pi = policy(c["dims"], c["acts"], c["ad"], c["ascale"], ctx); pi.set_params(c["p"] if p is None else p); return pi


def qnet(c, key, ctx):
    q = crux.ContinuousNetwork(parity.chain(list(c["qdims"]), list(c["qacts"])), ctx=ctx); q.set_params(c[key]); return q


def batch(c, ctx, weight=None, s=None):
    B = c["B"]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), crux.ContinuousSpace(c["ad"]), B, [] if weight is None else ["weight"], ctx=ctx)
    d = {"s": c["s"] if s is None else s, "a": c["a"], "sp": c["sp"], "r": c["r"].reshape(1, B), "done": c["done"].reshape(1, B), "episode_end": np.zeros((1, B), bool)}
    if weight is not None:
        d["weight"] = np.asarray(weight, np.float32).reshape(1, B)
    b.push_(d); return b


def grads(net, ctx):
    g = np.empty(net.n_params, np.float32); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def state(nets):
    """(parameters, Adam moments and beta powers) of every handle, for bit comparisons"""
    out = []
    for n in nets:
        m, v, bp = n.adam_state() if getattr(n, "optimizer", None) is not None else (None, None, None)
        out.append((n.get_params().copy(), None if m is None else m.copy(), None if v is None else v.copy(), None if bp is None else np.array(bp).copy()))
    return out


def same(s1, s2):
    for a, b in zip(s1, s2):
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)
