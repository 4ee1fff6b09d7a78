"""Plain NumPy reference of one policy-gradient minibatch for a conv Gaussian actor (csrc/conv_gauss.hip: crux_conv_pg_step_gauss): GaussianPolicy with a constant logSigma
(policies.jl:315-350) under ppo_loss / a2c_loss / reinforce_loss, every operand and intermediate in `dtype` (float64: the reference; float32: its restatement, whose error
against float64 sizes the tolerance). Trunk, head, critic and the norms are conv_pg_reference's; only the Gaussian head and the logSigma gradient are new.
tests/test_conv_gauss_reference.py pins the hand gradients against central differences of the float64 loss."""
import numpy as np

import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R

HALF_LOG_2PI, ENT0 = 0.9189385332046727, 1.4189385332046727


def gaussian(mu, a, ls, dtype):
    """log pi(a|s) = sum_d [-(a - mu)^2 / (2 sigma^2) - logSigma - log(2 pi) / 2] per column, d(logp)/d(mu) and d(logp)/d(logSigma) [ad x B]"""
    f = dtype.type; ls = ls.astype(dtype)[:, None]; s2 = np.exp(ls) ** 2; d = np.asarray(a).astype(dtype) - mu.astype(dtype)
    return (-(d * d) / (f(2) * s2) - f(HALF_LOG_2PI) - ls).sum(axis=0).astype(dtype), (d / s2).astype(dtype), (d * d / s2 - f(1)).astype(dtype)


def actor_seed(kind, mu, a, ls, adv, ret, oldlp, eps, lambda_p, lambda_e, dtype=np.float64):
    """loss, statistics, d(loss)/d(mu) [ad x B] and d(loss)/d(logSigma) [ad] of one minibatch. The entropy is the reference's 1.4189385 + sum(logSigma) (policies.jl:348)."""
    dtype = np.dtype(dtype); f = dtype.type; B = mu.shape[1]
    adv, ret, oldlp = (np.asarray(t).reshape(-1).astype(dtype) for t in (adv, ret, oldlp))
    logp, dmu, dls = gaussian(mu, a, ls, dtype)
    ratio = np.exp(logp - oldlp); lo, hi = f(1) - f(np.float32(eps)), f(1) + f(np.float32(eps))
    if kind == "ppo":
        u, cl = ratio * adv, np.clip(ratio, lo, hi) * adv
        p_loss = -np.minimum(u, cl).mean(); w = np.where(u <= cl, adv, 0) * ratio; clip_fraction = float(((ratio > hi) | (ratio < lo)).mean())
    else:
        if kind == "reinforce":
            adv, lambda_p, lambda_e = ret, 1.0, 0.0
        p_loss = -(logp * adv).mean(); w = adv; clip_fraction = 0.0
    lp, le = f(np.float32(lambda_p)), f(np.float32(lambda_e)); H = f(ENT0) + ls.astype(dtype).sum()
    wl = (-lp * w / f(B)).astype(dtype)      # d(loss)/d(logp) per column
    return {"loss": float(lp * p_loss - le * H), "entropy": float(H), "kl": float((oldlp - logp).mean()), "clip_fraction": clip_fraction, "ratio": ratio, "logp": logp,
            "dz": (wl[None, :] * dmu).astype(dtype), "g_ls": ((wl[None, :] * dls).sum(axis=1) - le).astype(dtype)}


def pg_reference(kind, sp, actor, ls, critic, s, a, adv, ret, oldlp, eps=0.2, lambda_p=1.0, lambda_e=0.1, dtype=np.float64):
    """one crux_conv_pg_step_gauss up to the gradients. actor, critic: (flat trunk parameters, flat head parameters without logSigma); critic None = no critic"""
    dtype = np.dtype(dtype); B = np.asarray(s).shape[1]; ad = len(ls); out = {}
    def seed_a(z):
        out.update(actor_seed(kind, z, a, ls, adv, ret, oldlp, eps, lambda_p, lambda_e, dtype)); return out["dz"]
    out["z"], out["g_trunk"], out["g_head"] = PG.network(sp, actor[0], PG.head_dims(sp, ad), actor[1], s, seed_a, dtype)
    if critic is not None:
        r = np.asarray(ret).reshape(1, -1).astype(dtype)
        def seed_c(v):
            out["critic_loss"] = float(((v - r) ** 2).mean()); out["critic_dabs"] = float(2 * np.abs(v - r).mean()); return (dtype.type(2) * (v - r) / dtype.type(B)).astype(dtype)
        out["v"], out["gc_trunk"], out["gc_head"] = PG.network(sp, critic[0], PG.head_dims(sp, 1), critic[1], s, seed_c, dtype)
    norm = lambda *gs: float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in gs)))      # noqa: E731
    out["grad_norm"] = norm(out["g_trunk"], out["g_head"], out["g_ls"])      # norm(grads) over Flux.params: trunk arrays, head arrays, logSigma
    if critic is not None:
        out["critic_grad_norm"] = norm(out["gc_trunk"], out["gc_head"])
    return out


def inputs(sp, B, ad, seed):
    """conv_pg_reference.inputs for a continuous action: parameters of both networks, kink-free byte-valued observations, a logSigma vector away from 0, actions around the
    actor's own mean, advantages of both signs, returns, and old log-probabilities around the actor's own so that some ratios fall outside 1 +- 0.2 and some inside"""
    rng = np.random.default_rng(seed); nets = []
    for nout in (ad, 1):
        dims = PG.head_dims(sp, nout)
        nets.append((CR.perturbed(CR.glorot_params(sp, rng), rng), R.perturbed_params(R.glorot_params(dims, rng), rng)))
    s = np.asfortranarray(rng.integers(0, 256, (sp["W"] * sp["H"] * sp["C"], B)).astype(np.float32)); bad = np.ones(B, bool)
    while bad.any():      # columns with a relu pre-activation of either network within 1e-4 of its kink are redrawn
        s[:, bad] = rng.integers(0, 256, (s.shape[0], int(bad.sum()))).astype(np.float32)
        bad = np.logical_or(*[CR._near_kink(pt, sp, s, 1e-4, head=(ph, PG.head_dims(sp, n), PG.ACTS)) for (pt, ph), n in zip(nets, (ad, 1))])
    ls = rng.uniform(-0.7, 0.3, ad).astype(np.float32)
    mu = CR.q_reference(sp, nets[0][0], PG.head_dims(sp, ad), PG.ACTS, nets[0][1], s)
    a = np.asfortranarray((mu + np.exp(ls.astype(np.float64))[:, None] * rng.normal(0, 1, (ad, B))).astype(np.float32))
    adv = rng.normal(0, 1, B).astype(np.float32); ret = rng.normal(0, 1, B).astype(np.float32)
    if B > 1:
        adv[0], adv[1] = abs(adv[0]), -abs(adv[1])
    logp = gaussian(mu, a, ls, np.dtype(np.float64))[0]
    shift = np.where(np.arange(B) % 2 == 0, rng.uniform(0.3, 0.5, B) * rng.choice([-1, 1], B), rng.uniform(-0.1, 0.1, B))      # log ratios: |.| >= 0.3 is outside 1 +- 0.2, |.| <= 0.1 inside
    return nets[0], ls, nets[1], s, a, adv, ret, (logp - shift).astype(np.float32)
