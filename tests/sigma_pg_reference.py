"""Float64 numpy restatement of the policy-gradient losses on two-headed Gaussian actors: ppo_loss (rl/ppo.jl:4-21), a2c_loss (rl/a2c.jl:4-15), reinforce_loss
(rl/reinforce.jl:4-13) and logpdf_bc_loss (il/bc.jl:10-18) of GaussianPolicy(mu, logSigma::ContinuousNetwork) / SquashedGaussianPolicy (policies.jl:315-350, 355-400). The
yardstick of tests/test_sigma_pg_reference.py (which pins it with float64 autograd) and tests/test_gpu_sigma_pg.py. Written from the equations, on top of
tests/sigma_head_reference.py (SR: the actor's Chain, logpdf, entropy, the cases) and tests/ensemble_reference.py (ER: the Chain passes, Adam64).

z = net(s), mu = z[:ad], l = z[ad:]; u = a (Gaussian) or atanh(clamp(a / ascale)) (squashed); sigma = exp(l) or exp(clamp(l, -5, 2)); lp_j = logpdf(s_j, a_j).
    ppo        r = exp(lp - old); p_loss = -mean(min(r A, clamp(r, 1 - eps, 1 + eps) A));  g = A where the unclipped term is the minimum, else 0
    a2c        p_loss = -mean(lp A); g = A, r = 1      reinforce: a2c with A = :return, lambda_p = 1, lambda_e = 0      bc: a2c with A = 1, old = 0, lambda_p = 1
    entropy    Gaussian: ENT0 + sum(l) -- ONE scalar over the whole minibatch (policies.jl:348: `sum` without dims); squashed: ENT0 + sum_d l per column (policies.jl:398)
    loss       lambda_p p_loss - lambda_e mean(entropy)
    seed       cf = -lambda_p g r;  dmu = cf (u - mu) / sigma^2 / B;  dl = cf ((u - mu)^2 / sigma^2 [clamp inactive] - 1) / B - lambda_e e,  e = 1 (Gaussian), 1 / B (squashed)
and [dmu; dl] goes through the Chain's backward pass.
"""
import numpy as np

import ensemble_reference as ER
import sigma_head_reference as SR

# two more shapes on SR's tables (SR.case / SR.tolerance read them by name): a 3-64-64-2 Pendulum actor has the dimensions of an instantiated register-resident learner shape
SR.SHAPES.setdefault("3-64-64-2x1", ((3, 64, 64, 2), ("relu", "relu", "identity"), 1))
SR.SHAPES.setdefault("3-64-64-2x1-tanh", ((3, 64, 64, 2), ("tanh", "tanh", "identity"), 1))
SR.CASE_SEED.setdefault("3-64-64-2x1", 35)
SR.CASE_SEED.setdefault("3-64-64-2x1-tanh", 36)

KINDS = ("ppo", "a2c", "reinforce", "bc")
LOSS_OF = {"ppo": "ppo", "a2c": "a2c", "reinforce": "reinforce", "bc": "logpdf_bc"}      # the names of crux.jl_amd/_lib.py: LOSS
EPS_CLIP = 0.2
# (shape, B, ascale, clamp): SR's step cases without the 4200-column one, the 3-64-64-2x1 shapes, the 17-wide shape at two more sizes, SR's three clamp variants
STEP_CASES = ([(n, B, sc, None) for n, B, sc in SR.STEP_CASES if B != 4200]
              + [("3-64-64-2x1", 37, 0.0, None), ("3-64-64-2x1", 128, 1.0, None), ("3-64-64-2x1", 257, 2.0, None), ("3-64-64-2x1-tanh", 1, 2.0, None)]
              + [("17-256-256-2x6", 257, 0.0, None), ("17-256-256-2x6", 300, 1.0, None)]
              + [("5-100-100-2x3", 37, 2.0, k) for k in (0, 1, 2)])


def lambda_e_of(kind, ascale):
    """bc: BC's default 1e-3; reinforce: none; ppo / a2c: PPO's default 0.1 for the squashed policy, 1e-3 for the plain one -- its entropy is a SUM over the minibatch, and at
    0.1 the logSigma bias gradient (about -0.1 B) sets a gradient scale under which over a quarter of a wide trunk counts as zero"""
    return 0.0 if kind == "reinforce" else 1e-3 if kind == "bc" else (0.1 if ascale > 0 else 1e-3)


def batch(name, B, ascale, kind, clamp=None):
    """SR.case plus the on-policy columns: stored actions from the policy (c["a"]), old logprob = logpdf + N(0, 0.3) in Float32 (about half the ratios leave [0.8, 1.2]),
    advantage and return ~ N(0, 1); bc: advantage 1, old logprob 0; reinforce: the return is the weight"""
    c = dict(SR.case(name, B, ascale, clamp))
    rng = np.random.default_rng(977 + 13 * B + int(10 * ascale) + (0 if clamp is None else 100 + clamp) + 1000 * SR.CASE_SEED[name])
    c["logprob"] = (SR.logpdf(c, c["s"], c["a"]) + rng.normal(0, 0.3, B)).astype(np.float32)
    c["advantage"] = rng.normal(0, 1, B).astype(np.float32); c["return"] = rng.normal(0, 1, B).astype(np.float32)
    c["kind"], c["lambda_p"], c["lambda_e"], c["eps_clip"] = kind, 1.0, lambda_e_of(kind, ascale), EPS_CLIP
    return c


def columns(c, kind):
    """(weight A, old logprob) of a kind, over the whole batch"""
    B = c["B"]
    if kind == "bc":
        return np.ones(B), np.zeros(B)
    return np.asarray(c["return"] if kind == "reinforce" else c["advantage"], np.float64), np.asarray(c["logprob"], np.float64)


def pg_loss(c, kind, idx=None, p=None, lambda_e=None):
    """(loss, info, flat gradient, seed [dmu; dl]) of the columns idx (all by default) at the parameters p (c["p"] by default)"""
    idx = np.arange(c["B"]) if idx is None else np.asarray(idx); B = idx.size; sc = c["ascale"]
    le = np.float64(np.float32(c["lambda_e"] if lambda_e is None else lambda_e)); lam_p = 1.0 if kind in ("reinforce", "bc") else np.float64(np.float32(c["lambda_p"]))
    if kind == "reinforce":
        le = 0.0
    s = np.asarray(c["s"], np.float64)[:, idx]; a = np.asarray(c["a"], np.float64)[:, idx]
    A, old = (x[idx] for x in columns(c, kind))
    mu, l, hs = SR.forward(c, s, p=p); sg = SR._sigma(c, l); s2 = sg * sg
    u = np.arctanh(np.clip(a / sc, np.float64(np.float32(-1.0) + np.float32(1e-5)), np.float64(np.float32(1.0) - np.float32(1e-5)))) if sc > 0 else a
    lp = SR._logprob(c, mu, l, u)
    eps = np.float64(np.float32(c["eps_clip"])); lo, hi = np.float64(np.float32(1.0) - np.float32(eps)), np.float64(np.float32(1.0) + np.float32(eps))
    if kind == "ppo":
        r = np.exp(lp - old); un, cl = r * A, np.clip(r, lo, hi) * A
        p_loss = -np.mean(np.minimum(un, cl)); g = np.where(un <= cl, A, 0.0); clip_fraction = float(np.mean((r > hi) | (r < lo)))
    else:
        r = np.ones(B); p_loss = -np.mean(lp * A); g = A; clip_fraction = 0.0
    ent = SR.ENT0 + (l.sum() / B if sc > 0 else l.sum())      # mean over the columns (squashed) / the scalar over everything (Gaussian)
    loss = lam_p * p_loss - le * ent
    cf = -lam_p * g * r; d = u - mu; inr = ((l >= -5.0) & (l <= 2.0)) if sc > 0 else 1.0
    dz = np.vstack([cf * d / s2 / B, cf * (d * d / s2 * inr - 1.0) / B - le * (1.0 / B if sc > 0 else 1.0)])
    grad = ER.backward(c["p"] if p is None else p, c["dims"], c["acts"], hs, dz)
    info = {"loss": float(loss), "entropy": float(ent), "kl": float(np.mean(old - lp)), "clip_fraction": clip_fraction, "avg_advantage": float(np.mean(A)),
            "avg_return": float(np.mean(np.asarray(c["return"], np.float64)[idx])), "grad_norm": float(np.sqrt(grad @ grad)), "ratio": r, "weight": A, "l": l}
    return float(loss), info, grad, dz


def pg_step(c, kind, lr=1e-3, idx=None, p=None, opt=None):
    """one train!: (info, gradient, parameters after the Adam step). A NaN norm updates nothing"""
    _, info, g, _ = pg_loss(c, kind, idx, p); p = np.asarray(c["p"] if p is None else p, np.float64)
    opt = ER.Adam64(p.size, lr=lr) if opt is None else opt
    return info, g, (p if np.isnan(info["grad_norm"]) else opt.step(p, g))


def pg_chain(c, kind, minibatches, lr=1e-3, target_kl=None):
    """the host loop of train! over a list of column-index arrays: (parameters, one info per step, the gradients). target_kl: stop after the first step whose kl exceeds it"""
    p = np.asarray(c["p"], np.float64); opt = ER.Adam64(p.size, lr=lr); infos, grads = [], []
    for idx in minibatches:
        info, g, p = pg_step(c, kind, lr, idx, p, opt); infos.append(info); grads.append(g)
        if target_kl is not None and info["kl"] > target_kl:
            break
    return p, infos, grads


def skipped_share(g):
    return ER.skipped_share(g)
