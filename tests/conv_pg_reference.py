"""Plain NumPy reference of one policy-gradient minibatch over trunk + dense head (csrc/conv_pair.hip: crux_conv_pg_step): the categorical head with the reference's eps
(policies.jl:135,152-155), ppo_loss / a2c_loss / reinforce_loss (rl/ppo.jl:4-21, a2c.jl:4-15, reinforce.jl:4-13), the critic's Flux.mse, and their gradients written out by
hand, every operand and intermediate in `dtype`. The trunk is conv_reference.trunk_reference, the head dense_reference.chain_reference. tests/test_conv_pg_reference.py pins
the hand gradients against torch autograd in float64."""
import numpy as np

import conv_reference as CR
import dense_reference as R

EPS = float(np.finfo(np.float32).eps)

# the shapes of tests/test_gpu_conv_pg.py: a non-VEC layer 0 whose cout fills no tile, with asymmetric kernel, stride and padding, then a second layer; and a trunk whose
# layer 0 meets the VEC conditions (k1, s1 multiples of 4, no padding along W, W a multiple of 4)
PLAIN = CR.spec(9, 7, 2, [CR.layer((3, 2), 2, 5, "relu", (2, 1), (1, 0)), CR.layer((2, 2), 5, 3, "relu")], scale=1.0 / 255.0)
VEC = CR.spec(8, 8, 4, [CR.layer((4, 4), 4, 6, "relu", 4)], scale=1.0 / 255.0)
N_ACTIONS, HIDDEN, ACTS = 3, 16, ["relu", "identity"]


def head_dims(sp, nout):
    return [CR.n_features(sp), HIDDEN, nout]


def categorical(z, a, dtype):
    """softmax over the columns' logits (max-subtracted), log pi(a|s) = log(sum(p .* onehot)), entropy = -sum(p .* log(p .+ eps)); and d(logp)/dz, d(entropy)/dz [n x B]"""
    e = np.exp(z - z.max(axis=0, keepdims=True)); p = (e / e.sum(axis=0, keepdims=True)).astype(dtype); a = np.asarray(a).astype(dtype)
    q = (p * a).sum(axis=0); lg = np.log(p + dtype.type(EPS))
    H = -(p * lg).sum(axis=0); h = -lg - p / (p + dtype.type(EPS))
    return np.log(q).astype(dtype), H.astype(dtype), (p * a / q - p).astype(dtype), (p * (h - (h * p).sum(axis=0, keepdims=True))).astype(dtype)


def actor_seed(kind, z, a, adv, ret, oldlp, eps, lambda_p, lambda_e, dtype=np.float64):
    """loss, statistics and d(loss)/d(logits) of one minibatch; kind in ppo / a2c / reinforce"""
    dtype = np.dtype(dtype); f = dtype.type; B = z.shape[1]
    adv, ret, oldlp = (np.asarray(t).reshape(-1).astype(dtype) for t in (adv, ret, oldlp))
    logp, H, dlogp, dH = categorical(z.astype(dtype), a, dtype)
    ratio = np.exp(logp - oldlp)
    if kind == "ppo":
        u, cl = ratio * adv, np.clip(ratio, f(1) - f(np.float32(eps)), f(1) + f(np.float32(eps))) * adv
        p_loss = -np.minimum(u, cl).mean(); w = np.where(u <= cl, adv, 0) * ratio
        clip_fraction = float(((ratio > f(1) + f(np.float32(eps))) | (ratio < f(1) - f(np.float32(eps)))).mean())
    else:
        if kind == "reinforce":
            adv, lambda_p, lambda_e = ret, 1.0, 0.0
        p_loss = -(logp * adv).mean(); w = adv; clip_fraction = 0.0
    lp, le = f(np.float32(lambda_p)), f(np.float32(lambda_e))
    dz = ((-lp * w[None, :] * dlogp - le * dH) / f(B)).astype(dtype)
    return {"loss": float(lp * p_loss - le * H.mean()), "entropy": float(H.mean()), "kl": float((oldlp - logp).mean()), "clip_fraction": clip_fraction, "ratio": ratio, "logp": logp, "dz": dz}


def network(sp, p_trunk, dims, p_head, s, seed_fn, dtype=np.float64):
    """forward through trunk and head, seed_fn(output) -> d(loss)/d(output), back through both: (output, flat trunk gradient, flat head gradient)"""
    f = CR.trunk_reference(p_trunk, sp, s, np.zeros((CR.n_features(sp), np.asarray(s).shape[1])), dtype, want_dx=False)["y"]
    z = CR.q_reference(sp, p_trunk, dims, ACTS, p_head, s, dtype)
    rh = R.chain_reference(p_head, dims, ACTS, f, seed_fn(z), dtype)
    rt = CR.trunk_reference(p_trunk, sp, s, rh["dx"], dtype, want_dx=False)
    return z, CR.flat_gradient(rt, sp), R.flat_gradient(rh, dims)


def pg_reference(kind, sp, actor, critic, s, a, adv, ret, oldlp, eps=0.2, lambda_p=1.0, lambda_e=0.1, dtype=np.float64):
    """one crux_conv_pg_step up to the gradients. actor, critic: (flat trunk parameters, flat head parameters); critic None = no critic (reinforce)"""
    dtype = np.dtype(dtype); B = np.asarray(s).shape[1]; out = {}
    def seed_a(z):
        out.update(actor_seed(kind, z, a, adv, ret, oldlp, eps, lambda_p, lambda_e, dtype)); return out["dz"]
    out["z"], out["g_trunk"], out["g_head"] = network(sp, actor[0], head_dims(sp, N_ACTIONS), actor[1], s, seed_a, dtype)
    if critic is not None:
        r = np.asarray(ret).reshape(1, -1).astype(dtype)
        def seed_c(v):
            out["critic_loss"] = float(((v - r) ** 2).mean()); out["critic_dabs"] = float(2 * np.abs(v - r).mean()); return (dtype.type(2) * (v - r) / dtype.type(B)).astype(dtype)
        out["v"], out["gc_trunk"], out["gc_head"] = network(sp, critic[0], head_dims(sp, 1), critic[1], s, seed_c, dtype)
    norm = lambda *gs: float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in gs)))      # noqa: E731
    out["grad_norm"] = norm(out["g_trunk"], out["g_head"])
    if critic is not None:
        out["critic_grad_norm"] = norm(out["gc_trunk"], out["gc_head"])
    return out


def inputs(sp, B, seed, kind="ppo", eps=0.2):
    """parameters of both networks, kink-free byte-valued observations, one-hot actions, advantages of both signs, returns, and old log-probabilities drawn around the
    actor's own so that some ratios fall outside 1 +- eps and some inside"""
    rng = np.random.default_rng(seed); nets = []
    for nout in (N_ACTIONS, 1):
        dims = head_dims(sp, nout)
        nets.append((CR.perturbed(CR.glorot_params(sp, rng), rng), R.perturbed_params(R.glorot_params(dims, rng), rng)))
    s = np.asfortranarray(rng.integers(0, 256, (sp["W"] * sp["H"] * sp["C"], B)).astype(np.float32)); bad = np.ones(B, bool)
    while bad.any():      # columns with a relu pre-activation of either network within 1e-4 of its kink are redrawn
        s[:, bad] = rng.integers(0, 256, (s.shape[0], int(bad.sum()))).astype(np.float32)
        bad = np.logical_or(*[CR._near_kink(pt, sp, s, 1e-4, head=(ph, head_dims(sp, n), ACTS)) for (pt, ph), n in zip(nets, (N_ACTIONS, 1))])
    a = np.asfortranarray(np.eye(N_ACTIONS, dtype=bool)[:, rng.integers(0, N_ACTIONS, B)])
    adv = rng.normal(0, 1, B).astype(np.float32); ret = rng.normal(0, 1, B).astype(np.float32)
    if B > 1:
        adv[0], adv[1] = abs(adv[0]), -abs(adv[1])
    logp = categorical(CR.q_reference(sp, nets[0][0], head_dims(sp, N_ACTIONS), ACTS, nets[0][1], s), a, np.dtype(np.float64))[0]
    shift = np.where(np.arange(B) % 2 == 0, rng.uniform(0.3, 0.5, B) * rng.choice([-1, 1], B), rng.uniform(-0.1, 0.1, B))      # log ratios: |.| >= 0.3 is outside 1 +- 0.2, |.| <= 0.1 inside
    return nets[0], nets[1], s, a, adv, ret, (logp - shift).astype(np.float32)
