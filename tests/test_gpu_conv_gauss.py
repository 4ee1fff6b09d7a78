"""The policy-gradient step for a conv Gaussian actor (csrc/conv_gauss.hip) on the device.

1. One crux_conv_pg_step_gauss against conv_gauss_reference in float64 for ppo / a2c / reinforce. The tolerance is test_gpu_conv_pg.py's rule: a tensor (every parameter
   gradient of both networks, the logSigma gradient, the parameters after Adam) passes iff err <= M max(e32, u), M = conv_reference.M_MARGIN and e32 the float32
   restatement's error, both from the CPU alone. The seed dy lives in the step's scratch; it is checked through the head's last-layer gradients, which are its sums. The
   scalars pass within what that bound on mu (bz) allows -- log pi moves by at most blp = bz max_j sum_d |a - mu| / sigma^2 + ad bz^2 / (2 min sigma^2), a surrogate term by
   |A| ratio blp -- plus a few u of their own roundings; the entropy does not depend on mu. For PPO with B > 1 the reference's ratios lie on both sides of the clip.
2. A NaN observation: CRUX_ENAN, and trunk, head and logSigma of both networks untouched.
3. Two PPO iterations through solve on a HostMDP with a continuous action; SquashedGaussianPolicy over a conv chain still refuses by name."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_gauss_reference as GR
import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R
import parity
from parity import crux
from crux_jl_amd import _lib as L
from test_gpu_conv import _bound_check, _flat_slices
from test_gpu_conv_pg import ETA, _policy

pytestmark = pytest.mark.gpu
M, U = CR.M_MARGIN, CR.U32
_vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


def _actor(ctx, sp, params, ls):
    convs = [crux.Conv(ly["k"], ly["cin"], ly["cout"], ly["act"], ly["stride"], ly["pad"]) for ly in sp["layers"]]
    ch = crux.Chain(crux.Scale(sp["scale"]), *convs, crux.flatten, crux.Dense(CR.n_features(sp), PG.HIDDEN, "relu"), crux.Dense(PG.HIDDEN, len(ls)), input=(sp["W"], sp["H"], sp["C"]))
    pi = crux.GaussianPolicy(crux.ContinuousNetwork(ch, ctx=ctx), ls, ctx=ctx)
    pi.set_params(np.concatenate(list(params) + [ls])); pi.attach_optimizer(crux.Adam(np.float32(ETA)))
    return pi


def _step(ctx, kind, A, Cn, s, a, adv, ret, oldlp, eps, lp, le):
    """one crux_conv_pg_step_gauss on host inputs: (rc, actor info row, critic [loss, grad norm])"""
    arrs = [np.asfortranarray(s), np.asfortranarray(a, np.float32), adv, ret, oldlp]; d = [ctx.alloc(x.nbytes) for x in arrs]
    raw, craw = np.zeros(L.INFO_N, np.float32), np.zeros(2, np.float32)
    try:
        for dst, x in zip(d, arrs):
            ctx.h2d(dst, x)
        hc = (Cn.trunk.h, Cn.trunk.p.h, Cn.head_h) if Cn is not None else (None, None, None)
        rc = ctx.lib.crux_conv_pg_step_gauss(A.trunk.h, A.trunk.p.h, A.head_h, *hc, d[0], d[1], a.shape[0], d[2], d[3], d[4], s.shape[1], L.LOSS[kind], eps, lp, le, _vp(raw), _vp(craw))
    finally:
        for p in d:
            ctx.free(p)
    return rc, raw, craw


CASES = [(k, PG.PLAIN, B, ad, True) for k in ("ppo", "a2c", "reinforce") for B in (1, 33, 130) for ad in (1, 3)] + [("ppo", PG.VEC, 33, 3, True), ("reinforce", PG.PLAIN, 33, 3, False)]


@pytest.mark.parametrize("kind,sp,B,ad,with_critic", CASES, ids=["%s-%s-B%d-ad%d%s" % (k, "plain" if sp is PG.PLAIN else "vec", B, ad, "" if c else "-actor-only") for k, sp, B, ad, c in CASES])
def test_pg_step_gauss_matches_float64(gpu_ctx, kind, sp, B, ad, with_critic):
    ctx, eps, lp, le = gpu_ctx, 0.2, 0.7, 0.1
    actor, ls, critic, s, a, adv, ret, oldlp = GR.inputs(sp, B, ad, seed=60 + B + ad)
    if not with_critic:
        critic = None
    A, Cn = _actor(ctx, sp, actor, ls), (_policy(ctx, sp, 1, critic) if critic is not None else None)
    r64, r32 = (GR.pg_reference(kind, sp, actor, ls, critic, s, a, adv, ret, oldlp, eps, lp, le, t) for t in (np.float64, np.float32))
    if kind == "ppo" and B > 1:      # on the reference: ratios on both sides of the clip and inside it, none near its edges, advantages of both signs
        out = (r64["ratio"] > 1 + eps) | (r64["ratio"] < 1 - eps)
        assert (r64["ratio"] > 1 + eps).any() and (r64["ratio"] < 1 - eps).any() and (~out).any() and (adv > 0).any() and (adv < 0).any()
        assert np.minimum(np.abs(r64["ratio"] / (1 + np.float32(eps)) - 1), np.abs(r64["ratio"] / (1 - np.float32(eps)) - 1)).min() > 1e-3
    rc, raw, craw = _step(ctx, kind, A, Cn, s, a, adv, ret, oldlp, eps, lp, le)
    ctx.check(rc)
    nets = [("actor", A, actor, PG.head_dims(sp, ad), r64, r32, "g_", raw[L.INFO["grad_norm"]], r64["grad_norm"])]
    if Cn is not None:
        nets.append(("critic", Cn, critic, PG.head_dims(sp, 1), r64, r32, "gc_", craw[1], r64["critic_grad_norm"]))
    for tag, pi, p0, dims, q64, q32, key, norm, norm64 in nets:
        nt = pi.trunk.p.n_params; nl = R.n_layer_params(dims)
        gt, gh = (ctx.d2h(ctx.lib.crux_mlp_grads_ptr(h), np.empty(n, np.float32)) for h, n in ((pi.trunk.p.h, nt), (pi.head_h, pi.n_params - nt)))
        tensors = [(n, t, q64[key + "trunk"][i:j], q32[key + "trunk"][i:j]) for n, t, (i, j) in _flat_slices(tag + " trunk", gt, CR.layer_offsets(sp), [ly["cout"] for ly in sp["layers"]])]
        tensors += [(n, t, q64[key + "head"][i:j], q32[key + "head"][i:j]) for n, t, (i, j) in _flat_slices(tag + " head", gh[:nl], R.layer_offsets(dims), dims[1:])]
        p0 = list(p0)
        if tag == "actor":
            assert gh.size == nl + ad
            tensors.append(("actor dlogSigma", gh[nl:], r64["g_ls"], r32["g_ls"])); p0[1] = np.concatenate([p0[1], ls])
        _bound_check("%s B%d ad%d %s" % (kind, B, ad, tag), tensors)
        bn = np.sqrt(sum(t.size * (M * max(R.rel_err(t32, t64), U) * np.abs(t64).max()) ** 2 for _, t, t64, t32 in tensors))
        assert abs(norm - norm64) <= bn + 2 * U * norm64
        after = pi.get_params()
        for name, q0, q1, g in ((tag + " trunk", p0[0], after[:nt], gt), (tag + " head", p0[1], after[nt:], gh)):      # Flux Adam's first step on the device's own gradient
            small = CR.adam_small(q0, ETA); dlt = q1.astype(np.float64) - q0
            assert np.all(np.abs(dlt - CR.adam_first_step_delta(g, ETA)) <= small * ETA), name
            assert np.all(np.abs(dlt) <= ETA * (1 + small)) and CR.adam_sign_ok(q0, q1, g, ETA), name
    # the scalars: what the bound on mu allows
    bz = M * max(R.rel_err(r32["z"], r64["z"]), U) * np.abs(r64["z"]).max(); s2 = np.exp(ls.astype(np.float64))[:, None] ** 2; d = np.abs(a - r64["z"])
    blp = bz * (d / s2).sum(axis=0).max() + ad * bz * bz / (2 * s2.min()); mag = (d * d / (2 * s2) + GR.HALF_LOG_2PI + np.abs(ls)[:, None]).sum(axis=0).max()
    ent = GR.ENT0 + np.abs(ls).sum(); b_ent = 8 * U * ent; b_kl = blp + 8 * U * max(np.abs(oldlp).max(), mag)
    w = np.abs(ret if kind == "reinforce" else adv).astype(np.float64) * (r64["ratio"] if kind == "ppo" else 1.0); lpe, lee = (1.0, 0.0) if kind == "reinforce" else (lp, le)
    b_loss = lpe * w.mean() * blp * np.exp(blp) + lee * b_ent + 8 * U * (lpe * (w * np.maximum(1.0, mag)).mean() + lee * ent)
    print("PGG %s B%d ad%d loss %.9g ref %.9g bound %.3g | entropy %.9g ref %.9g bound %.3g | kl %.9g ref %.9g bound %.3g | clip %.6g ref %.6g" % (
        kind, B, ad, raw[0], r64["loss"], b_loss, raw[L.INFO["entropy"]], r64["entropy"], b_ent, raw[L.INFO["kl"]], r64["kl"], b_kl, raw[L.INFO["clip_fraction"]], r64["clip_fraction"]))
    assert abs(raw[L.INFO["loss"]] - r64["loss"]) <= b_loss and abs(raw[L.INFO["entropy"]] - r64["entropy"]) <= b_ent and abs(raw[L.INFO["kl"]] - r64["kl"]) <= b_kl
    assert raw[L.INFO["clip_fraction"]] == np.float32(r64["clip_fraction"])
    if Cn is not None:
        bv = M * max(R.rel_err(r32["v"], r64["v"]), U) * np.abs(r64["v"]).max()
        assert abs(craw[0] - r64["critic_loss"]) <= r64["critic_dabs"] * bv + bv * bv + 4 * U * r64["critic_loss"]


def test_nan_observation_leaves_trunk_head_and_logsigma_untouched(gpu_ctx):
    ctx, sp, B, ad = gpu_ctx, PG.PLAIN, 33, 3
    actor, ls, critic, s, a, adv, ret, oldlp = GR.inputs(sp, B, ad, seed=7)
    A, Cn = _actor(ctx, sp, actor, ls), _policy(ctx, sp, 1, critic)
    s = s.copy(order="F"); s[3, 5] = np.nan
    rc, _, _ = _step(ctx, "ppo", A, Cn, s, a, adv, ret, oldlp, 0.2, 1.0, 0.1)
    assert rc == L.ENAN
    assert np.array_equal(A.get_params(), np.concatenate(list(actor) + [ls])) and np.array_equal(Cn.get_params(), np.concatenate(critic))


def test_ppo_continuous_from_pixels_runs_and_squashed_still_refuses(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import ppo_pixels as px
    import ppo_pixels_continuous as ex
    env = ex.CatchContinuous(6, 6, seed=1); pi = ex.actor_critic(6, 6, seed=2, hidden=16, ctx=gpu_ctx); S = crux.ContinuousSpace((6, 6, 2))
    opt = lambda: {"batch_size": 16, "epochs": 2, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    store = []
    solver = crux.PPO(pi, S, N=64, dN=32, max_steps=6, a_opt=opt(), c_opt=opt(), interaction_storage=store)      # raises NotImplementedError without the Gaussian conv step
    before = [q.get_params() for q in (pi.A, pi.C)]; snap = []
    solver.post_batch_callback = (lambda f: lambda D, info: (snap.append(pi.A.get_params()), f(D, info)))(solver.post_batch_callback)      # the policy each block was sampled with
    crux.solve(solver, env.mdp())
    assert len(solver.history) == 2 and len(store) == 2 and len(snap) == 2
    for h in solver.history:
        assert all(np.isfinite(h[k]) for k in ("actor_loss", "actor_grad_norm", "kl", "entropy", "clip_fraction", "critic_loss", "critic_grad_norm")) and h["critic_batches_trained"] == 4
    for q, p0 in zip((pi.A, pi.C), before):
        nt = q.trunk.p.n_params; p1 = q.get_params()
        assert np.any(p1[:nt] != p0[:nt]) and np.any(p1[nt:] != p0[nt:])
    assert pi.A.get_params()[-1] != before[0][-1]      # logSigma trains
    now = pi.A.get_params()
    for blk, p in zip(store, snap):      # logprob of the stored actions under the policy that drew them: the explore kernel's logprob equals logpdf within the rule's bound
        pi.A.set_params(p); lp = pi.A.logpdf(blk["s"], blk["a"]); mu = pi.A.action(blk["s"]); s2 = float(np.exp(2.0 * pi.A.log_sigma()[0]))
        bz = M * U * np.abs(mu).max(); b = bz * (np.abs(blk["a"] - mu) / s2).max() + bz * bz / (2 * s2) + 8 * U * max(1.0, np.abs(lp).max())
        assert np.asarray(blk["logprob"]).size == 32 and np.abs(np.asarray(blk["logprob"]).reshape(-1) - lp.reshape(-1)).max() <= b
    pi.A.set_params(now)
    assert pi.A.entropy(store[0]["s"]) == np.float32(GR.ENT0) + pi.A.log_sigma()[0]
    with pytest.raises(NotImplementedError) as e:
        crux.SquashedGaussianPolicy(crux.ContinuousNetwork(px._chain(6, 6, 16, 1), ctx=gpu_ctx), np.zeros(1, np.float32), ctx=gpu_ctx)
    assert "SquashedGaussianPolicy" in str(e.value) and "conv" in str(e.value)
