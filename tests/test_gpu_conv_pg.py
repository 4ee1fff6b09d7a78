"""Paired conv trunks and the policy-gradient step over trunk + head (csrc/conv_pair.hip) on the device.

1. crux_conv_forward_pair / crux_conv_backward_pair equal two crux_conv_forward_cached / crux_conv_backward calls bit for bit (activations, every parameter gradient, d_dx),
   with equal layer tables and, through the fallback, with unequal ones.
2. One crux_conv_pg_step against conv_pg_reference in float64 for ppo / a2c / reinforce. The tolerance is test_gpu_conv.py's for crux_conv_td_step: a tensor passes iff
   err <= M max(e32, u) (M = conv_reference.M_MARGIN, e32 the float32 restatement's error, both from the CPU alone), the scalars within what that bound on the logits z (bz)
   and on the value v (bv) allows -- log pi moves by at most 2 bz, the entropy by 2 log(n) bz, a surrogate term by |A| ratio 2 bz -- plus a few u of their own roundings; the
   gradient norm within the norm of the tensors' bounds; the parameters after Adam as there. B = 1 holds one ratio, so both sides of the clip are asserted for B > 1.
3. A NaN observation: CRUX_ENAN and four untouched parameter vectors.  4. Two PPO iterations through solve on a HostMDP; LagrangePPO still refuses by name."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R
import parity
from parity import crux
from crux_jl_amd import _lib as L
from test_gpu_conv import GSCALE, _Run, _bound_check, _flat_slices

pytestmark = pytest.mark.gpu
M, U, ETA = CR.M_MARGIN, CR.U32, float(np.float32(1e-3))
OTHER = CR.spec(9, 7, 2, [CR.layer((3, 3), 2, 4, "tanh", 2)], scale=1.0 / 255.0)      # the same input extent as PLAIN, another layer table: the fallback
_vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.mark.parametrize("B", [1, 33, 130])      # one column, a ragged wave, 130 x 30 (PLAIN) and 130 x 4 (VEC) columns: more than one weight-gradient chunk of 512
@pytest.mark.parametrize("specs", [(PG.PLAIN, PG.PLAIN), (PG.VEC, PG.VEC), (PG.PLAIN, OTHER)], ids=["plain", "vec", "fallback"])
def test_pair_equals_two_single_passes_bit_for_bit(gpu_ctx, specs, B):
    ctx, rng = gpu_ctx, np.random.default_rng(B)
    ps = [CR.perturbed(CR.glorot_params(sp, rng), rng) for sp in specs]
    x = np.asfortranarray(rng.integers(0, 256, (specs[0]["W"] * specs[0]["H"] * specs[0]["C"], B)).astype(np.float32))
    dys = [np.asfortranarray(rng.normal(0, 1, (CR.n_features(sp), B)).astype(np.float32)) for sp in specs]
    single = [_Run(ctx, sp, p)(x, dy) for sp, p, dy in zip(specs, ps, dys)]
    t = [_Run(ctx, sp, p).t for sp, p in zip(specs, ps)]
    d = [ctx.alloc(a.nbytes) for a in (x, dys[0], dys[1], dys[0], dys[1], x, x)]      # x, dy0, dy1, y0, y1, dx0, dx1
    try:
        for dst, a in zip(d[:3], (x, dys[0], dys[1])):
            ctx.h2d(dst, a)
        for _ in range(2):      # two identical calls give identical bits
            ctx.check(ctx.lib.crux_conv_forward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[3], d[4]))
            ctx.check(ctx.lib.crux_conv_backward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[1], d[2], GSCALE, 1, d[5], d[6]))
            for m in range(2):
                y, dx, g = ctx.d2h(d[3 + m], np.empty_like(dys[m])), ctx.d2h(d[5 + m], np.empty_like(x)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(t[m].p.h), np.empty(ps[m].size, np.float32))
                for name, a, b in zip(("y", "dx", "gradient"), (y, dx, g), single[m]):
                    assert np.array_equal(a, b), (m, name)
    finally:
        for p in d:
            ctx.free(p)


def _policy(ctx, sp, nout, params):
    convs = [crux.Conv(ly["k"], ly["cin"], ly["cout"], ly["act"], ly["stride"], ly["pad"]) for ly in sp["layers"]]
    ch = crux.Chain(crux.Scale(sp["scale"]), *convs, crux.flatten, crux.Dense(CR.n_features(sp), PG.HIDDEN, "relu"), crux.Dense(PG.HIDDEN, nout), input=(sp["W"], sp["H"], sp["C"]))
    pi = crux.DiscreteNetwork(ch, list(range(nout)), ctx=ctx) if nout > 1 else crux.ContinuousNetwork(ch, ctx=ctx)
    pi.set_params(np.concatenate(params)); pi.attach_optimizer(crux.Adam(np.float32(ETA)))
    return pi


def _step(ctx, kind, A, Cn, s, a, adv, ret, oldlp, eps, lp, le):
    """one crux_conv_pg_step on host inputs: (rc, actor info row, critic [loss, grad norm])"""
    arrs = [np.asfortranarray(s), np.asfortranarray(a.astype(np.uint8)), adv, ret, oldlp]; d = [ctx.alloc(x.nbytes) for x in arrs]
    raw, craw = np.zeros(L.INFO_N, np.float32), np.zeros(2, np.float32)
    try:
        for dst, x in zip(d, arrs):
            ctx.h2d(dst, x)
        hc = (Cn.trunk.h, Cn.trunk.p.h, Cn.head_h) if Cn is not None else (None, None, None)
        rc = ctx.lib.crux_conv_pg_step(A.trunk.h, A.trunk.p.h, A.head_h, *hc, *d, s.shape[1], L.LOSS[kind], eps, lp, le, _vp(raw), _vp(craw))
    finally:
        for p in d:
            ctx.free(p)
    return rc, raw, craw


@pytest.mark.parametrize("kind,sp,B", [(k, PG.PLAIN, B) for k in ("ppo", "a2c", "reinforce") for B in (1, 33, 130)] + [("ppo", PG.VEC, 33)],
                         ids=lambda v: v if isinstance(v, str) else ("%dx%d" % (v["W"], v["H"]) if isinstance(v, dict) else "B%d" % v))
def test_pg_step_matches_float64(gpu_ctx, kind, sp, B):
    ctx, eps, lp, le = gpu_ctx, 0.2, 0.7, 0.1
    actor, critic, s, a, adv, ret, oldlp = PG.inputs(sp, B, seed=40 + B)
    if kind == "reinforce":
        critic = None
    A, Cn = _policy(ctx, sp, PG.N_ACTIONS, actor), (_policy(ctx, sp, 1, critic) if critic is not None else None)
    r64, r32 = (PG.pg_reference(kind, sp, actor, critic, s, a, adv, ret, oldlp, eps, lp, le, t) for t in (np.float64, np.float32))
    if kind == "ppo" and B > 1:      # on the reference: ratios on both sides of the clip, none near its edges, advantages of both signs
        out = (r64["ratio"] > 1 + eps) | (r64["ratio"] < 1 - eps)
        assert out.any() and (~out).any() and (adv > 0).any() and (adv < 0).any()
        assert np.minimum(np.abs(r64["ratio"] / (1 + np.float32(eps)) - 1), np.abs(r64["ratio"] / (1 - np.float32(eps)) - 1)).min() > 1e-3
    rc, raw, craw = _step(ctx, kind, A, Cn, s, a, adv, ret, oldlp, eps, lp, le)
    ctx.check(rc)
    nets = [("actor", A, actor, PG.head_dims(sp, PG.N_ACTIONS), r64["g_trunk"], r64["g_head"], r32["g_trunk"], r32["g_head"], raw[L.INFO["grad_norm"]], r64["grad_norm"])]
    if Cn is not None:
        nets.append(("critic", Cn, critic, PG.head_dims(sp, 1), r64["gc_trunk"], r64["gc_head"], r32["gc_trunk"], r32["gc_head"], craw[1], r64["critic_grad_norm"]))
    for tag, pi, p0, dims, gt64, gh64, gt32, gh32, norm, norm64 in nets:
        nt = pi.trunk.p.n_params
        gt, gh = (ctx.d2h(ctx.lib.crux_mlp_grads_ptr(h), np.empty(n, np.float32)) for h, n in ((pi.trunk.p.h, nt), (pi.head_h, pi.n_params - nt)))
        tensors = [(n, t, gt64[i:j], gt32[i:j]) for n, t, (i, j) in _flat_slices(tag + " trunk", gt, CR.layer_offsets(sp), [ly["cout"] for ly in sp["layers"]])]
        tensors += [(n, t, gh64[i:j], gh32[i:j]) for n, t, (i, j) in _flat_slices(tag + " head", gh, R.layer_offsets(dims), dims[1:])]
        _bound_check("%s B%d %s" % (kind, B, tag), tensors)
        bn = np.sqrt(sum(t.size * (M * max(R.rel_err(t32, t64), U) * np.abs(t64).max()) ** 2 for _, t, t64, t32 in tensors))
        assert abs(norm - norm64) <= bn + 2 * U * norm64
        after = pi.get_params()
        for name, q0, q1, g in ((tag + " trunk", p0[0], after[:nt], gt), (tag + " head", p0[1], after[nt:], gh)):      # Flux Adam's first step on the device's own gradient
            small = CR.adam_small(q0, ETA); dlt = q1.astype(np.float64) - q0
            assert np.all(np.abs(dlt - CR.adam_first_step_delta(g, ETA)) <= small * ETA), name
            assert np.all(np.abs(dlt) <= ETA * (1 + small)) and CR.adam_sign_ok(q0, q1, g, ETA), name
    # the scalars: what the bound on the logits allows
    bz = M * max(R.rel_err(r32["z"], r64["z"]), U) * np.abs(r64["z"]).max(); logn = np.log(PG.N_ACTIONS)
    b_ent = 2 * logn * bz + 8 * U * logn; b_kl = 2 * bz + 8 * U * max(np.abs(oldlp).max(), np.abs(r64["logp"]).max())
    w = np.abs(ret if kind == "reinforce" else adv).astype(np.float64) * (r64["ratio"] if kind == "ppo" else 1.0); lpe, lee = (1.0, 0.0) if kind == "reinforce" else (lp, le)
    b_loss = lpe * w.mean() * 2 * bz * np.exp(2 * bz) + lee * b_ent + 8 * U * (lpe * (w * np.maximum(1.0, np.abs(r64["logp"]))).mean() + lee * logn)
    print("PG %s B%d loss %.9g ref %.9g bound %.3g | entropy %.9g ref %.9g bound %.3g | kl %.9g ref %.9g bound %.3g | clip %.6g ref %.6g" % (
        kind, B, raw[0], r64["loss"], b_loss, raw[L.INFO["entropy"]], r64["entropy"], b_ent, raw[L.INFO["kl"]], r64["kl"], b_kl, raw[L.INFO["clip_fraction"]], r64["clip_fraction"]))
    assert abs(raw[L.INFO["loss"]] - r64["loss"]) <= b_loss and abs(raw[L.INFO["entropy"]] - r64["entropy"]) <= b_ent and abs(raw[L.INFO["kl"]] - r64["kl"]) <= b_kl
    assert raw[L.INFO["clip_fraction"]] == np.float32(r64["clip_fraction"])
    if Cn is not None:
        bv = M * max(R.rel_err(r32["v"], r64["v"]), U) * np.abs(r64["v"]).max()
        assert abs(craw[0] - r64["critic_loss"]) <= r64["critic_dabs"] * bv + bv * bv + 4 * U * r64["critic_loss"]


def test_nan_observation_leaves_all_four_parameter_vectors_untouched(gpu_ctx):
    ctx, sp, B = gpu_ctx, PG.PLAIN, 33
    actor, critic, s, a, adv, ret, oldlp = PG.inputs(sp, B, seed=7)
    A, Cn = _policy(ctx, sp, PG.N_ACTIONS, actor), _policy(ctx, sp, 1, critic)
    s = s.copy(order="F"); s[3, 5] = np.nan
    rc, _, _ = _step(ctx, "ppo", A, Cn, s, a, adv, ret, oldlp, 0.2, 1.0, 0.1)
    assert rc == L.ENAN
    assert np.array_equal(A.get_params(), np.concatenate(actor)) and np.array_equal(Cn.get_params(), np.concatenate(critic))


def test_ppo_from_pixels_runs_and_lagrange_ppo_still_refuses(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import ppo_pixels as ex
    env = ex.Catch(6, 6, seed=1); pi = ex.actor_critic(6, 6, seed=2, hidden=16, ctx=gpu_ctx); S = crux.ContinuousSpace((6, 6, 2))
    opt = lambda: {"batch_size": 16, "epochs": 2, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    solver = crux.PPO(pi, S, N=64, dN=32, max_steps=6, a_opt=opt(), c_opt=opt())      # raises NotImplementedError without the conv policy-gradient step
    before = [q.get_params() for q in (pi.A, pi.C)]
    crux.solve(solver, env.mdp())
    assert len(solver.history) == 2
    for h in solver.history:
        assert all(np.isfinite(h[k]) for k in ("actor_loss", "actor_grad_norm", "kl", "entropy", "clip_fraction", "critic_loss", "critic_grad_norm")) and h["critic_batches_trained"] == 4
    for q, p0 in zip((pi.A, pi.C), before):
        nt = q.trunk.p.n_params; p1 = q.get_params()
        assert np.any(p1[:nt] != p0[:nt]) and np.any(p1[nt:] != p0[nt:])
    mlp_v = crux.ContinuousNetwork(parity.chain([72, 8, 1], ["relu", "identity"]), ctx=gpu_ctx)
    for who, call in (("LagrangePPO", lambda: crux.LagrangePPO(pi, pi.C, S)), ("A2C", lambda: crux.A2C(crux.ActorCritic(pi.A, mlp_v), S))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value).startswith(who) and "convolutional trunk" in str(e.value)
