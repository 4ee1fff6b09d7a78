"""Behaviour cloning from pixels (csrc/conv_bc.hip) on the device: crux_conv_bc_step and crux_conv_bc_loss against conv_bc_reference in float64 under the rule of
test_gpu_conv_pg.py / test_gpu_conv_gauss.py (a tensor passes iff err <= M max(e32, u); a scalar within what that bound on z allows plus a few u), the NaN gate, and crux.BC /
solve / loss_value on Catch demonstrations with what still refuses by BC's name."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_bc_reference as BR
import conv_gauss_reference as GR
import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R
import parity
import pool_reference as PR
from parity import crux
from crux_jl_amd import _lib as L
from test_gpu_conv import _bound_check, _flat_slices
from test_gpu_conv_pg import ETA

pytestmark = pytest.mark.gpu
M, U = CR.M_MARGIN, CR.U32
_vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
POOLED = PR.spec(7, 6, 2, [CR.layer((3, 3), 2, 5, "relu", 1, 1)], [PR.pool("max", 2)])


def _policy(ctx, form, sp, net, ls, gauss=None):
    """categorical: DiscreteNetwork; gaussian: GaussianPolicy; mse: ContinuousNetwork, or (gauss=True) GaussianPolicy"""
    lay = []
    for ly, q in zip(sp["layers"], sp.get("pools", [None] * len(sp["layers"]))):
        lay += [crux.Conv(ly["k"], ly["cin"], ly["cout"], ly["act"], ly["stride"], ly["pad"])] + ([crux.MaxPool(q["k"], q["stride"], q["pad"])] if q else [])
    dims = BR.head_dims(sp, 3)
    ch = crux.Chain(crux.Scale(sp["scale"]), *lay, crux.flatten, crux.Dense(dims[0], dims[1], "relu"), crux.Dense(dims[1], 3), input=(sp["W"], sp["H"], sp["C"]))
    gauss = form == "gaussian" if gauss is None else gauss
    pi = crux.DiscreteNetwork(ch, [0, 1, 2], ctx=ctx) if form == "categorical" else crux.ContinuousNetwork(ch, ctx=ctx)
    pi = crux.GaussianPolicy(pi, ls, ctx=ctx) if gauss else pi
    pi.set_params(np.concatenate(list(net) + ([ls] if gauss else []))); pi.attach_optimizer(crux.Adam(np.float32(ETA)))
    return pi


def _call(ctx, pi, form, s, a, le, chunk=None):
    """crux_conv_bc_step (chunk None: (rc, info row)) or crux_conv_bc_loss (rc, [loss, entropy, logpdf]) on host inputs"""
    arrs = [np.asfortranarray(s), np.asfortranarray(a.astype(np.uint8) if form == "categorical" else a.astype(np.float32))]; d = [ctx.alloc(x.nbytes) for x in arrs]
    out = np.zeros(L.INFO_N if chunk is None else 3, np.float32); h = (pi.trunk.h, pi.trunk.p.h, pi.head_h); loss = L.LOSS["mse_action" if form == "mse" else "logpdf_bc"]
    try:
        for dst, x in zip(d, arrs):
            ctx.h2d(dst, x)
        rc = ctx.lib.crux_conv_bc_step(*h, *d, 3, s.shape[1], loss, le, _vp(out)) if chunk is None else ctx.lib.crux_conv_bc_loss(*h, *d, 3, s.shape[1], chunk, loss, le, _vp(out))
    finally:
        for p in d:
            ctx.free(p)
    return rc, out


def _scalar_bounds(form, r64, r32, a, ls, le):
    """(loss, entropy, logpdf) bounds from the bound bz on z, as the two conv policy-gradient tests derive them (weight 1, ratio 1, lambda_p 1)"""
    bz = M * max(R.rel_err(r32["z"], r64["z"]), U) * np.abs(r64["z"]).max(); d = np.abs(a.astype(np.float64) - r64["z"])
    if form == "mse":
        return (2 * d * bz + bz * bz).mean() + 4 * U * r64["loss"], 0.0, 0.0
    if form == "categorical":
        logn = np.log(3.0); blp, mag, ent, b_ent = 2 * bz, abs(r64["logpdf"]), logn, 2 * logn * bz + 8 * U * logn
    else:
        s2 = np.exp(ls.astype(np.float64))[:, None] ** 2; blp = bz * (d / s2).sum(axis=0).max() + 3 * bz * bz / (2 * s2.min())
        mag = (d * d / (2 * s2) + GR.HALF_LOG_2PI + np.abs(ls)[:, None]).sum(axis=0).max(); ent = GR.ENT0 + np.abs(ls).sum(); b_ent = 8 * U * ent
    b_lp = blp + 8 * U * max(1.0, mag)
    return b_lp + le * b_ent + 8 * U * (max(1.0, mag) + le * ent), b_ent, b_lp


CASES = [(f, PG.PLAIN, B, None) for f in BR.FORMS for B in (1, 33, 130)] + [("categorical", PG.VEC, 33, None), ("categorical", POOLED, 33, None), ("mse", PG.PLAIN, 33, True)]


@pytest.mark.parametrize("form,sp,B,gauss", CASES, ids=["%s-%s-B%d%s" % (f, "plain" if sp is PG.PLAIN else "vec" if sp is PG.VEC else "pooled", B, "-gaussian-policy" if g else "") for f, sp, B, g in CASES])
def test_bc_step_matches_float64(gpu_ctx, form, sp, B, gauss):
    ctx, le = gpu_ctx, 0.05
    if sp is POOLED:      # N(0, 1) images away from every relu kink and max-pool tie of the float64 reference (pool_reference.clean_images)
        rng = np.random.default_rng(3); net = (CR.perturbed(CR.glorot_params(sp, rng), rng), R.perturbed_params(R.glorot_params(BR.head_dims(sp, 3), rng), rng))
        ls, s, a = None, PR.clean_images(net[0], sp, B, rng), np.asfortranarray(np.eye(3, dtype=bool)[:, rng.integers(0, 3, B)])
    else:
        net, ls, s, a = BR.inputs(form, sp, B, seed=80 + B)
    pi = _policy(ctx, form, sp, net, ls, gauss); has_ls = isinstance(pi, crux.GaussianPolicy)
    r64, r32 = (BR.bc_reference(form, sp, net, ls if has_ls else None, s, a, le, t) for t in (np.float64, np.float32))
    rc, raw = _call(ctx, pi, form, s, a, le); ctx.check(rc)
    nt = pi.trunk.p.n_params; dims = BR.head_dims(sp, 3); nl = R.n_layer_params(dims)
    gt, gh = (ctx.d2h(ctx.lib.crux_mlp_grads_ptr(h), np.empty(n, np.float32)) for h, n in ((pi.trunk.p.h, nt), (pi.head_h, pi.n_params - nt)))
    tensors = [(n, t, r64["g_trunk"][i:j], r32["g_trunk"][i:j]) for n, t, (i, j) in _flat_slices("trunk", gt, CR.layer_offsets(sp), [ly["cout"] for ly in sp["layers"]])]
    tensors += [(n, t, r64["g_head"][i:j], r32["g_head"][i:j]) for n, t, (i, j) in _flat_slices("head", gh[:nl], R.layer_offsets(dims), dims[1:])]
    p0 = [net[0], np.concatenate([net[1], ls]) if has_ls else net[1]]
    if form == "gaussian":
        tensors.append(("dlogSigma", gh[nl:], r64["g_ls"], r32["g_ls"]))
    _bound_check("bc %s B%d" % (form, B), tensors)
    bn = np.sqrt(sum(t.size * (M * max(R.rel_err(t32, t64), U) * np.abs(t64).max()) ** 2 for _, t, t64, t32 in tensors))
    assert abs(raw[L.INFO["grad_norm"]] - r64["grad_norm"]) <= bn + 2 * U * r64["grad_norm"]
    after = pi.get_params()
    if form == "mse" and has_ls:      # action(pi, s) = mu: a zero logSigma gradient, logSigma bit-unchanged
        assert not gh[nl:].any() and np.array_equal(after[nt + nl:].view(np.uint32), ls.view(np.uint32))
        p0[1], after, gh = net[1], after[:nt + nl], gh[:nl]
    for name, q0, q1, g in (("trunk", p0[0], after[:nt], gt), ("head", p0[1], after[nt:], gh)):      # Flux Adam's first step on the device's own gradient
        small = CR.adam_small(q0, ETA); dlt = q1.astype(np.float64) - q0
        assert np.all(np.abs(dlt - CR.adam_first_step_delta(g, ETA)) <= small * ETA), name
        assert np.all(np.abs(dlt) <= ETA * (1 + small)) and CR.adam_sign_ok(q0, q1, g, ETA), name
    b = _scalar_bounds(form, r64, r32, a, ls, le); got = (raw[L.INFO["loss"]], raw[L.INFO["entropy"]], raw[L.INFO["kl"]])
    print("BC %s B%d" % (form, B), got, [r64[k] for k in ("loss", "entropy", "logpdf")], b)
    assert all(abs(g - r64[k]) <= bk for g, k, bk in zip(got, ("loss", "entropy", "logpdf"), b))


@pytest.mark.parametrize("n", [70, 20])
@pytest.mark.parametrize("form", BR.FORMS)
def test_bc_loss_in_chunks_matches_float64_and_changes_nothing(gpu_ctx, form, n):
    ctx, le, sp = gpu_ctx, 0.05, PG.PLAIN
    net, ls, s, a = BR.inputs(form, sp, n, seed=90 + n)
    pi = _policy(ctx, form, sp, net, ls); hs = (pi.trunk.p.h, pi.head_h); sizes = (pi.trunk.p.n_params, pi.n_params - pi.trunk.p.n_params)
    r64, r32 = (BR.bc_reference(form, sp, net, ls if form == "gaussian" else None, s, a, le, t) for t in (np.float64, np.float32))
    rc, _ = _call(ctx, pi, form, s[:, :5], a[:, :5], le); ctx.check(rc)      # one step first: gradient buffers and Adam moments that are not all zero
    state = lambda: [pi.get_params(), *pi.adam_state()] + [ctx.d2h(ctx.lib.crux_mlp_grads_ptr(h), np.empty(k, np.float32)) for h, k in zip(hs, sizes)]      # noqa: E731
    pi.set_params(np.concatenate(list(net) + ([ls] if form == "gaussian" else []))); before = state()
    (rc1, o1), (rc2, o2) = _call(ctx, pi, form, s, a, le, chunk=33), _call(ctx, pi, form, s, a, le, chunk=33); ctx.check(rc1); ctx.check(rc2)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and all(x.tobytes() == y.tobytes() and x.any() for x, y in zip(before, state()))
    b = _scalar_bounds(form, r64, r32, a, ls, le)
    print("BCLOSS %s n%d" % (form, n), o1, [r64[k] for k in ("loss", "entropy", "logpdf")], b)
    assert all(abs(g - r64[k]) <= bk for g, k, bk in zip(o1, ("loss", "entropy", "logpdf"), b))


def test_nan_observation_leaves_trunk_head_and_logsigma_untouched(gpu_ctx):
    net, ls, s, a = BR.inputs("gaussian", PG.PLAIN, 33, seed=7)
    pi = _policy(gpu_ctx, "gaussian", PG.PLAIN, net, ls); s = s.copy(order="F"); s[3, 5] = np.nan
    rc, _ = _call(gpu_ctx, pi, "gaussian", s, a, 0.05)
    assert rc == L.ENAN and np.array_equal(pi.get_params(), np.concatenate(list(net) + [ls]))


def test_bc_through_the_public_interface(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import bc_pixels as ex
    env = ex.Catch(6, 6, seed=1); S = crux.ContinuousSpace((6, 6, 2)); demo = ex.demonstrations(env, S, 64, ctx=gpu_ctx)
    pi = ex.policy(6, 6, seed=2, hidden=16, ctx=gpu_ctx); nt = pi.trunk.p.n_params; p0 = pi.get_params()
    opt = lambda: {"batch_size": 16, "epochs": 2, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    solver = crux.BC(pi, S, demo, opt=opt(), window=1)      # raises NotImplementedError without the conv BC step
    crux.solve(solver)
    assert len(solver.history) == 3 and all(np.isfinite(h["loss"]) and np.isfinite(h["validation_error"]) and np.isfinite(h["entropy"]) for h in solver.history)
    assert np.any(pi.get_params()[:nt] != p0[:nt]) and np.any(pi.get_params()[nt:] != p0[nt:])
    assert 16 < len(solver.D_val) < 32 and solver.history[-1]["validation_error"] == crux.loss_value(pi, solver.a_opt, solver.P, solver.D_val)      # two chunks of at most 16 rows
    g = crux.GaussianPolicy(crux.ContinuousNetwork(ex.chain(6, 6, 16, 3), ctx=gpu_ctx), np.zeros(3, np.float32), ctx=gpu_ctx); g.two_headed = True      # (its constructor refuses the real thing)
    for call in (lambda: crux.BC(g, S, demo, two_headed=True), lambda: crux.BC(pi, S, demo, loss=crux.CustomLoss(lambda y, D, P: (0.0, y)))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value).startswith("BC") and "convolutional trunk" in str(e.value)
