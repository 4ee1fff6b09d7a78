"""MaxPool / MeanPool in the conv trunk (csrc/conv_pool.hip) on the device, against torch's float64 on the CPU (tests/pool_reference.py).

Bound of the trunk grid and the td step, per tensor: max |T - T64| <= (M max(e32, u) + mean_extra u) max |T64| with M = conv_reference.M_MARGIN, e32 the float32 restatement
and mean_extra the add-on of a mean pool (pool_reference.py's head; 0 for max). Max pooling routes a gradient by a comparison: the seeded observations are drawn so that in
the float64 reference every window's largest element leads the next by more than twice the forward bound (asserted here, on the reference alone)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_reference as CR
import dense_reference as R
import parity
import pool_reference as PR
from parity import crux
from crux_jl_amd import _lib as L
from test_gpu_conv import GSCALE, _Run, _flat_slices, _grad_tensors
from test_gpu_conv_ensemble import _Members, _ptrs
from test_gpu_wide import Handle
from test_pool_reference import host_spec

pytestmark = pytest.mark.gpu
M, U = PR.M_MARGIN, PR.U32
WINDOWS = list(PR.POOLS)


class _PRun(_Run):
    """test_gpu_conv._Run over a spec with pools"""

    def __init__(self, ctx, sp, params=None):
        self.ctx, self.sp, self.t = ctx, sp, crux.ConvTrunk(host_spec(sp), ctx=ctx, seed=7, stream=2)
        if params is not None:
            self.t.p.set_params(params)


def _bound_check(tag, tensors, extra):
    bad = []
    for name, t, t64, t32 in tensors:
        e32, eg = R.rel_err(t32, t64), R.rel_err(t, t64); allowed = M * max(e32, U) + extra * U
        print("POOL %s %s e32_u %.3f gpu_u %.3f allowed_u %.3f" % (tag, name, e32 / U, eg / U, allowed / U))
        if not eg <= allowed:
            bad.append((name, "gpu %.2f u" % (eg / U), "allowed %.2f u" % (allowed / U)))
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("where", [0, 1], ids=["inner", "last"])
@pytest.mark.parametrize("kind", ["max", "mean"])
@pytest.mark.parametrize("window", WINDOWS)
def test_pooled_trunk_matches_float64(gpu_ctx, window, kind, where, act, B):
    sp, p, x, dy, r64, r32 = PR.grid_case(window, kind, where, act, B)
    assert not PR.near_tie(r64, r32, sp).any() and not PR.near_kink(r64, sp).any()      # the condition on the inputs, on the reference alone
    y, dx, g = _PRun(gpu_ctx, sp, p)(x, dy)
    tensors = [("y", y, r64["y"], r32["y"]), ("dx", dx, r64["dx"], r32["dx"])]
    for name, t, l, k in _grad_tensors(g / GSCALE, sp):
        tensors.append((name, t, r64[k][l], r32[k][l]))
    _bound_check("%s %s %d %s B%d" % (window, kind, where, act, B), tensors, PR.mean_extra(r64, sp))


# ---- the pool kernels in isolation: a 1 x 1 identity Conv(3 => 3) hands the image on exactly (1 x + 0 ...), so Y_0 is the input bit for bit and d_dx is dY_0 --------------
def _identity_trunk(ctx, window, kind):
    k, s, p = PR.POOLS[window]
    sp = PR.spec(7, 6, 3, [CR.layer((1, 1), 3, 3, "identity")], [PR.pool(kind, k, s, p)])
    return sp, _PRun(ctx, sp, np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)]))


def _window_max_f32(img, q):
    """NumPy's float32 maximum over every window of img [W, H, C, B], padding as -inf"""
    (k1, k2), (s1, s2), (p1, p2) = q["k"], q["stride"], q["pad"]; W, H = img.shape[:2]; PW, PH = (W + 2 * p1 - k1) // s1 + 1, (H + 2 * p2 - k2) // s2 + 1
    pad = np.full((W + 2 * p1, H + 2 * p2) + img.shape[2:], -np.inf, np.float32); pad[p1:p1 + W, p2:p2 + H] = img
    out = np.full((PW, PH) + img.shape[2:], -np.inf, np.float32)
    for u1 in range(k1):
        for u2 in range(k2):
            out = np.maximum(out, pad[u1:u1 + s1 * (PW - 1) + 1:s1, u2:u2 + s2 * (PH - 1) + 1:s2])
    return out


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("kind", ["max", "mean"])
@pytest.mark.parametrize("window", WINDOWS)
def test_pool_kernels_alone(gpu_ctx, window, kind, B):
    """small integers: ties in nearly every window, and every sum exact in float32"""
    sp, run = _identity_trunk(gpu_ctx, window, kind); q = sp["pools"][0]; rng = np.random.default_rng(B)
    x = np.asfortranarray(rng.integers(-2, 3, (7 * 6 * 3, B)).astype(np.float32)); dy = np.asfortranarray(rng.integers(-4, 5, (PR.n_features(sp), B)).astype(np.float32))
    y, dx, _ = run(x, dy); y2, dx2, _ = run(x, dy)
    assert np.array_equal(y, y2) and np.array_equal(dx, dx2)      # two identical calls give identical bits
    r64 = PR.reference(run.t.p.get_params(), sp, x, dy, np.float64)
    if kind == "max":
        assert np.array_equal(y.view(np.uint32), _window_max_f32(x.reshape((7, 6, 3, B), order="F"), q).reshape((-1, B), order="F").view(np.uint32))
        assert np.array_equal(dx, r64["dx"])      # torch's choice among tied elements; sums of small integers
    else:
        assert np.array_equal(y, r64["y"].astype(np.float32))      # an exact sum and one correctly rounded division
        n_b = -(-q["k"][0] // q["stride"][0]) * -(-q["k"][1] // q["stride"][1])
        assert np.abs(dx - r64["dx"]).max() <= n_b * U * np.abs(dy).max() * n_b / (q["k"][0] * q["k"][1])      # an n_b-term sum (exact here) and one division
    covered = PR.reference(run.t.p.get_params(), sp.copy() | {"pools": [dict(q, kind="mean")]}, x, np.ones_like(dy), np.float64)["dx"] != 0
    assert covered.all() == (window == "3x2s2x1p1x0") and np.all(dx[~covered] == 0)      # dropped trailing rows / columns and, at stride > window, the gaps: exactly 0


# ---- pair and group: each member bit-identical to its single pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specs", [("3x3s2", "3x3s2"), ("3x3s2", "2x2s2")], ids=["equal", "fallback"])
def test_pooled_pair_equals_two_single_passes_bit_for_bit(gpu_ctx, specs):
    ctx, B = gpu_ctx, 33; rng = np.random.default_rng(5)
    sps = [PR.grid_spec(specs[0], "max", 0, "relu"), PR.grid_spec(specs[1], "max" if specs[0] == specs[1] else "mean", 0, "relu")]
    sps = [PR.spec(7, 6, 2, sp["layers"], [sp["pools"][0], PR.pool("mean", 2)]) for sp in sps]      # an inner and a last pool in every member
    ps = [CR.perturbed(CR.glorot_params(sp, rng), rng) for sp in sps]
    x = np.asfortranarray(rng.normal(0, 1, (84, B)).astype(np.float32)); dys = [np.asfortranarray(rng.normal(0, 1, (PR.n_features(sp), B)).astype(np.float32)) for sp in sps]
    single = [_PRun(ctx, sp, p)(x, dy) for sp, p, dy in zip(sps, ps, dys)]
    t = [_PRun(ctx, sp, p).t for sp, p in zip(sps, ps)]
    d = [ctx.alloc(a.nbytes) for a in (x, dys[0], dys[1], dys[0], dys[1], x, x)]      # x, dy0, dy1, y0, y1, dx0, dx1
    try:
        for dst, a in zip(d[:3], (x, dys[0], dys[1])):
            ctx.h2d(dst, a)
        ctx.check(ctx.lib.crux_conv_forward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[3], d[4]))
        ctx.check(ctx.lib.crux_conv_backward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[1], d[2], GSCALE, 1, d[5], d[6]))
        for m in range(2):
            got = (ctx.d2h(d[3 + m], np.empty_like(dys[m])), ctx.d2h(d[5 + m], np.empty_like(x)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(t[m].p.h), np.empty(ps[m].size, np.float32)))
            for name, a, b in zip(("y", "dx", "gradient"), got, single[m]):
                assert np.array_equal(a, b) and np.any(b), (m, name)
    finally:
        for p in d:
            ctx.free(p)


class _PMembers(_Members):
    def __init__(self, ctx, sp, dims, acts, pts, phs):
        self.ctx, self.t = ctx, [_PRun(ctx, sp, p).t for p in pts]
        self.heads = [Handle(ctx, dims, acts) for _ in phs]
        for h, p in zip(self.heads, phs):
            h.set(p)
        self.arrs = (_ptrs([t.h for t in self.t]), _ptrs([t.p.h for t in self.t]), _ptrs([h.h for h in self.heads]))


def test_pooled_group_of_five_equals_single_passes_bit_for_bit(gpu_ctx):
    Mn, B = 5, 33; rng = np.random.default_rng(9)      # groups of four share layer 0: the last group holds one member
    g = PR.grid_spec("3x2s2x1p1x0", "max", 0, "tanh"); sp = PR.spec(7, 6, 2, g["layers"], [g["pools"][0], PR.pool("mean", (3, 3), 2)])
    F = PR.n_features(sp); dims, acts = [F, 24, 3], ["tanh", "identity"]
    pts = [CR.perturbed(CR.glorot_params(sp, rng), rng) for _ in range(Mn)]; phs = [R.perturbed_params(R.glorot_params(dims, rng), rng) for _ in range(Mn)]
    x = np.asfortranarray(rng.normal(0, 1, (84, B)).astype(np.float32)); dys = [np.asfortranarray(rng.normal(0, 1, (3, B)).astype(np.float32)) for _ in range(Mn)]
    ref = _PMembers(gpu_ctx, sp, dims, acts, pts, phs); want = [ref.single(m, x, dys[m], F) for m in range(Mn)]
    got = _PMembers(gpu_ctx, sp, dims, acts, pts, phs).passes(x, dys, F)
    for m in range(Mn):
        for name, a, b in zip(("output", "d_dx of the head", "trunk gradient", "head gradient"), got[m], want[m]):
            assert np.array_equal(a, b) and np.any(b), (m, name)


# ---- one crux_conv_td_step on a pooled trunk --------------------------------------------------------------------------------------------------------------------------------
def test_td_step_on_a_pooled_trunk_matches_float64(gpu_ctx):
    ctx, B = gpu_ctx, 33; rng = np.random.default_rng(17)
    sp = PR.spec(7, 6, 2, [CR.layer((3, 3), 2, 5, "relu", 1, 1), CR.layer((3, 3), 5, 17, "tanh", 1, 1)], [PR.pool("max", 2), PR.pool("mean", (2, 2), 1)])
    F = PR.n_features(sp); dims, acts = [F, 32, 3], ["tanh", "identity"]
    ch = crux.Chain(crux.Conv((3, 3), 2, 5, "relu", pad=1), crux.MaxPool(2), crux.Conv((3, 3), 5, 17, "tanh", pad=1), crux.MeanPool((2, 2), stride=1), crux.flatten,
                    crux.Dense(F, 32, "tanh"), crux.Dense(32, 3), input=(7, 6, 2))
    pi = crux.DiscreteNetwork(ch, [1, 2, 3], seed=3, ctx=ctx); pi.set_params(CR.perturbed(pi.get_params(), rng)); nt = pi.trunk.p.n_params
    pt, ph = pi.get_params()[:nt], pi.get_params()[nt:]
    s = PR.clean_images(pt, sp, B, rng); a = np.asfortranarray(np.eye(3, dtype=bool)[:, rng.integers(0, 3, B)]); y = rng.normal(0, 1, B).astype(np.float32)
    d = {"s": s, "sp": s, "r": np.zeros((1, B), np.float32), "a": a, "done": np.zeros((1, B), bool), "episode_end": np.zeros((1, B), bool)}
    buf = crux.ExperienceBuffer(crux.ContinuousSpace((7, 6, 2)), crux.DiscreteSpace(3), B, [], ctx=ctx); buf.push_(d)
    pi.attach_optimizer(crux.Adam(np.float32(1e-3)))
    d_y = ctx.alloc(4 * B); raw = np.zeros(L.INFO_N, np.float32)
    try:
        ctx.h2d(d_y, y)
        ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_y, 0, raw.ctypes.data_as(C.c_void_p)))
        gt, gh = ctx.d2h(ctx.lib.crux_mlp_grads_ptr(pi.trunk.p.h), np.empty(nt, np.float32)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(pi.head_h), np.empty(ph.size, np.float32))
    finally:
        ctx.free(d_y)
    r64, r32 = (PR.td_reference(sp, pt, dims, acts, ph, s, a, y, t) for t in (np.float64, np.float32))
    assert not PR.near_tie(r64["trunk"], r32["trunk"], sp).any() and not PR.near_kink(r64["trunk"], sp).any()
    tensors = [(n, t, r64["g_trunk"][i:j], r32["g_trunk"][i:j]) for n, t, (i, j) in _flat_slices("trunk", gt, CR.layer_offsets(sp), [ly["cout"] for ly in sp["layers"]])]
    tensors += [(n, t, r64["g_head"][i:j], r32["g_head"][i:j]) for n, t, (i, j) in _flat_slices("head", gh, R.layer_offsets(dims), dims[1:])]
    _bound_check("td step", tensors, PR.mean_extra(r64["trunk"], sp))
    assert np.isfinite(raw[0]) and np.any(pi.get_params()[:nt] != pt) and np.any(pi.get_params()[nt:] != ph)


# ---- two iterations of DQN.solve and PPO.solve through a Chain with MaxPool ------------------------------------------------------------------------------------------------------
def test_dqn_and_ppo_solve_through_a_pooled_chain(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import dqn_pixels_pool as ex
    env = ex.Catch(6, 6, seed=1); S = crux.ContinuousSpace((6, 6, 2)); pi = ex.q_network(6, 6, seed=2, hidden=16, ctx=gpu_ctx)
    solver = crux.DQN(pi, S, N=24, dN=4, c_opt={"batch_size": 16, "optimizer": crux.Adam(np.float32(1e-3))}, buffer_size=64, buffer_init=16, max_steps=6)
    before = pi.get_params(); nt = pi.trunk.p.n_params
    crux.solve(solver, env.mdp())
    assert len(solver.history) == 2 and all(np.isfinite(h["critic_loss"]) and np.isfinite(h["critic_grad_norm"]) for h in solver.history)
    assert np.any(pi.get_params()[:nt] != before[:nt]) and np.any(pi.get_params()[nt:] != before[nt:])
    ac = crux.ActorCritic(crux.DiscreteNetwork(ex.pooled_chain(6, 6, 16, 3), [0, 1, 2], seed=3, ctx=gpu_ctx), crux.ContinuousNetwork(ex.pooled_chain(6, 6, 16, 1), seed=4, ctx=gpu_ctx))
    opt = lambda: {"batch_size": 16, "epochs": 2, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    ppo = crux.PPO(ac, S, N=64, dN=32, max_steps=6, a_opt=opt(), c_opt=opt()); before = [q.get_params() for q in (ac.A, ac.C)]
    crux.solve(ppo, env.mdp())
    assert len(ppo.history) == 2 and all(np.isfinite(h[k]) for h in ppo.history for k in ("actor_loss", "actor_grad_norm", "critic_loss", "critic_grad_norm"))
    for q, p0 in zip((ac.A, ac.C), before):
        n = q.trunk.p.n_params; p1 = q.get_params()
        assert np.any(p1[:n] != p0[:n]) and np.any(p1[n:] != p0[n:])


# ---- crux_conv_set_pool refuses by name ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pools,rc,word", [
    ([(1, 9, 2, 2, 2, 0, 0), None], L.EINVAL, "does not fit"),            # a window wider than the layer's 8 x 8 output
    ([(2, 2, 2, 1, 1, 2, 0), None], L.EINVAL, "does not fit"),            # pad >= window
    ([(1, 2, 2, 0, 2, 0, 0), None], L.EINVAL, "does not fit"),            # stride 0
    ([(3, 2, 2, 2, 2, 0, 0), None], L.EINVAL, "kind 3"),
    ([(1, 6, 6, 6, 6, 0, 0), None], L.EINVAL, "no longer fits"),          # the next Conv((3, 3)) on a 1 x 1 input
    ([None, (1, 17, 16, 1, 1, 0, 0)], L.EUNSUP, "256"),
], ids=["window", "pad", "stride", "kind", "next_conv", "window256"])
def test_set_pool_refusals_name_themselves_and_change_nothing(gpu_ctx, pools, rc, word):
    ctx = gpu_ctx
    t = crux.ConvTrunk(crux.ConvSpec(10, 10, 1, 1.0, [crux.Conv(3, 1, 4), crux.Conv(3, 4, 4)]), ctx=ctx)
    arr = (L.PoolLayer * 2)()
    for a, q in zip(arr, pools):
        if q:
            a.kind, a.k1, a.k2, a.stride1, a.stride2, a.pad1, a.pad2 = q
    got = ctx.lib.crux_conv_set_pool(t.h, arr)
    assert got == rc and int(ctx.lib.crux_conv_out_features(t.h)) == 6 * 6 * 4
    with pytest.raises(crux.CruxError) as e:
        ctx.check(got)
    assert "crux_conv_set_pool" in str(e.value) and word in str(e.value)
    arr[0].kind, arr[0].k1, arr[0].k2, arr[0].stride1, arr[0].stride2, arr[0].pad1, arr[0].pad2 = 1, 2, 2, 2, 2, 0, 0; arr[1].kind = 0
    ctx.check(ctx.lib.crux_conv_set_pool(t.h, arr)); assert int(ctx.lib.crux_conv_out_features(t.h)) == 2 * 2 * 4      # 8 x 8 -> 4 x 4 -> Conv 2 x 2
    arr[0].kind = 0
    ctx.check(ctx.lib.crux_conv_set_pool(t.h, arr)); assert int(ctx.lib.crux_conv_out_features(t.h)) == 6 * 6 * 4      # all kinds 0: a plain trunk again
