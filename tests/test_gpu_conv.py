"""The convolutional trunk (csrc/conv.hip) and DQN over trunk + head against float64, through the C ABI and the host mirror (crux.jl_amd/conv.py).

Grid: forward / dX / dW / db of every case of conv_reference.grid_cases against trunk_reference(float64) under err <= M max(e32, u) per tensor (err = max |T - T64| / max |T64|,
e32 the same for the float32 NumPy restatement, M = conv_reference.M_MARGIN from the CPU alone), grad_scale = 0.5. relu members draw kink-free observations; no entry is
left out of any comparison. Further: Flux's flip on the hand example, the input scale as one Float32 multiply, bit-reproducibility (two runs; one handle at B = 37, 129, 37
against a fresh one; the want_param_grads / d_dx flags), crux_conv_dqn_target and one crux_conv_td_step on a staged batch of 32, the host mirror, and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_reference as CR
import dense_reference as R
import parity
from parity import crux
from crux_jl_amd import _lib as L

pytestmark = pytest.mark.gpu
GSCALE = 0.5      # != 1 and a power of two: the scaled gradient is compared without a rounding of the test's own
M, U = CR.M_MARGIN, CR.U32


def host_spec(sp):
    return crux.ConvSpec(sp["W"], sp["H"], sp["C"], sp["scale"], [crux.Conv(ly["k"], ly["cin"], ly["cout"], ly["act"], ly["stride"], ly["pad"]) for ly in sp["layers"]])


class _Run:
    """forward + pullback of one trunk through the C ABI"""

    def __init__(self, ctx, sp, params=None):
        self.ctx, self.sp, self.t = ctx, sp, crux.ConvTrunk(host_spec(sp), ctx=ctx, seed=7, stream=2)
        if params is not None:
            self.t.p.set_params(params)

    def __call__(self, x, dy, want_g=1, want_dx=True, cached=True):
        ctx, t, B = self.ctx, self.t, x.shape[1]
        d_x, d_dy, d_y, d_dx = ctx.alloc(x.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
            ctx.check((ctx.lib.crux_conv_forward_cached if cached else ctx.lib.crux_conv_forward)(t.h, t.p.h, d_x, B, d_y))
            ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_dy, GSCALE, want_g, d_dx if want_dx else None))
            y, dx, g = np.empty_like(dy), np.empty_like(x), np.empty(t.p.n_params, np.float32)
            ctx.d2h(d_y, y); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(t.p.h), g)
            if want_dx:
                ctx.d2h(d_dx, dx)
            return y, (dx if want_dx else None), g
        finally:
            for d in (d_x, d_dy, d_y, d_dx):
                ctx.free(d)


def _grad_tensors(g, sp):
    out = []
    for l, ((wo, bo), ly) in enumerate(zip(CR.layer_offsets(sp), sp["layers"])):
        out.append(("dW%d" % l, g[wo:bo].reshape(ly["k"] + (ly["cin"], ly["cout"]), order="F"), l, "dW")); out.append(("db%d" % l, g[bo:bo + ly["cout"]], l, "db"))
    return out


def _bound_check(tag, tensors):
    """[(name, T_gpu, T_64, T_32)] under err <= M max(e32, u); prints every figure before it asserts"""
    bad = []
    for name, t, t64, t32 in tensors:
        e32, eg = R.rel_err(t32, t64), R.rel_err(t, t64); ratio = eg / max(e32, U)
        print("CONV %s %s e32_u %.3f gpu_u %.3f ratio %.3f" % (tag, name, e32 / U, eg / U, ratio))
        if not eg <= M * max(e32, U):
            bad.append((name, "e32 %.2f u" % (e32 / U), "gpu %.2f u" % (eg / U), "ratio %.2f > M = %.2f" % (ratio, M)))
    assert not bad, bad


@pytest.mark.parametrize("case", CR.grid_cases(), ids=CR.case_id)
def test_trunk_matches_float64_on_the_grid(gpu_ctx, case):
    sp, B = case
    p, x, dy = CR.case_inputs(case)
    y, dx, g = _Run(gpu_ctx, sp, p)(x, dy)
    r64, r32 = CR.trunk_reference(p, sp, x, dy, np.float64), CR.trunk_reference(p, sp, x, dy, np.float32)
    tensors = [("y", y, r64["y"], r32["y"]), ("dx", dx, r64["dx"], r32["dx"])]
    for name, t, l, kind in _grad_tensors(g / GSCALE, sp):
        tensors.append((name, t, r64[kind][l], r32[kind][l]))
    _bound_check(CR.case_id(case), tensors)
    if sp["layers"][0]["stride"] == (3, 3):      # stride > kernel: the inputs no window covers have a gradient of exactly 0
        d = dx.reshape((sp["W"], sp["H"], B), order="F")
        assert np.all(d[2::3] == 0) and np.all(d[:, 2::3] == 0) and np.count_nonzero(d) == np.count_nonzero(r64["dx"])


def test_flip_hand_example_through_the_c_abi(gpu_ctx):
    """Conv((2,1), 1=>1), weight [a, b], input [x1, x2, x3]: [a x2 + b x1, a x3 + b x2] -- exact in Float32 for these integers"""
    sp = CR.spec(3, 1, 1, [CR.layer((2, 1), 1, 1)]); a, b = 2.0, -3.0
    x = np.asfortranarray(np.array([[5.0, 1.0], [7.0, 0.0], [11.0, -2.0]], np.float32)); dy = np.ones((2, 2), np.float32, order="F")
    y, dx, g = _Run(gpu_ctx, sp, np.array([a, b, 0.5], np.float32))(x, dy)
    assert np.array_equal(y[:, 0], [a * 7 + b * 5 + 0.5, a * 11 + b * 7 + 0.5]) and np.array_equal(y[:, 1], [b * 1 + 0.5, a * -2 + 0.5])
    assert np.array_equal(g / GSCALE, [7 + 11 + 0 - 2, 5 + 7 + 1 + 0, 4.0]) and np.array_equal(dx[:, 0], [b, a + b, a])


def test_input_scale_is_one_multiply_to_the_bit(gpu_ctx):
    """Scale(1/255) on uint8-valued floats equals scaling the input first; both vector-load and dword forms of the forward kernel"""
    for W, k, s in ((16, 4, 4), (9, 3, 2)):
        sp = CR.spec(W, W, 2, [CR.layer((k, k), 2, 5, "tanh", s)], scale=1.0 / 255.0); sp1 = dict(sp, scale=1.0); rng = np.random.default_rng(5)
        p = CR.perturbed(CR.glorot_params(sp, rng), rng); x = np.asfortranarray(rng.integers(0, 256, (W * W * 2, 6)).astype(np.float32))
        dy = np.asfortranarray(rng.normal(0, 1, (CR.n_features(sp), 6)).astype(np.float32))
        ya, _, ga = _Run(gpu_ctx, sp, p)(x, dy); yb, _, gb = _Run(gpu_ctx, sp1, p)(np.asfortranarray((x * np.float32(sp["scale"])).astype(np.float32)), dy)
        assert np.array_equal(ya, yb) and np.array_equal(ga, gb)


def test_reproducible_bits_workspace_reuse_and_flags(gpu_ctx):
    sp = CR.TWO_LAYER; rng = np.random.default_rng(6); p = CR.perturbed(CR.glorot_params(sp, rng), rng)
    xs = {B: (np.asfortranarray(rng.normal(0, 1, (512, B)).astype(np.float32)), np.asfortranarray(rng.normal(0, 1, (CR.n_features(sp), B)).astype(np.float32))) for B in (37, 129)}
    one = _Run(gpu_ctx, sp, p)
    first = one(*xs[37]); again = one(*xs[37])                       # two runs: identical bits
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    big = one(*xs[129]); small = one(*xs[37])                         # the workspace grew once (32 -> 64 -> 256 columns) and is re-used at the smaller B
    for B, got in ((37, small), (129, big)):
        fresh = _Run(gpu_ctx, sp, p)(*xs[B])
        for name, a, b in zip(("y", "dx", "gradient"), got, fresh):
            assert np.array_equal(a, b), (B, name)
    y0, dx0, g0 = first
    y1, dx1, g1 = one(*xs[37], want_g=1, want_dx=False)               # flags select outputs without changing them
    assert dx1 is None and np.array_equal(y1, y0) and np.array_equal(g1, g0)
    ctx = gpu_ctx; ctx.check(ctx.lib.crux_mlp_set_params(one.t.p.h, p.ctypes.data_as(C.c_void_p), p.size))
    before = np.empty(p.size, np.float32); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(one.t.p.h), before)
    y2, dx2, g2 = one(*xs[37], want_g=0, want_dx=True)
    assert np.array_equal(y2, y0) and np.array_equal(dx2, dx0) and np.array_equal(g2, before)      # want_param_grads = 0 leaves the gradient vector as it was
    y3, _, _ = one(*xs[37], cached=False)
    assert np.array_equal(y3, y0)


# ---- crux_conv_dqn_target and one crux_conv_td_step on a staged batch of 32 -----------------------------------------------------------------------------------------------
STEP_SPEC = CR.spec(10, 10, 2, [CR.layer((3, 3), 2, 6, "relu", 1)])      # 10x10x2 -> 6@(3,3)/1 relu -> flatten -> 384-32-3
STEP_DIMS, STEP_ACTS, ETA = [384, 32, 3], ["relu", "identity"], float(np.float32(1e-3))


def _step_policy(ctx, seed):
    ch = crux.Chain(crux.Conv((3, 3), 2, 6, "relu"), crux.flatten, crux.Dense(384, 32, "relu"), crux.Dense(32, 3), input=(10, 10, 2))
    return crux.DiscreteNetwork(ch, [1, 2, 3], seed=seed, ctx=ctx)


@pytest.mark.parametrize("use_weight", [0, 1])
def test_dqn_target_and_td_step_match_float64(gpu_ctx, use_weight):
    ctx, B, gamma = gpu_ctx, 32, np.float32(0.95); rng = np.random.default_rng(11 + use_weight)
    pi, pim = _step_policy(ctx, 3), _step_policy(ctx, 4)
    nt = pi.trunk.p.n_params
    for q in (pi, pim):
        q.set_params(CR.perturbed(q.get_params(), rng))
    pt, ph = pi.get_params()[:nt], pi.get_params()[nt:]; ptm, phm = pim.get_params()[:nt], pim.get_params()[nt:]
    s = CR.kink_free_images(pt, STEP_SPEC, B, rng, head=(ph, STEP_DIMS, STEP_ACTS))
    d = {"s": s, "sp": np.asfortranarray(rng.normal(0, 1, (200, B)).astype(np.float32)), "r": rng.normal(0, 1, (1, B)).astype(np.float32),
         "a": np.asfortranarray(np.eye(3, dtype=bool)[:, rng.integers(0, 3, B)]), "done": rng.random((1, B)) < 0.3, "episode_end": np.zeros((1, B), bool),
         "weight": rng.uniform(0.2, 1.5, (1, B)).astype(np.float32)}
    buf = crux.ExperienceBuffer(crux.ContinuousSpace((10, 10, 2)), crux.DiscreteSpace(3), B, ["weight"], ctx=ctx); buf.push_(d)
    d_y, d_err = ctx.alloc(4 * B), ctx.alloc(4 * B)
    try:
        ctx.check(ctx.lib.crux_conv_dqn_target(pim.trunk.h, pim.trunk.p.h, pim.head_h, buf.h, float(gamma), d_y))
        y = ctx.d2h(d_y, np.empty(B, np.float32))
        y64, y32 = (CR.dqn_target_reference(STEP_SPEC, ptm, STEP_DIMS, STEP_ACTS, phm, d["sp"], d["r"], d["done"], gamma, t) for t in (np.float64, np.float32))
        _bound_check("target", [("y", y, y64, y32)])
        pi.attach_optimizer(crux.Adam(np.float32(ETA)))
        w = d["weight"] if use_weight else None
        r64, r32 = (CR.td_reference(STEP_SPEC, pt, STEP_DIMS, STEP_ACTS, ph, s, d["a"], y, w, t) for t in (np.float64, np.float32))
        raw = np.zeros(L.INFO_N, np.float32)
        if use_weight:      # the prioritized-buffer twin: the same step, and td_error of the same forward pass
            ctx.check(ctx.lib.crux_conv_td_step_with_error(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_y, 1, d_err, raw.ctypes.data_as(C.c_void_p)))
            err = ctx.d2h(d_err, np.empty(B, np.float32))
        else:
            ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_y, 0, raw.ctypes.data_as(C.c_void_p)))
        gt, gh = np.empty(nt, np.float32), np.empty(ph.size, np.float32)
        ctx.d2h(ctx.lib.crux_mlp_grads_ptr(pi.trunk.p.h), gt); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(pi.head_h), gh)
    finally:
        ctx.free(d_y); ctx.free(d_err)
    # gradients of both handles under the M bound, per tensor
    tensors = [(n, t, r64["g_trunk"][a:b], r32["g_trunk"][a:b]) for n, t, (a, b) in _flat_slices("trunk", gt, CR.layer_offsets(STEP_SPEC), [ly["cout"] for ly in STEP_SPEC["layers"]])]
    tensors += [(n, t, r64["g_head"][a:b], r32["g_head"][a:b]) for n, t, (a, b) in _flat_slices("head", gh, R.layer_offsets(STEP_DIMS), STEP_DIMS[1:])]
    _bound_check("step w%d" % use_weight, tensors)
    # loss, Qavg, grad_norm: what the bound on Q and on the gradient tensors allows. |dQ| <= bQ = M max(e32(Q), u) max|Q|; the loss mean((Q - y)^2 w) then moves by at most
    # mean(2 |Q - y| w) bQ (+ bQ^2), Qavg by bQ, the norm by the norm of the tensors' bounds; each + 2 u of its value for its own Float32 roundings
    bQ = M * max(R.rel_err(r32["Q"], r64["Q"]), U) * np.abs(r64["Q"]).max()
    bn = np.sqrt(sum(t.size * (M * max(R.rel_err(t32, t64), U) * np.abs(t64).max()) ** 2 for _, t, t64, t32 in tensors))
    print("STEP w%d loss %.9g ref %.9g bound %.3g | Qavg %.9g ref %.9g bound %.3g | grad_norm %.9g ref %.9g bound %.3g" % (
        use_weight, raw[0], r64["loss"], r64["dabs_w"] * bQ + bQ * bQ, raw[2], r64["qavg"], bQ, raw[1], r64["grad_norm"], bn))
    assert abs(raw[0] - r64["loss"]) <= r64["dabs_w"] * bQ + bQ * bQ + 4 * U * abs(r64["loss"])      # (4 u: each term (Q - y)^2 w is two Float32 products, then the cast)
    assert abs(raw[2] - r64["qavg"]) <= bQ + 2 * U * abs(r64["qavg"])
    assert abs(raw[1] - r64["grad_norm"]) <= bn + 2 * U * r64["grad_norm"]
    if use_weight:
        assert np.abs(err - np.abs(r64["Q"] - y)).max() <= bQ + 2 * U * np.abs(r64["Q"] - y).max()
    # parameters after Flux Adam's first step, every element: the update the device's own gradient defines, in Float64, within adam_small eta; |update| <= eta (1 + small);
    # its sign never that of +g, and no element stays put whose update exceeds half its spacing (conv_reference.adam_sign_ok)
    for name, p0, p1, g in (("trunk", pt, pi.get_params()[:nt], gt), ("head", ph, pi.get_params()[nt:], gh)):
        small = CR.adam_small(p0, ETA); dlt = p1.astype(np.float64) - p0
        print("ADAM %s max |dlt - dlt64| / eta %.3g (allowed %.3g)  max |dlt| / eta %.9g" % (name, np.abs(dlt - CR.adam_first_step_delta(g, ETA)).max() / ETA, small.max(), np.abs(dlt).max() / ETA))
        assert np.all(np.abs(dlt - CR.adam_first_step_delta(g, ETA)) <= small * ETA), name
        assert np.all(np.abs(dlt) <= ETA * (1 + small)) and CR.adam_sign_ok(p0, p1, g, ETA), name
    assert np.array_equal(pim.get_params(), np.concatenate([ptm, phm]))      # the target network is read only


def _flat_slices(tag, g, offs, outs):
    out = []
    for l, ((wo, bo), o) in enumerate(zip(offs, outs)):
        out += [("%s dW%d" % (tag, l), g[wo:bo], (wo, bo)), ("%s db%d" % (tag, l), g[bo:bo + o], (bo, bo + o))]
    return out


# ---- host mirror ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_mirror_value_params_clone_polyak(gpu_ctx):
    ctx = gpu_ctx; rng = np.random.default_rng(21); pi = _step_policy(ctx, 5)
    assert pi.is_conv == "conv" and pi.network.dims == STEP_DIMS
    nt = pi.trunk.p.n_params; assert nt == 3 * 3 * 2 * 6 + 6 and pi.n_params == nt + R.n_layer_params(STEP_DIMS)
    assert [a.shape for a in pi.params()] == [(3, 3, 2, 6), (6,), (32, 384), (32,), (3, 32), (3,)]      # Flux.params order, conv weights 4-D
    lim = np.sqrt(6.0 / (9 * 2 + 9 * 6)); w0 = pi.params()[0]
    assert np.abs(w0).max() <= lim and np.abs(w0).max() > 0.5 * lim and not np.any(pi.params()[1])          # glorot_uniform for Conv, zero bias
    p = CR.perturbed(pi.get_params(), rng); pi.set_params(p)
    assert np.array_equal(pi.get_params(), p) and np.array_equal(np.concatenate([a.reshape(-1, order="F") for a in pi.params()]), p)
    s = np.asfortranarray(rng.normal(0, 1, (200, 9)).astype(np.float32))
    q = crux.value(pi, s)
    q64, q32 = (CR.q_reference(STEP_SPEC, p[:nt], STEP_DIMS, STEP_ACTS, p[nt:], s, t) for t in (np.float64, np.float32))
    _bound_check("value", [("Q", q, q64, q32)])
    pim = crux.clone_policy(pi)
    assert pim.is_conv and np.array_equal(pim.get_params(), p)
    p2 = CR.perturbed(p, rng); pi.set_params(p2)
    crux.polyak_average_(pim, pi, 0.5)
    # crux_polyak on an MLP handle over the same values: the bits both handles of the conv policy must have
    ma, mb = crux.ParamVector(p, ctx=ctx), crux.ParamVector(p2, ctx=ctx); ctx.check(ctx.lib.crux_polyak(ma.h, mb.h, 0.5))
    assert np.array_equal(pim.get_params(), ma.get_params()) and np.array_equal(pi.get_params(), p2)
    pi.attach_optimizer(crux.Adam(np.float32(1e-3))); m, v, bp = pi.adam_state()
    assert m.size == pi.n_params and not m.any() and not v.any()


def test_glorot_draws_follow_the_header_convention(gpu_ctx):
    """weight n of the trunk, counted through the layers' weight arrays (biases not counted), is (u - 0.5) * sqrt(24 / (k1 k2 (cin + cout))) with u = crux_u32_to_f32 of word 0
    of philox(seed, counter = n, stream + TRUNK_STREAM, CRUX_RNG_INIT = 7); biases are zero. Bit for bit, through the oracle's Philox."""
    import oracle as O
    from crux_jl_amd.conv import TRUNK_STREAM
    sp = CR.TWO_LAYER; seed, stream = 9, 3
    got = crux.ConvTrunk(host_spec(sp), ctx=gpu_ctx, seed=seed, stream=stream).p.get_params()
    want, n = np.zeros_like(got), 0
    for ly, (wo, bo) in zip(sp["layers"], CR.layer_offsets(sp)):
        scale = np.sqrt(np.float32(24.0) / np.float32(ly["k"][0] * ly["k"][1] * (ly["cin"] + ly["cout"])))
        for e in range(wo, bo):
            v = np.zeros(4, np.uint32); O.lib().orc_philox(seed, n, stream + TRUNK_STREAM, 7, O.vpz(v)); n += 1
            want[e] = (np.float32(int(v[0]) >> 8) * np.float32(5.9604644775390625e-08) - np.float32(0.5)) * scale
    assert want.dtype == np.float32 and np.array_equal(got, want)


def test_explore_on_the_host_seam_draws_like_an_mlp_with_these_outputs(gpu_ctx):
    """action(pi, s) is the argmax of value(pi, s); and with epsilon = 1 every action is the exploration kernel's random draw, which does not look at the network: it must be the
    draw an MLP with as many outputs gets for the same seed, interaction index and step counters"""
    ctx = gpu_ctx; rng = np.random.default_rng(31); pi = _step_policy(ctx, 6); E = 7
    mlp = crux.DiscreteNetwork(parity.chain([4, 3], ["identity"]), [1, 2, 3], seed=1, ctx=ctx)
    s = np.asfortranarray(rng.normal(0, 1, (200, E)).astype(np.float32)); st = np.arange(E, dtype=np.int64) * 3
    cfg = parity.rollout_cfg(explore=False, reset=False, head="greedy_q", i0=5)
    a, _ = crux.policy_explore(pi, cfg, s, 11, st)
    assert a.shape == (3, E) and np.array_equal(np.argmax(a, axis=0), np.argmax(crux.value(pi, s), axis=0)) and np.all(a.sum(axis=0) == 1)
    cfg = parity.rollout_cfg(explore=True, reset=False, head="greedy_q", i0=5); cfg.eps_start = cfg.eps_stop = 1.0; cfg.eps_steps = 1
    a1, _ = crux.policy_explore(pi, cfg, s, 11, st); a2, _ = crux.policy_explore(mlp, cfg, np.asfortranarray(rng.normal(0, 1, (4, E)).astype(np.float32)), 11, st)
    assert np.array_equal(a1, a2) and len(set(np.argmax(a1, axis=0))) > 1


def test_dqn_solve_runs_the_call_by_call_loop_on_pixels(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import dqn_pixels as ex
    env = ex.Catch(6, 6, seed=1); pi = ex.q_network(6, 6, seed=2, hidden=16, ctx=gpu_ctx)
    # buffer_init = 16 interactions come first (solve counts them: off_policy.jl:122-125), then the iterations at i = 16, 20, 24 <= N - dN
    solver = crux.DQN(pi, crux.ContinuousSpace((6, 6, 2)), N=28, dN=4, c_opt={"batch_size": 16, "optimizer": crux.Adam(np.float32(1e-3))}, buffer_size=64, buffer_init=16, max_steps=6)
    before = pi.get_params(); nt = pi.trunk.p.n_params
    crux.solve(solver, env.mdp())
    after, minus = pi.get_params(), solver.agent.pi_minus.get_params()
    assert len(solver.history) == 3 and not solver._pending and all(np.isfinite(h["critic_loss"]) and np.isfinite(h["critic_grad_norm"]) for h in solver.history)
    assert np.any(after[:nt] != before[:nt]) and np.any(after[nt:] != before[nt:])                       # both handles were trained
    assert np.any(minus[:nt] != after[:nt]) and np.any(minus[nt:] != after[nt:])                         # pi_minus follows by polyak(tau), it is not pi
    assert np.any(minus[:nt] != before[:nt]) and np.any(minus[nt:] != before[nt:])                       # ... and the target update reached both of its handles
    assert len(solver.buffer) == 16 + 12


# ---- refusals: by name, before any device call ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_themselves_and_touch_nothing(gpu_ctx):
    ctx = gpu_ctx; pi = _step_policy(ctx, 8); S = crux.ContinuousSpace((10, 10, 2)); before = pi.get_params()
    mlp = lambda dims: crux.ContinuousNetwork(parity.chain(dims, ["relu", "identity"]), ctx=ctx)      # noqa: E731
    gauss = crux.GaussianPolicy(parity.chain([200, 8, 1], ["relu", "identity"]), np.zeros(1, np.float32), ctx=ctx)
    conv_v = crux.ContinuousNetwork(crux.Chain(crux.Conv((3, 3), 2, 6, "relu"), crux.flatten, crux.Dense(384, 1), input=(10, 10, 2)), ctx=ctx)
    cases = [("PPO", lambda: crux.PPO(crux.ActorCritic(pi, mlp([200, 8, 1])), S)),
             ("PPO", lambda: crux.PPO(crux.ActorCritic(gauss, conv_v), S)),
             ("SAC", lambda: crux.SAC(crux.ActorCritic(gauss, crux.DoubleNetwork(conv_v, mlp([201, 8, 1]))), S, N=10)),
             ("SoftQ", lambda: crux.SoftQ(pi, S, N=10)),
             ("Sampler", lambda: crux.Sampler(crux.CartPoleMDP(), pi)),
             ("train!", lambda: crux.train_(pi, crux.TrainingParams(loss=crux.value_mse_loss, optimizer=crux.Adam(np.float32(1e-3))), {}, None, [1])),
             # network-valued arguments that never pass through PolicyParams; `same` is a 'same' conv whose flatten is as wide as the observation: the silent case
             ("fill_gae!", lambda: crux.fill_gae_(None, same, 0.95, 0.99)),
             ("fill_gae!", lambda: crux.fill_gae_(None, crux.ActorCritic(gauss, conv_v), 0.95, 0.99)),
             ("batch_train_gail_d_", lambda: crux.batch_train_gail_d_(same, crux.TrainingParams(loss=crux.gail_d_loss, optimizer=crux.Adam(np.float32(1e-3))), None, None)),
             ("batch_train_gail_d_chain_", lambda: crux.imitation.batch_train_gail_d_chain_(same, None, None, None)),
             ("gail_reward_", lambda: crux.gail_reward_(same, None)),
             ("OnPolicyGAIL (D)", lambda: crux.OnPolicyGAIL(crux.ActorCritic(gauss, mlp([200, 8, 1])), S, 0.99, same, None)),
             ("DiagonalFisherRegularizer", lambda: crux.DiagonalFisherRegularizer(same)),
             ("MixtureNetwork", lambda: crux.MixtureNetwork([gauss, gauss], same, ctx=ctx)),
             ("OrthogonalRegularizer", lambda: crux.orthogonal_regularizer(same))]
    same = crux.ContinuousNetwork(crux.Chain(crux.Conv((3, 3), 2, 2, "relu", pad=1), crux.flatten, crux.Dense(200, 1), input=(10, 10, 2)), ctx=ctx)
    with pytest.raises(NotImplementedError) as eh:      # and behind the named refusals: a conv policy has no whole-network handle for any other path to read
        same.h
    assert "convolutional trunk" in str(eh.value) and same.head_h and pi.head_h
    for who, call in cases:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert who in str(e.value) and "convolutional trunk" in str(e.value), (who, str(e.value))
    assert not getattr(pi, "always_stochastic", False) and pi.optimizer is None and np.array_equal(pi.get_params(), before)      # SoftQ and train! changed nothing
    for kw, word in (({"dilation": 2}, "dilation"), ({"groups": 2}, "groups")):
        with pytest.raises(NotImplementedError) as e:
            crux.Conv((3, 3), 2, 6, **kw)
        assert word in str(e.value)
        ly = (L.ConvLayer * 1)(); a = ly[0]                                                   # and the C ABI itself: CRUX_EUNSUP, the message names the field
        a.k1, a.k2, a.cin, a.cout, a.stride1, a.stride2, a.pad1, a.pad2, a.act, a.dilation1, a.dilation2, a.groups = 3, 3, 2, 6, 1, 1, 0, 0, 0, kw.get("dilation", 1), 1, kw.get("groups", 1)
        h = C.c_void_p(); rc = ctx.lib.crux_conv_create(ctx.h, 10, 10, 2, 1.0, 1, ly, C.byref(h))
        assert rc == L.EUNSUP and h.value is None
        with pytest.raises(crux.CruxError) as e2:
            ctx.check(rc)
        assert word in str(e2.value)
    assert np.array_equal(pi.get_params(), before)
