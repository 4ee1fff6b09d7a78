"""Optimiser(ClipValue(c), Adam) on the device (csrc/sac.hip AdamClipGatedOp, crux_adam_set_clip_value) through the three steps that take it:
  dense   a DiscreteNetwork 8-128-128-4 through crux_td_step (the dense engine's route)
  conv    the trunk + head pair of tests/test_gpu_conv.py's step (10x10x2 -> Conv 3x3, 6 -> 384-32-3) through crux_conv_td_step
  wide    a trunk with a wide head (12x12x2 -> Conv 3x3, 13 -> 1300-40-3: crux_mlp_create_wide) through crux_conv_td_step
each on a staged batch of 32. c is the median of |g| of the float64 reference gradient, so about half of all elements are clamped (asserted on the CPU side: 40-60 %, and every
handle has clamped and unclamped elements).

What is asserted: the raw quantities (gradient buffers, loss, Qavg, grad_norm) are bit-identical to the same step on a twin without the clamp; after the first step m and v are
bit-equal to the kernel's Float64 expressions of the device's own gradient after clip_value (optimiser_reference.first_step_mv_f32) -- the first PARAMETER step alone cannot show
a clamp, m / sqrt(v) normalises it away; over three teacher-forced steps the moments are within one Float32 ulp of the float64 step from the device's previous state and the
parameters within conv_reference.adam_small; |m| <= (1 - b1^t) c and v <= (1 - b2^t) c^2 everywhere while the twin violates both; c = 0 restores AdamGatedOp's bits; the setter
refuses NaN, Inf and negatives; a clamped handle is CRUX_EUNSUP with nothing changed in crux_dqn_epochs, crux_adam_apply and a narrow crux_td_step. Host: DQN.solve on pixels with
a wide head and the chain optimiser, a dense-critic DQN with PER taking the call-by-call loop, and the named refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conv_reference as CR
import dense_reference as R
import optimiser_reference as OR
import parity
from parity import crux
from crux_jl_amd import _lib as L

pytestmark = pytest.mark.gpu
B, ETA = 32, float(np.float32(1e-3))
DENSE_DIMS, DENSE_ACTS = [8, 128, 128, 4], ["relu", "relu", "identity"]
CONV = {"conv": dict(W=10, cout=6, dims=[384, 32, 3]), "wide": dict(W=12, cout=13, dims=[1300, 40, 3])}
HEAD_ACTS = ["relu", "identity"]


def _policy(ctx, kind, seed):
    if kind == "dense":
        return crux.DiscreteNetwork(parity.chain(DENSE_DIMS, DENSE_ACTS), [1, 2, 3, 4], seed=seed, ctx=ctx)
    k = CONV[kind]; d = k["dims"]
    ch = crux.Chain(crux.Conv((3, 3), 2, k["cout"], "relu"), crux.flatten, crux.Dense(d[0], d[1], "relu"), crux.Dense(d[1], d[2]), input=(k["W"], k["W"], 2))
    return crux.DiscreteNetwork(ch, [1, 2, 3], seed=seed, ctx=ctx)


def _handles(pi):
    return [pi.trunk.p.h, pi.head_h] if pi.is_conv else [pi.h]


def _grads(ctx, pi):
    return np.concatenate([ctx.d2h(ctx.lib.crux_mlp_grads_ptr(h), np.empty(int(ctx.lib.crux_mlp_n_params(h)), np.float32)) for h in _handles(pi)])


def _step(ctx, pi, buf, d_y):
    raw = np.zeros(L.INFO_N, np.float32)
    if pi.is_conv:
        ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_y, 0, raw.ctypes.data_as(C.c_void_p)))
    else:
        ctx.check(ctx.lib.crux_td_step(pi.h, buf.h, d_y, 0, raw.ctypes.data_as(C.c_void_p)))
    return raw


def _reference_gradient(kind, p, s, a, y):
    """the float64 gradient of mean((Q(s, a) - y)^2) over all of Flux.params(pi): only c is taken from it"""
    if kind == "dense":
        z = R.chain_reference(p, DENSE_DIMS, DENSE_ACTS, s, np.zeros((4, B)), np.float64)["y"]
        d = (z * a).sum(axis=0) - y.astype(np.float64)
        return R.flat_gradient(R.chain_reference(p, DENSE_DIMS, DENSE_ACTS, s, a * (2.0 * d / B)[None, :], np.float64), DENSE_DIMS)
    k = CONV[kind]; sp = CR.spec(k["W"], k["W"], 2, [CR.layer((3, 3), 2, k["cout"], "relu", 1)]); nt = CR.n_params(sp)
    r = CR.td_reference(sp, p[:nt], k["dims"], HEAD_ACTS, p[nt:], s, a, y, None, np.float64)
    return np.concatenate([r["g_trunk"], r["g_head"]])


@pytest.fixture(scope="module", params=["dense", "conv", "wide"])
def case(request, gpu_ctx):
    """one staged batch, the clamped policy, its twin without the clamp, the reference's c"""
    kind, ctx = request.param, gpu_ctx; rng = np.random.default_rng({"dense": 41, "conv": 42, "wide": 43}[kind])
    pi, twin = _policy(ctx, kind, 3), _policy(ctx, kind, 3)
    p = CR.perturbed(pi.get_params(), rng); pi.set_params(p); twin.set_params(p)
    od = 8 if kind == "dense" else CONV[kind]["W"] ** 2 * 2; na = 4 if kind == "dense" else 3
    s = np.asfortranarray(rng.normal(0, 1, (od, B)).astype(np.float32)); a = np.asfortranarray(np.eye(na, dtype=bool)[:, rng.integers(0, na, B)])
    d = {"s": s, "sp": np.asfortranarray(rng.normal(0, 1, (od, B)).astype(np.float32)), "r": rng.normal(0, 1, (1, B)).astype(np.float32), "a": a,
         "done": rng.random((1, B)) < 0.3, "episode_end": np.zeros((1, B), bool)}
    S = crux.ContinuousSpace(8) if kind == "dense" else crux.ContinuousSpace((CONV[kind]["W"], CONV[kind]["W"], 2))
    buf = crux.ExperienceBuffer(S, crux.DiscreteSpace(na), B, [], ctx=ctx); buf.push_(d)
    y = rng.normal(0, 1, B).astype(np.float32); d_y = ctx.alloc(4 * B); ctx.h2d(d_y, y)
    g64 = _reference_gradient(kind, p, s, a.astype(np.float64), y)
    c = float(np.float32(np.median(np.abs(g64))))
    yield dict(kind=kind, ctx=ctx, pi=pi, twin=twin, p=p, buf=buf, d_y=d_y, g64=g64, c=c, sizes=pi._sizes())
    ctx.free(d_y)


def test_c_clamps_about_half_of_every_handle(case):
    g, c = np.abs(case["g64"]), case["c"]
    assert c > 0 and 0.4 <= np.mean(g > c) <= 0.6, (c, float(np.mean(g > c)))
    off = 0
    for n in case["sizes"]:
        part = g[off:off + n]; off += n
        assert np.any(part > c) and np.any(part <= c), n


def test_three_steps_clamp_in_registers_and_leave_the_raw_quantities_alone(case):
    ctx, pi, twin, c, buf, d_y = case["ctx"], case["pi"], case["twin"], case["c"], case["buf"], case["d_y"]
    pi.set_params(case["p"]); twin.set_params(case["p"])
    pi.attach_optimizer(crux.Optimiser(crux.ClipValue(c), crux.Adam(np.float32(ETA)))); twin.attach_optimizer(crux.Adam(np.float32(ETA)))
    for h in _handles(pi):
        assert ctx.lib.crux_adam_get_clip_value(h) == np.float32(c)
    for h in _handles(twin):
        assert ctx.lib.crux_adam_get_clip_value(h) == 0.0
    for t in (1, 2, 3):
        p0 = pi.get_params(); m0, v0, bp0 = pi.adam_state()
        raw = _step(ctx, pi, buf, d_y); g = _grads(ctx, pi)
        p1 = pi.get_params(); m1, v1, bp1 = pi.adam_state()
        assert np.all(np.isfinite(raw[:3])) and np.allclose(bp1, [0.9 ** (t + 1), 0.999 ** (t + 1)], rtol=1e-14)
        if t == 1:
            # raw quantities: the twin without the clamp took the same step from the same parameters
            raw_t = _step(ctx, twin, buf, d_y); g_t = _grads(ctx, twin)
            assert np.array_equal(g, g_t) and np.array_equal(raw, raw_t)
            assert 0.3 <= np.mean(np.abs(g) > np.float32(c)) <= 0.7                      # the device's own gradient is clamped about as often as the reference's
            assert abs(raw[1] - np.sqrt((g.astype(np.float64) ** 2).sum())) <= 4 * R.U32 * raw[1]      # grad_norm is the RAW gradient's
            # first-step moments: bit for bit the kernel's Float64 expressions of clip_value(g): this is what fails without the clamp
            m_want, v_want = OR.first_step_mv_f32(g, np.float32(c))
            assert np.array_equal(m1, m_want) and np.array_equal(v1, v_want)
            mt, vt, _ = twin.adam_state(); m_raw, v_raw = OR.first_step_mv_f32(g, 0)
            assert np.array_equal(mt, m_raw) and np.array_equal(vt, v_raw) and not np.array_equal(mt, m1)
            bm, bv = OR.moment_bounds(1, c)
            assert np.abs(mt).max() > bm and vt.max() > bv                               # the unclamped twin violates the bounds
        # teacher-forced: the float64 step from the device's previous state and its own raw gradient
        d64, m64, v64 = OR.teacher_forced_f64(p0, m0, v0, g, t, np.float32(c), ETA)
        assert np.all(np.abs(m1 - m64) <= OR.ulp32(m64)), (t, "m")
        assert np.all(np.abs(v1 - v64) <= OR.ulp32(v64)), (t, "v")
        dlt = p1.astype(np.float64) - p0
        print("CLIP %s step %d max |dlt - dlt64| / eta %.3g  max |m| / c %.6f" % (case["kind"], t, np.abs(dlt - d64).max() / ETA, np.abs(m1).max() / c))
        assert np.all(np.abs(dlt - d64) <= CR.adam_small(p0, ETA) * ETA), t
        bm, bv = OR.moment_bounds(t, c)
        assert np.abs(m1).max() <= bm and v1.max() <= bv, t
        assert np.array_equal(_grads(ctx, pi), g)                                        # the gradient buffer keeps the raw gradient after the step


def test_setter_zero_restores_plain_adam_and_refuses_bad_values(case):
    ctx, c, buf, d_y = case["ctx"], case["c"], case["buf"], case["d_y"]
    a, b = _policy(ctx, case["kind"], 3), _policy(ctx, case["kind"], 3)
    a.set_params(case["p"]); b.set_params(case["p"])
    a.attach_optimizer(crux.Optimiser(crux.ClipValue(c), crux.Adam(np.float32(ETA)))); a.attach_optimizer(crux.Adam(np.float32(ETA)))      # a plain Adam afterwards clears it
    b.attach_optimizer(crux.Adam(np.float32(ETA)))
    for h in _handles(a):
        assert ctx.lib.crux_adam_get_clip_value(h) == 0.0
        ctx.check(ctx.lib.crux_adam_set_clip_value(h, c)); ctx.check(ctx.lib.crux_adam_set_clip_value(h, 0.0))
        for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
            rc = ctx.lib.crux_adam_set_clip_value(h, bad)
            assert rc == L.EINVAL and "crux_adam_set_clip_value" in ctx.lib.crux_last_error(ctx.h).decode() and ctx.lib.crux_adam_get_clip_value(h) == 0.0
    ra, rb = _step(ctx, a, buf, d_y), _step(ctx, b, buf, d_y)
    assert np.array_equal(ra, rb) and np.array_equal(a.get_params(), b.get_params())
    for x, y in zip(a.adam_state(), b.adam_state()):
        assert np.array_equal(x, y)


def test_other_adam_sites_refuse_a_clamped_handle(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib; rng = np.random.default_rng(5)
    wide_enough = crux.DiscreteNetwork(parity.chain(DENSE_DIMS, DENSE_ACTS), [1, 2, 3, 4], seed=1, ctx=ctx)
    narrow = crux.DiscreteNetwork(parity.chain([8, 16, 4], ["relu", "identity"]), [1, 2, 3, 4], seed=2, ctx=ctx)
    target = crux.clone_policy(wide_enough)
    d = {"s": np.asfortranarray(rng.normal(0, 1, (8, B)).astype(np.float32)), "sp": np.asfortranarray(rng.normal(0, 1, (8, B)).astype(np.float32)),
         "r": rng.normal(0, 1, (1, B)).astype(np.float32), "a": np.asfortranarray(np.eye(4, dtype=bool)[:, rng.integers(0, 4, B)]), "done": np.zeros((1, B), bool), "episode_end": np.zeros((1, B), bool)}
    src = crux.ExperienceBuffer(crux.ContinuousSpace(8), crux.DiscreteSpace(4), 64, [], ctx=ctx); src.push_(d)
    batch = crux.ExperienceBuffer(crux.ContinuousSpace(8), crux.DiscreteSpace(4), B, [], ctx=ctx); batch.push_(d)
    chain = crux.Optimiser(crux.ClipValue(0.5), crux.Adam(np.float32(ETA)))
    wide_enough.attach_optimizer(chain); narrow.attach_optimizer(chain)
    d_y = ctx.alloc(4 * B); ctx.h2d(d_y, np.zeros(B, np.float32)); infos = np.zeros((2, L.INFO_N), np.float32); raw = np.zeros(L.INFO_N, np.float32)
    try:
        for net, name, call in ((wide_enough, "crux_dqn_epochs", lambda: lib.crux_dqn_epochs(wide_enough.h, target.h, src.h, batch.h, 0.99, 0, 0.0, 0, 2, infos.ctypes.data_as(C.c_void_p))),
                                (wide_enough, "crux_adam_apply", lambda: lib.crux_adam_apply(wide_enough.h, 1.0)),
                                (narrow, "crux_td_step", lambda: lib.crux_td_step(narrow.h, batch.h, d_y, 0, raw.ctypes.data_as(C.c_void_p)))):
            before = (net.get_params(), _grads(ctx, net)) + net.adam_state() + (batch["s"],)
            rc = call(); msg = lib.crux_last_error(ctx.h).decode()
            assert rc == L.EUNSUP and name in msg and "ClipValue" in msg, (name, rc, msg)
            ctx.sync()
            for x, y in zip(before, (net.get_params(), _grads(ctx, net)) + net.adam_state() + (batch["s"],)):
                assert np.array_equal(x, y), name
    finally:
        ctx.free(d_y)


# ---- host mirror ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_dqn_solve_on_pixels_with_a_wide_head_and_the_chain_optimiser(gpu_ctx):
    sys.path.insert(0, os.path.join(parity.ROOT, "examples"))
    import dqn_pixels as ex
    ctx = gpu_ctx; env = ex.Catch(12, 12, seed=1); c = 1e-4
    ch = crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((3, 3), 2, 13, "relu"), crux.flatten, crux.Dense(1300, 40, "relu"), crux.Dense(40, 3), input=(12, 12, 2))
    pi = crux.DiscreteNetwork(ch, [0, 1, 2], seed=2, ctx=ctx)
    solver = crux.DQN(pi, crux.ContinuousSpace((12, 12, 2)), N=28, dN=4, c_opt={"batch_size": 16, "optimizer": crux.Optimiser(crux.ClipValue(c), crux.Adam(np.float32(1e-3)))},
                      buffer_size=64, buffer_init=16, max_steps=12)
    before = pi.get_params(); nt = pi.trunk.p.n_params
    crux.solve(solver, env.mdp())
    after, minus = pi.get_params(), solver.agent.pi_minus.get_params()
    assert len(solver.history) == 3 and not solver._pending and all(np.isfinite(h["critic_loss"]) and np.isfinite(h["critic_grad_norm"]) for h in solver.history)
    assert np.any(after[:nt] != before[:nt]) and np.any(after[nt:] != before[nt:]) and np.any(minus[nt:] != before[nt:])
    assert [ctx.lib.crux_adam_get_clip_value(h) for h in _handles(pi)] == [np.float32(c)] * 2 and all(ctx.lib.crux_adam_get_clip_value(h) == 0.0 for h in _handles(solver.agent.pi_minus))
    m, v, bp = pi.adam_state(); steps = 3 * 4
    bm, bv = OR.moment_bounds(steps, float(np.float32(c)))
    assert np.isclose(bp[0], 0.9 ** (steps + 1)) and 0 < np.abs(m).max() <= bm and v.max() <= bv      # 12 clamped steps on both handles
    assert crux.value(pi, env.observation(env.initialstate(0, 0))).shape == (3, 1)
    crux.polyak_average_(solver.agent.pi_minus, pi, 1.0); assert np.array_equal(solver.agent.pi_minus.get_params(), after)


def test_dense_critic_dqn_with_per_takes_the_call_by_call_loop(gpu_ctx, monkeypatch):
    ctx = gpu_ctx; c = 1e-4; calls = {"step": 0}
    q = crux.DiscreteNetwork(parity.chain(DENSE_DIMS, DENSE_ACTS), [1, 2, 3, 4], seed=3, ctx=ctx)
    mdp = crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=5, discount=0.97)
    sv = crux.DQN(q, crux.ContinuousSpace(8), N=44, dN=4, buffer_size=128, prioritized=True, weighted_loss=True, buffer_init=32, max_steps=40,
                  c_opt={"batch_size": 32, "optimizer": crux.Optimiser(crux.ClipValue(c), crux.Adam(np.float32(1e-3)))})

    def refuse(*a):
        raise AssertionError("a fused / asynchronous / one-launch entry was called for a solver with a chain optimiser")
    real = ctx.lib.crux_td_step_with_error

    def counted(*a):
        calls["step"] += 1
        return real(*a)
    for name in ("crux_dqn_epochs", "crux_dqn_value_training_async", "crux_dqn_small_solve", "crux_dqn_epoch"):
        monkeypatch.setattr(ctx.lib, name, refuse)
    monkeypatch.setattr(ctx.lib, "crux_td_step_with_error", counted)
    crux.solve(sv, mdp)
    assert len(sv.history) == 3 and calls["step"] == 3 * 4 and not sv._pending
    m, v, bp = q.adam_state(); bm, bv = OR.moment_bounds(12, float(np.float32(c)))
    assert 0 < np.abs(m).max() <= bm and v.max() <= bv and np.isclose(bp[0], 0.9 ** 13)
    pr = sv.buffer.priority_params()["priorities"]
    assert len(np.unique(pr[:len(sv.buffer)])) > 1      # update_priorities! ran


def test_host_refusals_name_the_caller_before_any_device_call(gpu_ctx):
    ctx = gpu_ctx; S = crux.ContinuousSpace(8); chain = crux.Optimiser(crux.ClipValue(1.0), crux.Adam(np.float32(1e-3)))
    mlp = lambda dims: crux.ContinuousNetwork(parity.chain(dims, ["relu", "identity"]), ctx=ctx)      # noqa: E731
    gauss = crux.GaussianPolicy(parity.chain([8, 16, 1], ["relu", "identity"]), np.zeros(1, np.float32), ctx=ctx)
    narrow = crux.DiscreteNetwork(parity.chain([8, 64, 4], ["relu", "identity"]), [1, 2, 3, 4], ctx=ctx)
    wide_enough = crux.DiscreteNetwork(parity.chain([8, 128, 4], ["relu", "identity"]), [1, 2, 3, 4], ctx=ctx)
    tp = crux.TrainingParams(loss=crux.value_mse_loss, optimizer=chain)
    before = narrow.get_params()
    cases = [("OnPolicySolver", lambda: crux.PPO(crux.ActorCritic(gauss, mlp([8, 16, 1])), S, a_opt={"optimizer": chain})),
             ("OnPolicySolver", lambda: crux.PPO(crux.ActorCritic(gauss, mlp([8, 16, 1])), S, c_opt={"optimizer": chain})),
             ("OffPolicySolver", lambda: crux.SAC(crux.ActorCritic(gauss, crux.DoubleNetwork(mlp([9, 16, 1]), mlp([9, 16, 1]))), S, N=10, c_opt={"optimizer": chain})),
             ("SoftQ", lambda: crux.SoftQ(wide_enough, S, N=10, c_opt={"optimizer": chain})),
             ("DQN over a network narrower than 128", lambda: crux.DQN(narrow, S, N=10, c_opt={"optimizer": chain})),
             ("BatchSolver", lambda: crux.BatchSolver(agent=None, S=S, D_train=None, a_opt=tp)),
             ("train!", lambda: crux.train_(narrow, tp, {}, None, [1])),
             ("train!", lambda: crux.batch_train_(narrow, tp, {}, None)),
             ("DeepEnsemble.attach_optimizer", lambda: crux.DeepEnsemble(lambda: parity.chain([2, 8, 2], ["relu", "identity"]), 2, ctx=ctx).attach_optimizer(chain))]
    for who, call in cases:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert who in str(e.value) and "ClipValue" in str(e.value), (who, str(e.value))
    assert narrow.optimizer is None and np.array_equal(narrow.get_params(), before) and not getattr(wide_enough, "always_stochastic", False)
    ok = crux.DQN(wide_enough, S, N=10, c_opt={"optimizer": chain})      # the admitted case constructs
    assert ok.c_opt.chain_ok and ok.c_opt.optimizer is chain
    with pytest.raises(crux.CruxError) as e:      # a plain MLP chain wider than 1024 keeps today's error
        crux.ContinuousNetwork(parity.chain([8, 1025, 1], ["relu", "identity"]), ctx=ctx)
    assert "1025" in str(e.value)
