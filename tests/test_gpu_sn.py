"""GPU: spectrally normalised discriminators (DenseSN, csrc/spectral.hip + the dense engine) against the float64 yardstick of tests/sn_reference.py.

Parameters, u and data of every case come from numpy (`case`, `step_reference`), so each case also runs through the yardstick alone.
Shapes: 3-12-1 (the reference's test shape: sub-wave, out = 1), 4-100-100-2 tanh (D_SN: no multiple of 16, 32 or 64), 3-64-64-2-1 with the last layer plain
(QSA_SN: mixed mask, four layers), 5-300-2 (more rows than one 256-thread workgroup), 4-256-256-2 (both fused dense routes eligible); n_iterations 1 and 3;
B 1, 37 and 256.
Tolerances (those of tests/test_gpu_advil.py, test_gpu_cql.py, test_gpu_iq.py): 1e-4 relative on losses, norms, sigma and outputs, 1e-4 of the gradient scale on
gradients, 2e-5 absolute on parameters after one Adam step at lr 1e-3. Parameters whose float64 gradient lies within 1e-3 of the gradient scale of zero are not
compared (the first Adam step is lr sign(g) there); at most a quarter may be left out per case. Largest share left out over the step cases, measured with the
yardstick alone (`skipped_shares()`): 19.8 % (crux_offgail_d_step, 4-256-256-2, n_iterations 3, Bd 37); the others lie between 0 and 14.8 %.
u is a unit vector: 1e-4 absolute. After the first forward call only sigma and the output are compared (u's direction is ill-conditioned when the top singular
values are close, sigma is not).
"""
import ctypes as C

import numpy as np
import pytest

import sn_reference as SR

pytestmark = pytest.mark.gpu

LR = 1e-3
SEED = 0x5EED5A3F
STEP_SKIPPED_MAX = 0.25      # the cap; every step test prints its own share

SHAPES = {
    "3-12-1": ((3, 12, 1), ("relu", "identity"), (1, 1)),
    "4-100-100-2": ((4, 100, 100, 2), ("tanh", "tanh", "identity"), (1, 1, 1)),
    "3-64-64-2-1": ((3, 64, 64, 2, 1), ("relu", "relu", "relu", "identity"), (1, 1, 1, 0)),
    "5-300-2": ((5, 300, 2), ("relu", "identity"), (1, 1)),
    "4-256-256-2": ((4, 256, 256, 2), ("relu", "relu", "identity"), (1, 1, 1)),
    "4-100-100-3": ((4, 100, 100, 3), ("tanh", "tanh", "identity"), (1, 1, 1)),      # D_SN with a class for one set of negative demonstrations (K = 3)
}
GRID = ["3-12-1", "4-100-100-2", "3-64-64-2-1", "5-300-2", "4-256-256-2"]
CASE_SEED = {"3-12-1": 1, "4-100-100-2": 2, "3-64-64-2-1": 3, "5-300-2": 4, "4-256-256-2": 5, "4-100-100-3": 6}


def case(name, n_iter=1, seed=None):
    """dims, acts, the SN mask scaled to n_iter, Glorot-uniform weights with small positive biases and one standard-normal u per SN layer: numpy alone"""
    dims, acts, mask = SHAPES[name]
    rng = np.random.default_rng(CASE_SEED[name] if seed is None else seed)
    p = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o)); p += [rng.uniform(-lim, lim, i * o), np.abs(rng.normal(0, 0.3, o))]
    sn = tuple(n_iter * m for m in mask)
    us = [rng.standard_normal(dims[l + 1]).astype(np.float32) for l in range(len(mask)) if mask[l]]
    return {"dims": dims, "acts": acts, "sn": sn, "p": np.concatenate(p).astype(np.float32), "us": us, "rng": rng}


def _crux():
    from parity import crux
    return crux


def _net(ctx, c, lr=LR):
    crux = _crux(); k = 0; layers = []
    for l, a in enumerate(c["acts"]):
        if c["sn"][l]:
            layers.append(crux.DenseSN(c["dims"][l], c["dims"][l + 1], a, n_iterations=c["sn"][l], u=c["us"][k])); k += 1
        else:
            layers.append(crux.Dense(c["dims"][l], c["dims"][l + 1], a))
    net = crux.ContinuousNetwork(crux.Chain(*layers), ctx=ctx)
    net.set_params(c["p"]); net.attach_optimizer(crux.Adam(np.float32(lr)))
    return net


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rel(a, b, tol=1e-4):
    return np.abs(np.asarray(a, np.float64) - b).max() <= tol * max(1.0, np.abs(b).max())


def _state_close(net, cache, with_u=True):
    for (u, v, s), ur, vr, sr in zip(net.spectral_state(), cache["us"], cache["vs"], cache["sigmas"]):
        assert abs(s - sr) <= 1e-4 * abs(sr), (s, sr)
        if with_u:
            assert np.abs(u - ur).max() <= 1e-4 and np.abs(v - vr).max() <= 1e-4


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


# ---- 1. single forward pass and pullback ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37, 256])
@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("name", GRID)
def test_forward_and_pullback_match_reference(gpu_ctx, name, n_iter, B):
    ctx, c = gpu_ctx, case(name, n_iter); dims = c["dims"]; rng = c["rng"]
    x = np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32)); dy = np.asfortranarray(rng.normal(0, 1, (dims[-1], B)).astype(np.float32))
    net, net2 = _net(ctx, c), _net(ctx, c)
    d_x, d_dy, d_y, d_dx = ctx.alloc(x.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(x.nbytes)
    try:
        ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
        us = c["us"]
        for gs in (1.0, 0.25):      # two forward calls: u advances between them, on the device and in the yardstick
            yr, cache = SR.forward(c["p"], dims, c["acts"], c["sn"], us, x)
            gr, dxr = SR.backward(cache, dy, gs)
            ctx.check(ctx.lib.crux_mlp_forward_cached(net.h, d_x, B, d_y))
            y = np.empty_like(dy); ctx.d2h(d_y, y)
            _state_close(net, cache, with_u=gs == 1.0)
            assert _rel(y, yr)
            yh = net2.forward(x)                                                  # crux_mlp_forward_host from the same starting u: the same pass
            assert np.array_equal(_bits(yh), _bits(y))
            ctx.check(ctx.lib.crux_mlp_backward(net.h, d_x, B, d_dy, gs, 1, d_dx))
            dx = np.empty_like(x); ctx.d2h(d_dx, dx); g = _grads(net)
            assert np.abs(g - gr).max() <= 1e-4 * np.abs(gr).max(), (name, gs, np.abs(g - gr).max(), np.abs(gr).max())
            assert np.abs(dx - dxr).max() <= 1e-4 * max(np.abs(dxr).max(), 1e-30)
            us = cache["us"]
        assert np.array_equal(net.get_params(), c["p"])                           # the passes train nothing
    finally:
        for d in (d_x, d_dy, d_y, d_dx):
            ctx.free(d)


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("name", GRID)
def test_twenty_consecutive_forwards(gpu_ctx, name, n_iter):
    ctx, c = gpu_ctx, case(name, n_iter); dims = c["dims"]
    x = np.asfortranarray(c["rng"].normal(0, 1, (dims[0], 37)).astype(np.float32))
    net = _net(ctx, c); us = c["us"]
    for it in range(20):
        yr, cache = SR.forward(c["p"], dims, c["acts"], c["sn"], us, x); us = cache["us"]
        y = net.forward(x)
        _state_close(net, cache, with_u=it == 0)
        assert _rel(y, yr), it
    assert all(abs(np.linalg.norm(u) - 1.0) < 1e-5 for u, _, _ in net.spectral_state())


# ---- 2. one discriminator step ---------------------------------------------------------------------------------------------------------------------------------------
def _rows(rng, od, ad, n):
    return {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": np.zeros((1, n), bool)}


def _buffer(ctx, rows, od, ad, capacity=None):
    crux = _crux()
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), capacity or rows["s"].shape[1], [], ctx=ctx)
    b.push_(rows); return b


GAIL_STEPS = [("3-12-1", 1), ("3-12-1", 3), ("3-64-64-2-1", 1), ("3-64-64-2-1", 3)]
OFF_STEPS = [("4-100-100-2", 1, 37), ("4-256-256-2", 1, 128), ("4-256-256-2", 3, 37), ("4-100-100-3", 1, 37), ("4-100-100-3", 3, 64)]


def gail_step_reference(name, n_iter):
    """crux_gail_d_step on rows [1, 34) of the expert and [2, 23) of the policy buffer, x = vcat(a, s): everything the test needs, from numpy alone"""
    c = case(name, n_iter); od, ad = c["dims"][0] - 1, 1
    ex, pi = _rows(c["rng"], od, ad, 40), _rows(c["rng"], od, ad, 30)
    xe = np.concatenate([ex["a"][:, 1:34], ex["s"][:, 1:34]], 0); xp = np.concatenate([pi["a"][:, 2:23], pi["s"][:, 2:23]], 0)
    loss, g, us, cache = SR.bce_step(c["p"], c["dims"], c["acts"], c["sn"], c["us"], xe, xp)
    return c, ex, pi, loss, g, cache


def off_step_reference(name, n_iter, Bd, counter=9):
    import offgail_reference as OR
    c = case(name, n_iter); K = c["dims"][-1]; od, ad = c["dims"][0] - 1, 1
    datas = [_rows(c["rng"], od, ad, n) for n in [300, 40, 77][:K]]
    X = OR.gather(datas, Bd, SEED, counter)
    loss, g, us, cache = SR.ce_step(c["p"], c["dims"], c["acts"], c["sn"], c["us"], X, K, Bd)
    return c, datas, loss, g, cache


def skipped_shares():
    """no device: per step case, the share of parameters whose float64 gradient is within 1e-3 of the gradient scale of zero"""
    out = {}
    for name, n_iter in GAIL_STEPS:
        g = gail_step_reference(name, n_iter)[4]; out[("gail", name, n_iter)] = float((np.abs(g) <= 1e-3 * np.abs(g).max()).mean())
    for name, n_iter, Bd in OFF_STEPS:
        g = off_step_reference(name, n_iter, Bd)[3]; out[("off", name, n_iter, Bd)] = float((np.abs(g) <= 1e-3 * np.abs(g).max()).mean())
    return out


def _check_step(net, info, c, loss, g, cache):
    from parity import L
    print("loss %.7g (ref %.7g) norm %.7g (ref %.7g)" % (info[L.INFO["loss"]], loss, info[L.INFO["grad_norm"]], np.linalg.norm(g)))
    assert abs(info[L.INFO["loss"]] - loss) <= 1e-4 * max(1.0, abs(loss))
    assert abs(info[L.INFO["grad_norm"]] - np.linalg.norm(g)) <= 1e-4 * max(1.0, np.linalg.norm(g))
    assert np.abs(_grads(net) - g).max() <= 1e-4 * np.abs(g).max()
    _state_close(net, cache)
    want = SR.adam_first_step(c["p"], g, lr=LR)
    ok = np.abs(g) > 1e-3 * np.abs(g).max(); left_out = 1.0 - ok.mean()
    got = net.get_params()
    print("  entries not compared: %.2f %%; worst parameter error %.3g" % (100 * left_out, np.abs(got[ok] - want[ok]).max()))
    assert left_out <= STEP_SKIPPED_MAX, left_out
    assert np.abs(got[ok] - want[ok]).max() < 2e-5
    assert np.isfinite(got).all()


@pytest.mark.parametrize("name,n_iter", GAIL_STEPS)
def test_gail_d_step_matches_reference(gpu_ctx, name, n_iter):
    from parity import L
    c, ex, pi, loss, g, cache = gail_step_reference(name, n_iter); od = c["dims"][0] - 1
    net, bex, bpi = _net(gpu_ctx, c), _buffer(gpu_ctx, ex, od, 1), _buffer(gpu_ctx, pi, od, 1)
    info = np.zeros(L.INFO_N, np.float32)
    gpu_ctx.check(gpu_ctx.lib.crux_gail_d_step(net.h, bex.h, 1, 33, bpi.h, 2, 21, _vp(info)))
    _check_step(net, info, c, loss, g, cache)


@pytest.mark.parametrize("name,n_iter,Bd", OFF_STEPS)
def test_offgail_d_step_matches_reference(gpu_ctx, name, n_iter, Bd):
    crux = _crux()
    c, datas, loss, g, cache = off_step_reference(name, n_iter, Bd); od = c["dims"][0] - 1
    net = _net(gpu_ctx, c); srcs = [_buffer(gpu_ctx, d, od, 1, capacity=d["s"].shape[1] + 13) for d in datas]
    info = crux.offgail_d_step_(net, srcs, Bd, SEED, 9)
    _check_step(net, info, c, loss, g, cache)


# ---- 3. the chained entries are their compositions, u included -------------------------------------------------------------------------------------------------------
def _full_state(net):
    st = [net.get_params()] + list(net.adam_state())
    for u, v, s in net.spectral_state():
        st += [u, v, np.array([s], np.float32)]
    return st


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name,n_iter", [("4-100-100-2", 1), ("4-256-256-2", 3), ("4-100-100-3", 1)])
def test_offgail_round_equals_steps_then_reward(gpu_ctx, name, n_iter):
    crux = _crux(); Bd, E, c0 = 64, 4, 35
    outs = []
    for mode in ("round", "steps"):
        c = case(name, n_iter); K = c["dims"][-1]
        datas = [_rows(c["rng"], 3, 1, n) for n in [256, 100, 64][:K]]; batch_rows = _rows(c["rng"], 3, 1, 96)
        net = _net(gpu_ctx, c); srcs = [_buffer(gpu_ctx, d, 3, 1) for d in datas]; batch = _buffer(gpu_ctx, batch_rows, 3, 1)
        if mode == "round":
            info = crux.offgail_round_(net, srcs, Bd, E, batch, SEED, c0)
        else:
            for e in range(E):
                info = crux.offgail_d_step_(net, srcs, Bd, SEED, c0 + e)
            crux.offgail_reward_(net, batch, K)
        outs.append(_full_state(net) + [batch["r"].copy(), np.asarray(info, np.float32)])
        assert np.isfinite(outs[-1][0]).all() and np.isfinite(batch["r"]).all() and not np.array_equal(outs[-1][0], c["p"])
    _same_lists(outs[0], outs[1])


def test_nda_round_is_its_parts_in_turn(gpu_ctx):
    """the NDA-GAIL round with two DenseSN discriminators against crux_gail_d_batch_train twice, the reward / cost pass and the advantages (tests/test_gpu_nda_gail.py)"""
    import test_gpu_nda_gail as NG
    from parity import L
    crux = _crux(); shape = NG.SHAPES[0]; c = NG.case(shape); B = c["B"]
    sets = []
    for _ in range(2):
        st = NG.Setup(gpu_ctx, c)
        for attr, key, sd in (("D", "pD", 21), ("N", "pN", 22)):
            dims, acts = c["dims"], c["acts"]; rng = np.random.default_rng(sd)
            cc = {"dims": dims, "acts": acts, "sn": tuple([1] * len(acts)), "p": c[key], "us": [rng.standard_normal(d).astype(np.float32) for d in dims[1:]]}
            setattr(st, attr, _net(gpu_ctx, cc))
        sets.append(st)
    a, b = sets
    rc, rD, rN, out3 = NG._round(a, B, 2, 3, 5, 9, mbN=7)
    gpu_ctx.check(rc)
    wD, _ = NG._chain(b.D, b.demo, b.copyD, B, 2, 5)
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((3, L.INFO_N), np.float32)
    gpu_ctx.check(gpu_ctx.lib.crux_gail_d_batch_train(b.N.h, b.nda.h, b.copyN.h, B, 3, 7, NG.SEED + 1, 9, _vp(raw), _vp(rows)))
    w3 = crux.nda_reward_cost_(b.D, b.N, b.batch, 0.3); crux.nda_advantages_(b.batch, b.V, b.Vc, 0.95, 0.99)
    _same_lists([rD, rN, out3], [wD, raw, np.array(w3, np.float32)])
    _same_lists(_full_state(a.D) + _full_state(a.N), _full_state(b.D) + _full_state(b.N))
    for k in ["r", "cost"] + NG.ADV_COLS:
        assert a.batch[k].tobytes() == b.batch[k].tobytes() and np.isfinite(a.batch[k]).all(), k
    assert not np.array_equal(a.D.get_params(), c["pD"]) and not np.array_equal(a.N.get_params(), c["pN"])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_entries_that_read_raw_weights_refuse_an_sn_handle(gpu_ctx):
    from parity import L
    crux = _crux(); ctx, lib = gpu_ctx, gpu_ctx.lib
    sn, sn2 = _net(ctx, case("3-12-1")), _net(ctx, case("3-12-1"))
    c = case("3-12-1"); c["sn"] = (0, 0); c["us"] = []
    plain, plain2 = _net(ctx, c), _net(ctx, c)
    info = np.zeros(L.INFO_N, np.float32); out = np.zeros(1, np.float32)
    rows = _rows(np.random.default_rng(0), 2, 1, 8); buf = _buffer(ctx, rows, 2, 1)
    d8 = ctx.alloc(64); ctx.h2d(d8, np.zeros(16, np.float32))
    try:
        calls = {
            "crux_policy_explore": lambda n: lib.crux_policy_explore(n.h, None, 1, None, 0, None, None, None),
            "crux_q_step": lambda n: lib.crux_q_step(n.h, buf.h, d8, 0, _vp(info)),
            "crux_polyak": lambda n: lib.crux_polyak(n.h, (sn2 if n is sn else plain2).h, 0.5),
            "crux_gradient_penalty": lambda n: lib.crux_gradient_penalty(n.h, d8, None, 4, 1.0, 1.0, 0, 0, 0, _vp(out)),
            "crux_train_step": lambda n: lib.crux_train_step(n.h, None, None, None, 0, None),
            "crux_batch_train": lambda n: lib.crux_batch_train(n.h, None, None, None, None, None),
        }
        for entry, f in calls.items():
            assert f(sn) == L.EUNSUP, entry
            assert entry in (lib.crux_last_error(ctx.h) or b"").decode(), entry
            assert f(plain) != L.EUNSUP, entry
        assert calls["crux_polyak"](plain) == 0 and calls["crux_q_step"](plain) == 0 and calls["crux_gradient_penalty"](plain) == 0
        assert lib.crux_polyak(plain.h, sn.h, 0.5) == L.EUNSUP                       # either side
        with pytest.raises(L.CruxError):
            crux.copyto_(plain, sn)                                                  # unequal SN layers
        crux.copyto_(sn2, sn)                                                        # equal ones: W and b only
    finally:
        ctx.free(d8)
    with pytest.raises(ValueError):
        crux.PolicyParams(sn)
    assert np.array_equal(sn.get_params(), case("3-12-1")["p"])


# ---- 5. the host mirror -----------------------------------------------------------------------------------------------------------------------------------------------
def _sn_chain(dims, acts):
    crux = _crux()
    return crux.Chain(*[crux.DenseSN(dims[i], dims[i + 1], acts[i]) for i in range(len(acts))])


def test_offpolicy_gail_solves_with_a_densesn_discriminator(gpu_ctx):
    import parity
    crux = _crux(); ctx = gpu_ctx
    ch = lambda i, o: parity.chain([i, 64, 64, o], ["relu", "relu", "identity"])      # noqa: E731
    pi = crux.ActorCritic(crux.GaussianPolicy(ch(3, 1), np.zeros(1, np.float32), seed=1, stream=0),
                          crux.DoubleNetwork(crux.ContinuousNetwork(ch(4, 1), seed=1, stream=1), crux.ContinuousNetwork(ch(4, 1), seed=1, stream=2)))
    D = crux.ContinuousNetwork(_sn_chain([4, 12, 2], ["relu", "identity"]), seed=7, ctx=ctx)      # Chain(DenseSN(., 12, relu), DenseSN(12, output))
    p0, s0 = D.get_params().copy(), D.spectral_state()
    assert all(s == 0.0 and np.isfinite(u).all() and np.abs(u).max() > 0 for u, _, s in s0)
    demo = _buffer(ctx, _rows(np.random.default_rng(11), 3, 1, 200), 3, 1)
    opt = {"batch_size": 32, "optimizer": crux.Adam(np.float32(LR))}
    # one iteration: the fill advances i to buffer_init first, and the loop runs while i <= N - dN (off_policy.jl:122-133), so N = buffer_init + dN
    sv = crux.OffPolicyGAIL(pi, crux.ContinuousSpace(3), demo, D, N=68, dN=4, buffer_size=300, buffer_init=64, max_steps=50,
                            d_opt={"epochs": 3, "batch_size": 16, "optimizer": crux.Adam(np.float32(LR))}, c_opt=dict(opt, epochs=2), a_opt=dict(opt), SAC_alpha_opt=dict(opt))
    crux.solve(sv, crux.PendulumMDP(n_envs=1, seed=0))
    s1 = D.spectral_state()
    assert all(s > 0 and np.isfinite(s) for _, _, s in s1) and any(not np.array_equal(a[0], b[0]) for a, b in zip(s0, s1))
    assert not np.array_equal(D.get_params(), p0) and np.isfinite(D.get_params()).all() and np.isfinite(pi.A.get_params()).all()
    assert len(sv.history) == 1 and sv.gail_rounds == 2 and np.isfinite(sv.history[-1]["discriminator_loss"])      # c_opt.epochs callbacks in the one iteration


def test_onpolicy_gail_solves_with_a_densesn_discriminator(gpu_ctx):
    import parity
    crux = _crux(); ctx = gpu_ctx; acts = ["relu", "relu", "identity"]
    S = crux.ContinuousSpace(3)
    pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 64, 64, 1], acts), np.zeros(1, np.float32), seed=1, ctx=ctx), crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=2, ctx=ctx))
    D = crux.ContinuousNetwork(_sn_chain([4, 12, 1], ["relu", "identity"]), seed=3, ctx=ctx)
    p0 = D.get_params().copy()
    rows = _rows(np.random.default_rng(5), 3, 1, 300); rows["episode_end"] = np.zeros((1, 300), bool)
    demo = crux.ExperienceBuffer(S, crux.ContinuousSpace(1), 300, ctx=ctx); demo.push_(rows)
    sv = crux.OnPolicyGAIL(pi, S, gamma=0.99, D=D, demo=demo, N=256, dN=256, max_steps=64, normalize_demo=False,
                           a_opt={"epochs": 2, "batch_size": 128}, c_opt={"epochs": 2, "batch_size": 128}, d_opt={"epochs": 2, "batch_size": 128}, target_kl=None)
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    st = D.spectral_state()
    assert len(sv.history) == 1 and all(s > 0 and np.isfinite(s) for _, _, s in st)
    assert not np.array_equal(D.get_params(), p0) and np.isfinite(D.get_params()).all() and np.isfinite(pi.A.get_params()).all()
    with pytest.raises(ValueError):      # DenseSN in a policy or critic network
        crux.OnPolicyGAIL(crux.ActorCritic(pi.A, crux.ContinuousNetwork(_sn_chain([3, 12, 1], ["relu", "identity"]), ctx=ctx)), S, gamma=0.99, D=D, demo=demo, N=256, dN=256)
