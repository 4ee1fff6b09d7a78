"""GPU: OffPolicyGAIL's discriminator step, round and reward rewrite (crux_offgail_d_step / _round / _reward, csrc/gail_off.hip) and AdRIL's ring relabel
(crux_adril_relabel) against the float64 restatement of tests/offgail_reference.py; OffPolicyGAIL and AdRIL through value_training / solve against the manual
composition of the entry points; and a learning check of the discriminator on separable sources.

Reference: src/model_free/il/off_policy_gail.jl, il/AdRIL.jl. Tolerances of the step are those of tests/test_gpu_iq.py / test_gpu_cql.py: 1e-4 relative on loss and
norm, 2e-5 absolute on parameters after one Adam step, entries whose float64 gradient is within 1e-3 of the gradient scale of zero not compared -- and that mask may
leave out at most 12 % of the entries. The reward's tolerance is measured against the float32 NumPy restatement (see test_reward_matches_float64).
"""
import ctypes as C
import os

import numpy as np
import pytest

import offgail_reference as R
import parity
from parity import crux, L

pytestmark = pytest.mark.gpu

LR = 1e-3
SEED = 0x5EED5A3F
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _dnet(dims, act, seed=5, lr=LR):
    acts = [act] * (len(dims) - 2) + ["identity"]
    net = crux.ContinuousNetwork(parity.chain(dims, acts), seed=seed, stream=0)
    net.attach_optimizer(crux.Adam(np.float32(lr)))
    return net, acts


def _rows(od, ad, n, onehot, seed, lo=None):
    """n transitions; lo: every coordinate of vcat(s, a) uniform in [lo, lo + 1] (continuous actions only)"""
    rng = np.random.default_rng(seed)
    if lo is not None:
        s, a = rng.uniform(lo, lo + 1, (od, n)).astype(np.float32), rng.uniform(lo, lo + 1, (ad, n)).astype(np.float32)
    else:
        s = rng.normal(0, 1, (od, n)).astype(np.float32)
        a = np.eye(ad, dtype=bool)[rng.integers(0, ad, n)].T.copy() if onehot else rng.normal(0, 1, (ad, n)).astype(np.float32)
    return {"s": s, "a": a, "sp": rng.normal(0, 1, (od, n)).astype(np.float32), "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.1}


def _buffer(ctx, data, capacity=None, extras=(), prioritized=False):
    od, ad, n = data["s"].shape[0], data["a"].shape[0], data["s"].shape[1]
    A = crux.DiscreteSpace(ad) if data["a"].dtype == bool else crux.ContinuousSpace(ad)
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), A, capacity or n, list(extras), prioritized=prioritized, ctx=ctx)
    if n:
        b.push_(data)
    return b


def _adam_state(net):
    return list(net.adam_state())


STEP_CASES = [("tanh", 2, False, 1, 5), ("tanh", 3, True, 1, 6), ("tanh", 4, False, 50, 5), ("relu", 2, True, 50, 5), ("relu", 3, False, 50, 6), ("relu", 4, True, 128, 5),
              ("relu", 2, False, 128, 7), ("tanh", 3, True, 128, 5), ("relu", 3, False, 128, 5), ("tanh", 2, True, 50, 7)]


@pytest.mark.parametrize("act,K,onehot,Bd,nseed", STEP_CASES, ids=["%s-K%d-%s-Bd%d-s%d" % (c[0], c[1], "onehot" if c[2] else "cont", c[3], c[4]) for c in STEP_CASES])
def test_d_step_matches_reference(gpu_ctx, act, K, onehot, Bd, nseed):
    ctx, od, ad, ctr = gpu_ctx, 4, 3, 9
    dims = [od + ad, 32, 32, K]
    net, acts = _dnet(dims, act, seed=nseed)
    lens = [300, 40, 77, 150][:K]                                             # different lengths; the second is shorter than Bd = 50 and 128
    datas = [_rows(od, ad, n, onehot, 20 + k) for k, n in enumerate(lens)]
    srcs = [_buffer(ctx, d, capacity=n + 13) for d, n in zip(datas, lens)]    # sampled over len, not capacity
    p0 = net.get_params()
    X = R.gather(datas, Bd, SEED, ctr)
    layers = R.mlp_params(p0, dims)
    loss = R.ce_loss(layers, acts, X, K, Bd); loss.backward(); g_ref = R.flat_grad(layers)
    info = crux.offgail_d_step_(net, srcs, Bd, SEED, ctr)
    print("d_step %s K=%d Bd=%d: loss %.7g (ref %.7g) norm %.7g (ref %.7g)" % (act, K, Bd, info[L.INFO["loss"]], float(loss), info[L.INFO["grad_norm"]], np.linalg.norm(g_ref)))
    assert _close(info[L.INFO["loss"]], float(loss)), (info[0], float(loss))
    assert _close(info[L.INFO["grad_norm"]], np.linalg.norm(g_ref)), (info[1], np.linalg.norm(g_ref))
    want = R.adam_first_step(p0.astype(np.float64), g_ref, lr=LR)
    ok = np.abs(g_ref) > 1e-3 * np.abs(g_ref).max()
    left_out = 1.0 - ok.mean()
    print("  entries not compared: %.2f %%; worst parameter error %.3g" % (100 * left_out, np.abs(net.get_params()[ok] - want[ok]).max()))
    assert left_out <= 0.12, left_out
    assert np.abs(net.get_params()[ok] - want[ok]).max() < 2e-5


@pytest.mark.parametrize("onehot", [False, True])
def test_gathered_columns_are_the_rows_uniform_sample_draws(gpu_ctx, onehot):
    ctx, od, ad, Bd, ctr = gpu_ctx, 5, 3, 50, 4
    lens = [200, 31, 90]
    datas = [_rows(od, ad, n, onehot, 30 + k) for k, n in enumerate(lens)]
    srcs = [_buffer(ctx, d, capacity=n + 5) for d, n in zip(datas, lens)]
    X = crux.offgail_gather(srcs, Bd, SEED, ctr)
    assert np.array_equal(X.view(np.uint32), np.ascontiguousarray(R.gather(datas, Bd, SEED, ctr)).view(np.uint32))
    for k, src in enumerate(srcs):                                             # the library's own uniform_sample! with (seed, stream 16 + k, counter)
        crux.set_sample_stream_(src, SEED, 16 + k)
        t = crux.buffer_like(src, capacity=Bd)
        crux.uniform_sample_(t, src, B=Bd, i=ctr)
        want = np.concatenate([t["s"], t["a"].astype(np.float32)], axis=0)
        assert np.array_equal(X[:, k * Bd:(k + 1) * Bd].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), k
        assert np.array_equal(np.asarray(t.indices[:Bd]), R.sample_ids(SEED, 16 + k, ctr, Bd, lens[k]))


def _round_setup(ctx, K, seed=3, act="relu", nan=False):
    od, ad = 3, 1
    datas = [_rows(od, ad, n, False, 40 + k) for k, n in enumerate([256, 100, 64][:K])]
    if nan:
        datas[0]["s"][1, :] = np.where(np.arange(256) % 2 == 0, np.nan, datas[0]["s"][1, :])      # every draw of 64 demo rows meets one
    srcs = [_buffer(ctx, d) for d in datas]
    batch = _buffer(ctx, _rows(od, ad, 96, False, 50))
    net, acts = _dnet([od + ad, 64, 64, K], act, seed=seed)
    return net, srcs, batch


@pytest.mark.parametrize("K", [2, 3])
def test_round_equals_steps_then_reward(gpu_ctx, K):
    ctx, Bd, E, c0 = gpu_ctx, 64, 5, 35
    outs = []
    for mode in ("round", "round", "steps"):
        net, srcs, batch = _round_setup(ctx, K)
        if mode == "round":
            info = crux.offgail_round_(net, srcs, Bd, E, batch, SEED, c0)
        else:
            for e in range(E):
                info = crux.offgail_d_step_(net, srcs, Bd, SEED, c0 + e)
            crux.offgail_reward_(net, batch, K)
        outs.append([net.get_params(), batch["r"].copy(), info] + _adam_state(net))
    for other in outs[1:]:
        assert len(other) == len(outs[0])
        for a, b in zip(outs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(np.isfinite(outs[0][1])) and np.isfinite(outs[0][2][:2]).all()


def _reward_case(ctx, K, spread, seed):
    """a discriminator whose logits on the batch have the wanted spread: a linear map of the state, scaled"""
    od, ad, B = 3, 1, 512
    batch_data = _rows(od, ad, B, False, seed)
    net, acts = _dnet([od + ad, K], "relu", seed=seed)
    p = net.get_params().astype(np.float64)
    W = p[:(od + ad) * K].reshape((K, od + ad), order="F")
    x = np.concatenate([batch_data["s"], batch_data["a"]], 0).astype(np.float64)
    z = W @ x
    sc = spread / (z.max(0) - z.min(0)).max()
    p[:(od + ad) * K] *= sc
    net.set_params(p.astype(np.float32))
    return net, _buffer(ctx, batch_data), batch_data


def test_reward_matches_float64(gpu_ctx):
    """The GPU's worst error against float64 must not exceed 4 x max(e32, 1e-6), e32 = the worst error of the float32 NumPy restatement on the same logits:
    log(1 - p + 1e-5) amplifies the float32 rounding of 1 - p by up to 1 / (1 - p + 1e-5), so the yardstick is what float32 itself can do on these inputs."""
    lines = []
    for K in (2, 3, 4):
        net, batch, d = _reward_case(gpu_ctx, K, 6.0, 60 + K)
        layers = R.mlp_params(net.get_params(), [4, K])
        x = np.concatenate([d["s"], d["a"]], 0)
        z64 = R.mlp(layers, ["identity"], __import__("torch").as_tensor(x.astype(np.float64))).detach().numpy()
        assert (z64.max(0) - z64.min(0)).max() <= 6.0 + 1e-6
        r64 = R.reward(z64)
        W32 = net.get_params()[:4 * K].reshape((K, 4), order="F"); b32 = net.get_params()[4 * K:]
        z32 = (W32 @ x.astype(np.float32) + b32[:, None]).astype(np.float32)
        e32 = float(np.abs(R.reward(z32, np.float32).astype(np.float64) - r64).max())
        mean_r = crux.offgail_reward_(net, batch, K)
        got = batch["r"][0].astype(np.float64)
        eg = float(np.abs(got - r64).max())
        bound = 4 * max(e32, 1e-6)
        lines.append("K=%d  B=512  logit spread <= 6: e32 (float32 NumPy vs float64) %.3e   GPU vs float64 %.3e   ratio %.2f   bound 4 x max(e32, 1e-6) = %.3e" % (K, e32, eg, eg / max(e32, 1e-6), bound))
        print(lines[-1])
        assert eg <= bound, (K, eg, e32)
        assert _close(mean_r, r64.mean(), 1e-4)
    try:
        os.makedirs(PROFILES, exist_ok=True)
        with open(os.path.join(PROFILES, "offgail_parity.txt"), "w") as f:
            f.write("crux_offgail_reward against the float64 restatement (tests/test_gpu_offgail.py::test_reward_matches_float64)\n" + "\n".join(lines) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("K", [2, 4])
def test_reward_saturated_is_finite_and_bounded(gpu_ctx, K):
    net, batch, _d = _reward_case(gpu_ctx, K, 40.0, 70 + K)
    crux.offgail_reward_(net, batch, K)
    r = batch["r"][0]
    assert np.all(np.isfinite(r)) and np.abs(r).max() <= R.TERM_BOUND * np.abs(R.weights(K)).sum() * (1 + 1e-6)


def test_nan_demo_state_stops_the_round(gpu_ctx):
    ctx, K, Bd = gpu_ctx, 2, 64
    net, srcs, batch = _round_setup(ctx, K, nan=True)
    p0, r0, st0 = net.get_params(), batch["r"].copy(), _adam_state(net)
    with pytest.raises(L.CruxError) as e:
        crux.offgail_round_(net, srcs, Bd, 3, batch, SEED, 0)
    assert e.value.code == L.ENAN and "NaN detected" in str(e.value)
    assert np.array_equal(net.get_params(), p0) and np.array_equal(batch["r"], r0)
    assert all(np.array_equal(a, b) for a, b in zip(_adam_state(net), st0))
    with pytest.raises(L.CruxError) as e:
        crux.offgail_d_step_(net, srcs, Bd, SEED, 0)
    assert e.value.code == L.ENAN and np.array_equal(net.get_params(), p0)


def test_refusals(gpu_ctx):
    ctx, od, ad = gpu_ctx, 3, 1
    mk = lambda n, **kw: _buffer(ctx, _rows(od, ad, n, False, 80), **kw)
    demo, ring, batch = mk(50), mk(60), mk(32)
    D2, _ = _dnet([4, 16, 2], "relu"); D3, _ = _dnet([4, 16, 3], "relu"); Dw, _ = _dnet([5, 16, 2], "relu")

    def refused(code, fn):
        with pytest.raises(L.CruxError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert len(str(e.value)) > 10
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D2, [demo], 8, SEED, 0))                                       # K < 2
    refused(L.EINVAL, lambda: crux.offgail_d_step_(Dw, [demo, ring], 8, SEED, 0))                                 # input width
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D3, [demo, ring], 8, SEED, 0))                                 # output width != K
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D2, [demo, _buffer(ctx, _rows(od, 2, 20, False, 81))], 8, SEED, 0))       # act_dim differs
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D2, [demo, _buffer(ctx, _rows(2, ad, 20, False, 81))], 8, SEED, 0))       # obs_dim differs
    refused(L.EINVAL, lambda: crux.offgail_round_(D2, [demo, ring], 8, 2, _buffer(ctx, _rows(od, 2, 20, False, 82)), SEED, 0))   # batch differs
    oh = _buffer(ctx, _rows(3, 2, 20, True, 83)); Doh, _ = _dnet([5, 16, 2], "relu")
    refused(L.EINVAL, lambda: crux.offgail_d_step_(Doh, [oh, _buffer(ctx, _rows(3, 2, 20, False, 84))], 8, SEED, 0))         # action kind differs
    empty = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), 10, ctx=ctx)
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D2, [demo, empty], 8, SEED, 0))                                # an empty source
    refused(L.EINVAL, lambda: crux.offgail_d_step_(D2, [demo, ring], 0, SEED, 0))                                 # Bd < 1
    per = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), 64, prioritized=True, ctx=ctx); per.push_(_rows(od, ad, 40, False, 85))
    refused(L.EUNSUP, lambda: crux.offgail_d_step_(D2, [demo, per], 8, SEED, 0))                                  # a prioritized source
    refused(L.EUNSUP, lambda: crux.offgail_d_step_(D2, [demo, ring], (1 << 19) + 1, SEED, 0))                     # K Bd > 2^20
    p0 = D2.get_params()
    crux.offgail_round_(D2, [demo, ring], 8, 1, batch, SEED, 0)                                                   # and the accepted call still works afterwards
    assert not np.array_equal(D2.get_params(), p0)


# ---- AdRIL -----------------------------------------------------------------------------------------------------------------------------------------------------------
def _ring(ctx, cap):
    return crux.ExperienceBuffer(crux.ContinuousSpace(2), crux.ContinuousSpace(1), cap, ["i"], ctx=ctx)


def _push_block(ring, i_vals, seed=0):
    n = len(i_vals); d = _rows(2, 1, n, False, 90 + seed)
    d["i"] = np.asarray(i_vals, np.int64).reshape(1, n); d["r"][...] = 7.0
    ring.push_(d)


def _ring_state(ring):
    n = len(ring); return ring["i"][0, :n].copy(), ring["r"][0, :n].copy()


@pytest.mark.parametrize("cap,buffer_init", [(1000, 0), (120, 0)])
def test_adril_relabel_matches_callback_then_push(gpu_ctx, cap, buffer_init):
    ring, host, dN = _ring(gpu_ctx, cap), R.HostRing(cap), 50
    for t in range(5):
        iv = np.arange(buffer_init + 50 * t + 1, buffer_init + 50 * t + 51)
        R.adril_steps(host, iv, buffer_init, dN)
        _push_block(ring, iv, t)
        mx, k = crux.adril_relabel_(ring, 50, buffer_init, dN)
        gi, gr = _ring_state(ring); n = len(host)
        assert np.array_equal(gi, host.i[:n]) and np.array_equal(gr.view(np.uint32), host.r[:n].view(np.uint32)), t
        assert mx == 50 * (t + 1) + buffer_init and k == (0 if t == 0 else t)


def test_adril_k_zero_and_non_divisible_and_missing_column(gpu_ctx):
    ring, host = _ring(gpu_ctx, 100), R.HostRing(100)
    for iv in (np.arange(101, 121), np.arange(121, 151)):
        R.adril_steps(host, iv, 100, 50); _push_block(ring, iv); crux.adril_relabel_(ring, len(iv), 100, 50)
    col = ring["i"]; col[0, :5] = 100; ring["i"] = col; host.i[:5] = 100                 # crafted :i: rows old enough while k == 0
    iv = np.arange(141, 151)
    R.adril_steps(host, iv, 100, 50); _push_block(ring, iv)
    mx, k = crux.adril_relabel_(ring, 10, 100, 50)
    gi, gr = _ring_state(ring)
    assert (mx, k) == (150, 0) and np.all(np.isneginf(gr[:5])) and np.array_equal(gr.view(np.uint32), host.r[:60].view(np.uint32))
    # non-divisible: refused, rewards as they were
    _push_block(ring, np.arange(151, 178))
    _i0, r0 = _ring_state(ring)
    with pytest.raises(L.CruxError) as e:
        crux.adril_relabel_(ring, 27, 100, 50)
    assert e.value.code == L.EINVAL and "InexactError" in str(e.value)
    assert np.array_equal(_ring_state(ring)[1].view(np.uint32), r0.view(np.uint32))
    plain = _buffer(gpu_ctx, _rows(2, 1, 30, False, 3))
    with pytest.raises(L.CruxError) as e:
        crux.adril_relabel_(plain, 10, 0, 50)
    assert e.value.code == L.EINVAL and ":i" in str(e.value)


def test_adril_relabel_million_rows(gpu_ctx):
    n, dN = 1 << 20, 1 << 14
    ring = _ring(gpu_ctx, n)
    d = {"s": np.zeros((2, n), np.float32), "a": np.zeros((1, n), np.float32), "sp": np.zeros((2, n), np.float32), "r": np.full((1, n), 3.0, np.float32),
         "done": np.zeros((1, n), bool), "i": np.arange(1, n + 1, dtype=np.int64).reshape(1, n)}
    ring.push_(d)
    mx, k = crux.adril_relabel_(ring, dN, 0, dN)
    assert (mx, k) == (n, n // dN - 1)
    r = ring["r"][0]
    want = np.where(np.arange(1, n + 1) <= n - dN, np.float32(-1.0 / k), np.float32(0))      # closed form: the newest dN rows are fresh, every other row is old
    assert np.array_equal(r.view(np.uint32), want.astype(np.float32).view(np.uint32))


# ---- through the solvers ---------------------------------------------------------------------------------------------------------------------------------------------
def _sac_pi(seed=1):
    ch = lambda i, o: parity.chain([i, 64, 64, o], ["relu", "relu", "identity"])
    return crux.ActorCritic(crux.GaussianPolicy(ch(3, 1), np.zeros(1, np.float32), seed=seed, stream=0),
                            crux.DoubleNetwork(crux.ContinuousNetwork(ch(4, 1), seed=seed, stream=1), crux.ContinuousNetwork(ch(4, 1), seed=seed, stream=2)))


def _all_params(sv):
    pi, pim = sv.agent.pi, sv.agent.pi_minus
    return [pi.A.get_params(), pi.C.N1.get_params(), pi.C.N2.get_params(), pim.C.N1.get_params(), pim.C.N2.get_params(), sv.P["SAC_log_alpha"].get_params(), sv.discriminator.get_params()]


@pytest.mark.parametrize("n_nda", [0, 1])
def test_offpolicy_gail_value_training_matches_manual_composition(gpu_ctx, n_nda):
    ctx, B, Bd, epochs, d_epochs = gpu_ctx, 32, 16, 2, 3
    demo_data = _rows(3, 1, 200, False, 11); nda_data = [_rows(3, 1, 90, False, 12)][:n_nda]
    runs = []
    for manual in (False, True):
        demo = _buffer(ctx, demo_data); ndas = [_buffer(ctx, d) for d in nda_data]
        D, _ = _dnet([4, 32, 32, 2 + n_nda], "relu", seed=7)
        opt = {"batch_size": B, "optimizer": crux.Adam(np.float32(LR))}
        sv = crux.OffPolicyGAIL(_sac_pi(), crux.ContinuousSpace(3), demo, D, ndas=ndas, N=100, dN=4, buffer_size=300, d_opt={"epochs": d_epochs, "batch_size": Bd, "optimizer": crux.Adam(np.float32(LR))},
                                c_opt=dict(opt, epochs=epochs), a_opt=dict(opt), SAC_alpha_opt=dict(opt), noise_seed=5)
        sv.buffer.push_(_rows(3, 1, 150, False, 13))
        Dst = crux.buffer_like(sv.buffer, capacity=B)
        hist = []
        for it in range(2):
            sv.i = 20 + it
            if not manual:
                hist.append(crux.value_training(sv, Dst, np.float32(0.99))); continue
            pi, pim, la = sv.agent.pi, sv.agent.pi_minus, sv.P["SAC_log_alpha"]
            (_, t_opt), = sv.param_optimizers
            for net, p in ((pi.C.N1, sv.c_opt), (pi.C.N2, sv.c_opt), (pi.A, sv.a_opt), (la, t_opt), (D, sv.d_opt)):
                crux.api._ensure_opt(net, p)
            dy = ctx.alloc(4 * B); raw = np.zeros(L.INFO_N, np.float32); infos = []; vp = raw.ctypes.data_as(C.c_void_p)
            for ep in range(epochs):
                ctr = sv.i * epochs + ep; info = {}
                sv._rand(Dst, ctr)
                rd = crux.offgail_round_(D, [sv.demo, sv.buffer] + sv.ndas, Bd, d_epochs, Dst, sv.sample_seed, (it * epochs + ep) * d_epochs)
                info.update({"discriminator_loss": float(rd[0]), "discriminator_grad_norm": float(rd[1])})
                ctx.check(ctx.lib.crux_sac_target(pi.A.h, pim.C.N1.h, pim.C.N2.h, la.h, Dst.h, 0.99, sv.noise_seed, 3 * ctr, dy))
                ctx.check(ctx.lib.crux_sac_temp_step(pi.A.h, la.h, Dst.h, float(sv.P["SAC_H_target"]), sv.noise_seed, 3 * ctr + 1, vp))
                info.update({"temp_loss": float(raw[0]), "temp_grad_norm": float(raw[1]), "SAC alpha": float(raw[L.INFO["alpha"]])})
                ctx.check(ctx.lib.crux_double_q_step(pi.C.N1.h, pi.C.N2.h, Dst.h, dy, 0, vp))
                info.update({"critic_loss": float(raw[0]), "critic_grad_norm": float(raw[1]), "Q1avg": float(raw[L.INFO["q1avg"]]), "Q2avg": float(raw[L.INFO["q2avg"]])})
                ctx.check(ctx.lib.crux_sac_actor_step(pi.A.h, pi.C.N1.h, pi.C.N2.h, la.h, Dst.h, sv.noise_seed, 3 * ctr + 2, vp))
                info.update({"actor_loss": float(raw[0]), "actor_grad_norm": float(raw[1]), "entropy": float(raw[L.INFO["entropy"]])})
                crux.polyak_average_(pim, pi, sv.tau)
                infos.append(info)
            ctx.free(dy)
            hist.append({k: float(np.mean([d[k] for d in infos])) for k in infos[0]})
        runs.append((_all_params(sv), hist, Dst["r"].copy()))
        assert np.array_equal(demo["s"], demo_data["s"]) and np.array_equal(demo["a"], demo_data["a"]) and np.array_equal(demo["r"], demo_data["r"])      # the caller's buffer
        assert sv.demo is not demo and sv.discriminator is D and len(sv.ndas) == n_nda
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32))
    assert set(runs[0][1][-1]) == set(runs[1][1][-1]) and {"discriminator_loss", "discriminator_grad_norm", "critic_loss", "actor_loss", "temp_loss"} <= set(runs[0][1][-1])
    for k, v in runs[0][1][-1].items():
        assert v == runs[1][1][-1][k], (k, v, runs[1][1][-1][k])


def test_offpolicy_gail_rejects_what_it_cannot_run(gpu_ctx):
    demo = _buffer(gpu_ctx, _rows(3, 1, 50, False, 1)); S = crux.ContinuousSpace(3)
    D3, _ = _dnet([4, 16, 3], "relu")
    with pytest.raises(ValueError):
        crux.OffPolicyGAIL(_sac_pi(), S, demo, D3, N=100)                                        # 3 outputs, no NDA buffer
    with pytest.raises(TypeError):
        crux.OffPolicyGAIL(_sac_pi(), S, demo, crux.DiscreteNetwork(parity.chain([4, 16, 2], ["relu", "identity"]), [1, 2]), N=100)
    D2, _ = _dnet([4, 16, 2], "relu")
    with pytest.raises(NotImplementedError):
        crux.OffPolicyGAIL(_sac_pi(), S, demo, D2, N=100, prioritized=True)
    sv = crux.OffPolicyGAIL(_sac_pi(), S, demo, D3, ndas=[_buffer(gpu_ctx, _rows(3, 1, 20, False, 2))], normalize_demo=False, N=100)      # allowed here (see the docstring)
    assert len(sv.ndas) == 1 and sv.d_opt.epochs == 5 and sv.d_opt.name == "discriminator_" and sv.d_opt.batch_size == 128


@pytest.mark.parametrize("buffer_init", [0, 100])
def test_adril_solve_relabels_the_ring_like_the_reference(gpu_ctx, buffer_init):
    ctx, dN, B = gpu_ctx, 50, 32
    demo_data = _rows(3, 1, 128, False, 21); demo_data["r"][...] = np.random.default_rng(2).uniform(0.5, 2.0, (1, 128)).astype(np.float32)
    demo = _buffer(ctx, demo_data)
    mdp = crux.PendulumMDP(n_envs=1, seed=3)
    opt = {"batch_size": B}
    sv = crux.AdRIL(_sac_pi(), mdp.state_space(), demo, dN=dN, N=3 * dN + buffer_init, buffer_size=120 if buffer_init == 0 else 400, buffer_init=buffer_init, max_steps=40,
                    c_opt=dict(opt, epochs=2), a_opt=dict(opt), SAC_alpha_opt=dict(opt))
    assert sv.buffer.haskey("i") and sv.post_sample_callback is None and sv.post_sample_device is not None and sv.buffer_fractions == [0.5, 0.5]
    crux.solve(sv, mdp)
    # the restatement, fed the :i values the rollouts wrote: the pre-fill block (if any), then three blocks of dN
    host = R.HostRing(sv.buffer.capacity)
    if buffer_init:
        R.adril_steps(host, buffer_init + np.arange(1, buffer_init + 1), buffer_init, dN)
    for t in range(3):
        R.adril_steps(host, buffer_init + dN * t + np.arange(1, dN + 1), buffer_init, dN)
    gi, gr = _ring_state(sv.buffer); n = len(host)
    assert len(sv.buffer) == n and np.array_equal(gi, host.i[:n])
    assert np.array_equal(gr.view(np.uint32), host.r[:n].view(np.uint32)), (gr, host.r[:n])
    assert np.array_equal(sv.demo["r"], demo_data["r"]) and np.array_equal(demo["r"], demo_data["r"])      # the demonstrations keep their rewards
    assert len(sv.history) == 3 and all(np.isfinite(v) for h in sv.history for v in h.values())


def test_adril_requires_demo_rewards(gpu_ctx):
    class NoRewards:
        def haskey(self, k): return k != "r"
    with pytest.raises(ValueError, match="AdRIL requires a reward value for the demonstrations"):
        crux.AdRIL(_sac_pi(), crux.ContinuousSpace(3), NoRewards(), N=100)


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
def test_discriminator_learns_separable_sources(gpu_ctx, K):
    """Sources drawn from disjoint unit boxes (box k = [2k - 1, 2k] in every coordinate of vcat(s, a)): after 200 rounds of 5 epochs the loss is below log(K) / 2
    (log(K) = a head that cannot tell the classes apart) and demo rows earn more than policy rows."""
    ctx, Bd = gpu_ctx, 128
    datas = [_rows(3, 1, 512, False, 100 + k, lo=2.0 * k - 1.0) for k in range(K)]
    srcs = [_buffer(ctx, d) for d in datas]
    net, _acts = _dnet([4, 64, 64, K], "relu", seed=2, lr=1e-3)
    batch = _buffer(ctx, {k: np.concatenate([datas[0][k][:, :64], datas[1][k][:, :64]], axis=1) for k in datas[0]})
    for rd in range(200):
        info = crux.offgail_round_(net, srcs, Bd, 5, batch, SEED, 5 * rd)
    r = batch["r"][0]
    print("separable sources K=%d: last discriminator_loss %.3e (log(K)/2 = %.3f), mean reward demo %.3f policy %.3f" % (K, info[0], np.log(K) / 2, r[:64].mean(), r[64:].mean()))
    assert info[L.INFO["loss"]] < np.log(K) / 2
    assert r[:64].mean() > r[64:].mean()
