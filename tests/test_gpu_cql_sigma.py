"""GPU: CQL with a two-headed actor -- crux_cql_conservative_sigma / _alpha_step_sigma / _critic_step_sigma (csrc/cql.hip, k_cql_expand_sigma) and CQL(..., two_headed=True)
(crux.jl_amd/batch.py) -- against the float64 yardstick of tests/cql_sigma_reference.py (QR), which is built on tests/sigma_head_reference.py (SR) and tests/cql_reference.py (CR).

Tolerances are the project's own (tests/test_gpu_cql.py, test_gpu_sigma_head.py): 1e-4 relative on losses, norms, means and the steps' values, 1e-4 of the gradient scale on raw
gradients, 2e-5 absolute on parameters after one Adam step at lr 1e-3, where entries whose float64 gradient lies within 1e-3 of the gradient scale of zero are left out (Adam's
first step is lr sign(g) there). At most a quarter of a handle may be left out: tests/test_cql_sigma_reference.py asserts that on every case from the yardstick's own samples and
this file asserts it again on the share it sees (the gradient of the float64 losses fed the device's samples). Sampled actions: 2e-5 max(1, |a|max). Their logprobs get an
absolute tolerance by SR.tolerance's rule, four times the largest error of the float32 restatement against float64 over the case's own N B samples (the margin covers the tile
GEMMs' other summation order and the device's exp / log / tanh):
    case (shape, B, ascale, N)        float32 error a / lp       tolerance lp    largest device error a / lp (MI355X, profiles/cql_asaf_sigma_tests.txt)
    2-32-2x1          37  0     3          1.600e-07 / 4.087e-07      1.635e-06       1.116e-07 / 5.734e-07
    2-32-2x1           1  2     2          1.089e-07 / 6.361e-08      2.544e-07       1.295e-07 / 1.748e-07
    5-100-100-2x3     37  2     4          8.222e-07 / 1.695e-06      6.782e-06       5.725e-07 / 9.209e-07
    5-100-100-2x3    257  0     2          4.684e-07 / 1.212e-06      4.846e-06       4.030e-07 / 1.212e-06
    4-256-256-2x2    257  1     3          7.308e-07 / 1.733e-06      6.933e-06       3.934e-07 / 1.774e-06
    4-256-256-2x2     37  2    10          1.304e-06 / 1.498e-06      5.992e-06       6.250e-07 / 9.041e-07
    17-256-256-2x6    37  2     4          1.090e-06 / 1.969e-06      7.876e-06       5.808e-07 / 1.120e-06
    5-100-100-2x3     37  1     2          3.123e-07 / 4.846e-06      1.939e-05       3.719e-07 / 3.422e-06
(the last row is the clamp case, SR.case(..., clamp=0).)
Policy sample block 0 and its logprobs are crux_sigma_head_explore's bits (pi.exploration(s, SEED, ctr)); the uniform blocks are CR.uniform_samples' bits. Every test prints its
figures before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

import cql_reference as CR
import cql_sigma_reference as QR
import ensemble_reference as ER
import parity
import sigma_gpu_cases as G
from parity import crux, L

pytestmark = pytest.mark.gpu
SEED, CTR, THRESH, LO, HI, LR = QR.SEED, QR.CTR, QR.THRESH, QR.LO, QR.HI, QR.LR
ALL = QR.CASES + [QR.CLAMP_CASE]
IDS = ["%s-B%d-x%g-N%d" % r for r in ALL]
vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731


def _case(row):
    name, B, sc, N = row
    return QR.case(name, B, sc, 0 if row == QR.CLAMP_CASE else None), N


def _nets(c, ctx, log_alpha, opt=True):
    pi, q1, q2 = G.actor(c, ctx), G.qnet(c, "q1", ctx), G.qnet(c, "q2", ctx); la = crux.ParamVector([np.float32(log_alpha)], ctx=ctx)
    for n in (pi, q1, q2, la) if opt else ():
        n.attach_optimizer(crux.Adam(np.float32(LR)))
    return pi, q1, q2, la


def _conservative(ctx, pi, q1, q2, la, b, N, ctr=CTR, seed=SEED):
    B, ad = len(b), b.act_dim
    d_s, d_lp = ctx.alloc(4 * ad * 2 * N * B), ctx.alloc(4 * 2 * N * B); out = np.zeros(4, np.float32)
    ctx.check(ctx.lib.crux_cql_conservative_sigma(pi.h, q1.h, q2.h, la.h, b.h, N, LO, HI, THRESH, seed, ctr, vp(out), d_s, d_lp))
    samp, lp = np.empty((ad, 2 * N * B), np.float32, order="F"), np.empty(2 * N * B, np.float32)
    ctx.d2h(d_s, samp); ctx.d2h(d_lp, lp); ctx.free(d_s); ctx.free(d_lp)
    return out, samp, lp


@pytest.mark.parametrize("row", ALL, ids=IDS)
def test_samples_and_the_conservative_value(gpu_ctx, row):
    ctx = gpu_ctx; c, N = _case(row); B, ad, sc = c["B"], c["ad"], c["ascale"]
    pi, q1, q2, la = _nets(c, ctx, c["log_alpha"], opt=False); b = G.batch(c, ctx)
    out, samp, lp = _conservative(ctx, pi, q1, q2, la, b, N)
    ua, ulp = CR.uniform_samples(SEED, CTR, N, B, ad, LO, HI)
    assert np.array_equal(samp[:, N * B:], ua) and np.array_equal(lp[N * B:], ulp)                      # bit for bit
    a0, lp0 = pi.exploration(c["s"], SEED, CTR)                                                          # crux_sigma_head_explore: the k = 0 streams
    assert np.array_equal(samp[:, :B].view(np.uint32), np.ascontiguousarray(a0, np.float32).view(np.uint32))
    assert np.array_equal(lp[:B].view(np.uint32), np.ascontiguousarray(lp0[0], np.float32).view(np.uint32))
    ra, rlp = QR.policy_samples(c, N); e_a, e_lp = np.abs(samp[:, :N * B] - ra).max(), np.abs(lp[:N * B] - rlp).max()
    f_a, f_lp = QR.lp_error32(c, N); tol = QR.lp_tolerance(c, N); amax = np.abs(ra).max()
    print("samples %-16s B=%-4d ascale=%g N=%-2d: float32 error a %.3e lp %.3e, tolerance lp %.3e, device error a %.3e (bound %.3e) lp %.3e" %
          (row + (f_a, f_lp, tol, e_a, 2e-5 * max(1.0, amax), e_lp)))
    for log_alpha in QR.log_alphas(c) + (QR.BETA_CLAMP,):
        la.set_params(np.array([log_alpha], np.float32)); o2, s2, l2 = _conservative(ctx, pi, q1, q2, la, b, N)
        assert np.array_equal(s2, samp) and np.array_equal(l2, lp)
        lse, qd, beta, loss = (v.item() for v in QR.conservative(c, samp, lp, float(np.float32(log_alpha))))
        print("  conservative log alpha %+.3f:" % log_alpha, o2, lse, qd, beta, loss)
        assert G.close(o2[0], lse) and G.close(o2[1], qd) and G.close(o2[2], beta) and G.close(o2[3], loss)
    assert o2[2] == np.float32(1e6)
    assert e_a <= 2e-5 * max(1.0, amax) and e_lp <= tol
    if sc > 0:
        assert np.abs(samp[:, :N * B]).max() <= sc


def _check_critic_step(ctx, c, N, log_alpha, weighted=False, ctr=CTR):
    w = QR.weights(c) if weighted else None
    pi, q1, q2, la = _nets(c, ctx, log_alpha); b = G.batch(c, ctx, weight=w); B = c["B"]
    y = QR.target(c); d_y = ctx.alloc(4 * B); ctx.h2d(d_y, y)
    _, samp, lp = _conservative(ctx, pi, q1, q2, la, b, N, ctr)      # the samples the step draws (same counter)
    rinfo, gs, ps = QR.critic_step(c, samp, lp, float(la.get_params()[0]), y, w)
    before = G.state([pi, la]); info = np.zeros(L.INFO_N, np.float32)
    ctx.check(ctx.lib.crux_cql_critic_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, d_y, N, LO, HI, THRESH, 1 if weighted else 0, SEED, ctr, vp(info))); ctx.free(d_y)
    print("critic %s B=%d ascale=%g N=%d log alpha %+.3f%s:" % (c["name"], B, c["ascale"], N, log_alpha, " weighted" if weighted else ""),
          info[[0, 1, L.INFO["q1avg"], L.INFO["q2avg"]]], rinfo)
    res = []
    for net, g, p in zip((q1, q2), gs, ps):
        gg = G.grads(net, ctx); keep = np.abs(g) > 1e-3 * np.abs(g).max()
        res.append((np.abs(gg - g).max() / np.abs(g).max(), np.abs(net.get_params() - p)[keep].max(), ER.skipped_share(g)))
        print("  gradient error / scale %.2e, parameters %.2e, left out %.4f" % res[-1])
    assert G.close(info[0], rinfo["loss"]) and G.close(info[1], rinfo["grad_norm"])
    assert G.close(info[L.INFO["q1avg"]], rinfo["q1avg"]) and G.close(info[L.INFO["q2avg"]], rinfo["q2avg"])
    for e_g, e_p, share in res:
        assert e_g <= 1e-4 and share <= 0.25 and e_p <= 2e-5
    G.same(before, G.state([pi, la]))      # nothing reaches the actor (ignore_derivatives), and the critic step leaves CQL_log_alpha alone


@pytest.mark.parametrize("row", ALL, ids=IDS)
def test_critic_step_matches_float64(gpu_ctx, row):
    c, N = _case(row)
    for log_alpha in QR.log_alphas(c):
        _check_critic_step(gpu_ctx, c, N, log_alpha)


def test_weighted_and_beta_clamp_critic_steps(gpu_ctx):
    name, B, sc, N = QR.WEIGHTED_CASE; c = QR.case(name, B, sc)
    _check_critic_step(gpu_ctx, c, N, float(c["log_alpha"]), weighted=True)
    _check_critic_step(gpu_ctx, c, N, QR.BETA_CLAMP)


@pytest.mark.parametrize("row", ALL, ids=IDS)
def test_alpha_step_matches_float64(gpu_ctx, row):
    ctx = gpu_ctx; c, N = _case(row)
    for log_alpha in QR.log_alphas(c) + (QR.BETA_CLAMP,):
        pi, q1, q2, la = _nets(c, ctx, log_alpha); b = G.batch(c, ctx); x0 = float(la.get_params()[0])
        _, samp, lp = _conservative(ctx, pi, q1, q2, la, b, N, CTR + 1)
        rinfo, g, x1r = QR.alpha_step(c, samp, lp, x0, lr=LR)
        before = G.state([pi, q1, q2]); info = np.zeros(L.INFO_N, np.float32)
        ctx.check(ctx.lib.crux_cql_alpha_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, N, LO, HI, THRESH, SEED, CTR + 1, vp(info)))
        x1 = float(la.get_params()[0])
        print("alpha %s log alpha %+.3f:" % (row, log_alpha), info[[0, 1, L.INFO["alpha"]]], rinfo, g, x1, x1r)
        assert G.close(info[0], rinfo["loss"]) and G.close(info[1], rinfo["grad_norm"]) and G.close(info[L.INFO["alpha"]], rinfo["alpha"])
        if log_alpha > np.log(1e6):
            assert g == 0.0 and info[1] == 0.0 and x1 == x0
        else:
            assert abs(x1 - x1r) <= 2e-5
        G.same(before, G.state([pi, q1, q2]))


def test_two_identical_calls_give_identical_bits(gpu_ctx):
    ctx = gpu_ctx; name, B, sc, N = QR.CASES[4]; c = QR.case(name, B, sc); res = []
    for _ in range(2):
        pi, q1, q2, la = _nets(c, ctx, 0.0); b = G.batch(c, ctx)
        d_y = ctx.alloc(4 * B); ctx.h2d(d_y, QR.target(c)); i1, i2 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
        ctx.check(ctx.lib.crux_cql_critic_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, d_y, N, LO, HI, THRESH, 0, SEED, 5, vp(i1)))
        ctx.check(ctx.lib.crux_cql_alpha_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, N, LO, HI, THRESH, SEED, 6, vp(i2))); ctx.free(d_y)
        res.append((i1, i2, q1.get_params(), q2.get_params(), la.get_params()) + _conservative(ctx, pi, q1, q2, la, b, N, 7))
    for x, y in zip(*res):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("sc", [0.0, 2.0])
def test_nan_state_is_an_error_that_changes_nothing(gpu_ctx, sc):
    ctx = gpu_ctx; c = QR.case("5-100-100-2x3", 37, sc); N, B = 3, 37
    s = c["s"].copy(); s[2, 5] = np.nan
    pi, q1, q2, la = _nets(c, ctx, 0.0); b = G.batch(c, ctx, s=s)
    d_y = ctx.alloc(4 * B); ctx.h2d(d_y, QR.target(c)); before = G.state([pi, q1, q2, la]); info = np.zeros(L.INFO_N, np.float32)
    with pytest.raises(crux.CruxError) as e:
        ctx.check(ctx.lib.crux_cql_critic_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, d_y, N, LO, HI, THRESH, 0, SEED, 3, vp(info)))
    assert e.value.code == L.ENAN
    G.same(before, G.state([pi, q1, q2, la]))
    with pytest.raises(crux.CruxError) as e:
        ctx.check(ctx.lib.crux_cql_alpha_step_sigma(pi.h, q1.h, q2.h, la.h, b.h, N, LO, HI, THRESH, SEED, 4, vp(info)))
    assert e.value.code == L.ENAN
    G.same(before, G.state([pi, q1, q2, la])); ctx.free(d_y)
    for n in (q1, q2, la):
        assert np.allclose(n.adam_state()[2], [0.9, 0.999]) and not n.adam_state()[0].any() and not n.adam_state()[1].any()


def _solve_setup(ctx, n=96):
    od, ad, sc = 11, 3, 1.0; acts = ["relu", "relu", "identity"]
    A = G.policy([od, 64, 64, 2 * ad], acts, ad, sc, ctx, seed=13, stream=0)
    Q1 = crux.ContinuousNetwork(parity.chain([od + ad, 64, 64, 1], acts), seed=13, stream=1, ctx=ctx)
    Q2 = crux.ContinuousNetwork(parity.chain([od + ad, 64, 64, 1], acts), seed=13, stream=2, ctx=ctx)
    rng = np.random.default_rng(3)
    data = {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(-1, 1, (1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.1, "episode_end": np.zeros((1, n), bool)}
    D = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), n, ctx=ctx); D.push_(data)
    return crux.ActorCritic(A, crux.DoubleNetwork(Q1, Q2)), D, crux.ContinuousSpace(od)


def _manual(ctx, pi, D, S, epochs, B, gamma, N, noise_seed=0):
    """solve(::BatchSolver) from the step entry points with batch.py's counters 8g + {0 .. 4}: CQL alpha, SAC temperature, sac_target, critics, polyak, actor"""
    A, Q = pi.A, pi.C; lib = ctx.lib; pim = crux.clone_policy(pi)
    Dn = crux.normalize_(crux.copy_buffer(D), S, crux.ContinuousSpace(A.act_dim))
    sla = crux.ParamVector([np.log(np.float32(1.0))], ctx=ctx); cla = crux.ParamVector([np.log(np.float32(1.0))], ctx=ctx)
    for n in (A, Q.N1, Q.N2, sla, cla):
        n.attach_optimizer(crux.Adam(np.float32(3e-4)))
    mb = crux.buffer_like(Dn, capacity=B); d_y = ctx.alloc(4 * B); raw = np.zeros(L.INFO_N, np.float32); H, g, n = float(np.float32(-A.act_dim)), 0, len(Dn)
    for epoch in range(epochs + 1):
        crux.shuffle_device_(Dn, 0, epoch)
        for k0 in range(0, n, B):
            m = min(B, n - k0); mb.clear_(); mb.push_(Dn, ids=np.arange(k0 + 1, k0 + m + 1)); base = 8 * g
            ctx.check(lib.crux_cql_alpha_step_sigma(A.h, Q.N1.h, Q.N2.h, cla.h, mb.h, N, -1.0, 1.0, 10.0, noise_seed, base + 0, vp(raw)))
            ctx.check(lib.crux_sac_temp_step(A.h, sla.h, mb.h, H, noise_seed, base + 1, vp(raw)))
            ctx.check(lib.crux_sac_target(A.h, pim.C.N1.h, pim.C.N2.h, sla.h, mb.h, gamma, noise_seed, base + 2, d_y))
            ctx.check(lib.crux_cql_critic_step_sigma(A.h, Q.N1.h, Q.N2.h, cla.h, mb.h, d_y, N, -1.0, 1.0, 10.0, 0, noise_seed, base + 3, vp(raw)))
            crux.polyak_average_(pim, pi, np.float32(0.005))
            ctx.check(lib.crux_sac_actor_step(A.h, Q.N1.h, Q.N2.h, sla.h, mb.h, noise_seed, base + 4, vp(raw)))
            g += 1
    ctx.free(d_y)
    return g, pim, sla, cla


def test_solve_is_the_manual_composition(gpu_ctx):
    ctx, B, epochs, gamma, N = gpu_ctx, 32, 1, 0.99, 4
    pi1, D1, S = _solve_setup(ctx); pi2, D2, _ = _solve_setup(ctx)
    with pytest.raises(NotImplementedError, match=r"^CQL:.*two_headed=True"):
        crux.CQL(pi1, S, D1)
    sv = crux.CQL(pi1, S, D1, a_opt={"batch_size": B, "epochs": epochs}, gamma=gamma, CQL_n_action_samples=N, two_headed=True)
    assert sv.P["SAC_H_target"] == np.float32(-3.0)
    p0 = pi1.A.get_params().copy()
    crux.solve(sv)
    g, pim2, sla, cla = _manual(ctx, pi2, D2, S, epochs, B, gamma, N)
    assert len(sv.history) == epochs + 1 and sv.grad_steps == g == (epochs + 1) * 3
    for h in sv.history:
        for k in ("CQL alpha", "SAC alpha", "critic_loss", "actor_loss", "entropy"):
            assert k in h and np.isfinite(h[k]), (k, h)
    leaves1 = crux.api._leaves(pi1) + crux.api._leaves(sv.agent.pi_minus) + [sv.P["SAC_log_alpha"], sv.P["CQL_log_alpha"]]
    leaves2 = crux.api._leaves(pi2) + crux.api._leaves(pim2) + [sla, cla]
    for n1, n2 in zip(leaves1, leaves2):
        assert np.array_equal(n1.get_params().view(np.uint32), n2.get_params().view(np.uint32))
    assert not np.array_equal(pi1.A.get_params(), p0) and pi1.A.two_headed and sv.agent.pi_minus.A.two_headed


def test_refusals(gpu_ctx):
    ctx = gpu_ctx; c = QR.case("5-100-100-2x3", 37, 0.0); B = 37
    pi, q1, q2, la = _nets(c, ctx, 0.0); b = G.batch(c, ctx); out = np.zeros(4, np.float32); info = np.zeros(L.INFO_N, np.float32); d_y = ctx.alloc(4 * B)
    const = crux.GaussianPolicy(parity.chain([5, 100, 100, 3], list(c["acts"])), np.full(3, -0.3, np.float32), ctx=ctx)      # constant logSigma: the plain entries' actor
    wrong = G.policy([5, 16, 4], ["relu", "identity"], 2, 1.0, ctx)                                                          # two-headed, 2 x 2 rows against ad = 3
    for bad in (const, wrong):
        before = [n.get_params() for n in (bad, q1, q2, la)]
        assert ctx.lib.crux_cql_conservative_sigma(bad.h, q1.h, q2.h, la.h, b.h, 2, LO, HI, THRESH, 0, 0, vp(out), None, None) == L.EINVAL
        assert ctx.lib.crux_cql_alpha_step_sigma(bad.h, q1.h, q2.h, la.h, b.h, 2, LO, HI, THRESH, 0, 0, vp(info)) == L.EINVAL
        assert ctx.lib.crux_cql_critic_step_sigma(bad.h, q1.h, q2.h, la.h, b.h, d_y, 2, LO, HI, THRESH, 0, 0, 0, vp(info)) == L.EINVAL
        assert not out.any() and not info.any() and all(np.array_equal(x, n.get_params()) for x, n in zip(before, (bad, q1, q2, la)))
    # cql_check's ranges hold for the new entries too
    assert ctx.lib.crux_cql_conservative_sigma(pi.h, q1.h, q2.h, la.h, b.h, 0, LO, HI, THRESH, 0, 0, vp(out), None, None) == L.EINVAL
    assert ctx.lib.crux_cql_conservative_sigma(pi.h, q1.h, q2.h, la.h, b.h, 2, 1.0, 1.0, THRESH, 0, 0, vp(out), None, None) == L.EINVAL
    # the plain entry still refuses the two-headed handle by its flag
    assert ctx.lib.crux_cql_conservative(pi.h, q1.h, q2.h, la.h, b.h, 2, LO, HI, THRESH, 0, 0, vp(out), None, None) == L.EUNSUP
    ctx.free(d_y)
    ac = crux.ActorCritic(pi, crux.DoubleNetwork(q1, q2)); S = crux.ContinuousSpace(5)
    with pytest.raises(NotImplementedError, match=r"^CQL:.*two_headed=True"):
        crux.CQL(ac, S, b)
    # with a constant-logSigma actor the keyword changes nothing: the solver is built and dispatches to the plain entries
    sv = crux.CQL(crux.ActorCritic(const, crux.DoubleNetwork(q1, q2)), S, b, two_headed=True)
    assert not sv.agent.pi.A.two_headed
