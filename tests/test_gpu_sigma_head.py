"""GPU: two-headed Gaussian actors -- GaussianPolicy / SquashedGaussianPolicy whose logSigma is a network on mu's trunk (crux_mlp_set_sigma_head; csrc/sac.hip SigmaExploreOp,
SigmaLogpdfOp, SigmaActorGradOp; csrc/rollout.h rollout_head_sigma) -- against the float64 yardstick of tests/sigma_head_reference.py, and the chained SAC epochs, the generic
rollout / explore kernels and the host mirror against each other.

Tolerances are the project's own (tests/test_gpu_mixture.py, _ensemble, _advil): 1e-4 relative on forward values, loss and norms, 1e-4 of the gradient scale on gradients,
2e-5 absolute on parameters after one Adam step at lr 1e-3, where parameters whose float64 gradient lies within 1e-3 of the gradient scale of zero are left out (Adam's first
step is lr sign(g) there). At most a quarter of a handle may be left out: tests/test_sigma_head_reference.py asserts that on every step case with the yardstick alone, from
the normals of this file's comparison (the device's Philox draws restated on the host, SR.philox_normals), and this file asserts it again on the share it sees. The largest
share is 0.2288 (4-256-256-2x2, B = 257, ascale 1); the lone column of 4-256-256-2x2 leaves out 0.1980 (its hidden biases are 0.5 + |N(0, 0.3)|, SR.HIDDEN_BIAS_OF: with the
default biases over 0.32 of that relu handle sits next to a dead unit).

lp and y get a per-shape absolute tolerance by the MR.mixture_tolerance rule: four times the largest error of the float32 restatement against float64 over the shape's
B x ascale grid (the margin covers the tile GEMMs' other summation order and the device's exp / log / tanh). Stored actions for logpdf are drawn from the policy itself.
    shape             float32 error lp / y       tolerance lp / y         largest device error lp / y (MI355X, profiles/sigma_head_tests.txt)
    2-32-2x1          1.156e-06 / 2.932e-07      4.623e-06 / 1.173e-06    1.142e-06 / 3.54e-07
    5-100-100-2x3     2.952e-06 / 4.608e-07      1.181e-05 / 1.843e-06    1.841e-06 / 5.61e-07
    4-256-256-2x2     2.976e-06 / 5.144e-07      1.190e-05 / 2.057e-06    1.394e-06 / 3.54e-07
    17-256-256-2x6    5.506e-06 / 6.803e-07      2.202e-05 / 2.721e-06    2.857e-06 / 6.66e-07
(lp: the larger of exploration's logprob and logpdf of the stored actions.) Every test prints its figures before it asserts.

The executor's decision rule: adding SigmaExploreOp / SigmaActorGradOp to the op table gave no phase kernel scratch or spills (profiles/sigma_head_kernel_resources.txt), so
the ops are in the table and crux_sac_epoch / crux_sac_epochs record a two-headed actor on the generic plan; they are compared with the call-by-call sequence bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cql_reference as CR
import ensemble_reference as ER
import parity
import sigma_head_reference as SR
from parity import crux, L

pytestmark = pytest.mark.gpu
LR = 1e-3
SEED = SR.SEED


@functools.lru_cache(maxsize=None)
def _case(name, B, sc, clamp=None):
    return SR.case(name, B, sc, clamp)


def _policy(dims, acts, ad, sc, ctx, **kw):
    """the reference's idiom: base = [Dense...]; mu = Chain(base..., Dense(h, ad)); logSigma = Chain(base..., Dense(h, ad))"""
    base = [crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(dims) - 2)]
    mu, ls = crux.Chain(*base, crux.Dense(dims[-2], ad)), crux.Chain(*base, crux.Dense(dims[-2], ad))
    return crux.SquashedGaussianPolicy(mu, ls, sc, ctx=ctx, **kw) if sc > 0 else crux.GaussianPolicy(mu, ls, ctx=ctx, **kw)


def _actor(c, ctx):
    pi = _policy(c["dims"], c["acts"], c["ad"], c["ascale"], ctx); pi.set_params(c["p"]); return pi


def _qnet(c, key, ctx):
    q = crux.ContinuousNetwork(parity.chain(list(c["qdims"]), list(c["qacts"])), ctx=ctx); q.set_params(c[key]); return q


def _batch(c, ctx):
    B = c["B"]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), crux.ContinuousSpace(c["ad"]), B, ctx=ctx)
    b.push_({"s": c["s"], "a": c["a"], "sp": c["sp"], "r": c["r"].reshape(1, B), "done": c["done"].reshape(1, B), "episode_end": np.zeros((1, B), bool)})
    return b


def _normals(ctr, B, ad):
    """GaussExploreOp's draws: column j, row d = randn(Philox(seed, counter, stream = j ad + d, NOISE))"""
    return SR.philox_normals(ctr, B, ad)


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _grads(net, ctx):
    g = np.empty(net.n_params, np.float32); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


FWD = [(n, B) for n in SR.GRID_SHAPES for B in SR.BS] + [("17-256-256-2x6", 37)]


@pytest.mark.parametrize("name,B", FWD)
def test_exploration_logpdf_entropy_action(gpu_ctx, name, B):
    ctx = gpu_ctx; tlp, _ = SR.tolerance(name); worst = 0.0
    for sc in SR.ASCALES:
        c = _case(name, B, sc); pi = _actor(c, ctx); ad = c["ad"]; eps = _normals(7, B, ad)
        a, lp = pi.exploration(c["s"], SEED, 7); ra, rlp, _ = SR.explore(c, c["s"], eps)
        assert a.shape == (ad, B) and lp.shape == (1, B)
        e_a, e_lp = np.abs(a - ra).max(), np.abs(lp[0] - rlp).max()
        l2 = pi.logpdf(c["s"], c["a"]); e_l2 = np.abs(l2[0] - SR.logpdf(c, c["s"], c["a"])).max(); worst = max(worst, e_lp, e_l2)
        ent, rent = pi.entropy(c["s"]), SR.entropy(c, c["s"]); act = pi.action(c["s"])
        print("%s B=%d ascale=%g: a %.2e lp %.2e logpdf %.2e (tolerance %.2e) entropy %.2e action %.2e" % (name, B, sc, e_a, e_lp, e_l2, tlp, np.abs(ent - rent).max(),
                                                                                                            np.abs(act - SR.action(c, c["s"])).max()))
        assert e_a <= 1e-4 * max(1.0, np.abs(ra).max()) and e_lp <= tlp and e_l2 <= tlp
        assert np.shape(ent) == ((1, B) if sc > 0 else ()) and np.abs(ent - rent).max() <= 1e-4 * max(1.0, np.abs(rent).max())
        assert np.abs(act - SR.action(c, c["s"])).max() <= 1e-4 * max(1.0, sc)
        if sc > 0:
            assert np.abs(a).max() <= sc and np.abs(act).max() <= sc
    print("%s B=%d: largest device error of lp %.3e" % (name, B, worst))


@pytest.mark.parametrize("name", ["2-32-2x1", "5-100-100-2x3"])
def test_clamped_log_sigma(gpu_ctx, name):
    """logSigma head biases -6 / 0 / 3: below, inside and above the squashed head's clamp (-l itself stays unclamped); the Gaussian head does not clamp"""
    ctx = gpu_ctx
    for sc in (0.0, 2.0):
        for k in (0, 1, 2):
            c = _case(name, 37, sc, k); pi = _actor(c, ctx); eps = _normals(3, 37, c["ad"])
            a, lp = pi.exploration(c["s"], SEED, 3); ra, rlp, _ = SR.explore(c, c["s"], eps)
            print("%s ascale=%g clamp case %d: a %.2e lp %.2e" % (name, sc, k, np.abs(a - ra).max(), np.abs(lp[0] - rlp).max()))
            assert np.abs(a - ra).max() <= 1e-4 * max(1.0, np.abs(ra).max()) and np.abs(lp[0] - rlp).max() <= 1e-4 * max(1.0, np.abs(rlp).max())


@pytest.mark.parametrize("name,B", FWD)
def test_sac_target_and_temperature_step(gpu_ctx, name, B):
    ctx = gpu_ctx; _, ty = SR.tolerance(name)
    for sc in SR.ASCALES:
        c = _case(name, B, sc); pi, q1t, q2t, b = _actor(c, ctx), _qnet(c, "q1t", ctx), _qnet(c, "q2t", ctx), _batch(c, ctx); ad = c["ad"]
        la = crux.ParamVector([c["log_alpha"]], ctx=ctx); la.attach_optimizer(crux.Adam(np.float32(LR)))
        d_y = ctx.alloc(4 * B); y = np.empty(B, np.float32)
        ctx.check(ctx.lib.crux_sac_target(pi.h, q1t.h, q2t.h, la.h, b.h, float(c["gamma"]), SEED, 11, d_y)); ctx.d2h(d_y, y); ctx.free(d_y)
        ry = SR.sac_target(c, _normals(11, B, ad)); e_y = np.abs(y - ry).max()
        info = np.zeros(L.INFO_N, np.float32)
        ctx.check(ctx.lib.crux_sac_temp_step(pi.h, la.h, b.h, float(c["H"]), SEED, 12, info.ctypes.data_as(C.c_void_p)))
        rinfo, rla = SR.temp_step(c, _normals(12, B, ad))
        print("%s B=%d ascale=%g: y %.2e (tolerance %.2e) temp" % (name, B, sc, e_y, ty), info[[0, 1, L.INFO["alpha"]]], rinfo, float(la.get_params()[0]), rla)
        assert e_y <= ty
        assert _close(info[0], rinfo["loss"]) and _close(info[1], rinfo["grad_norm"]) and _close(info[L.INFO["alpha"]], rinfo["alpha"])
        assert abs(float(la.get_params()[0]) - rla) <= 2e-5


@pytest.mark.parametrize("name,B,sc", SR.STEP_CASES, ids=lambda v: str(v))
def test_actor_step_matches_float64(gpu_ctx, name, B, sc):
    """train!(actor, sac_actor_loss): loss, entropy, norm, the raw gradient (crux_mlp_grads_ptr) and the parameters after one Adam step"""
    ctx = gpu_ctx; c = _case(name, B, sc); pi, q1, q2, b = _actor(c, ctx), _qnet(c, "q1", ctx), _qnet(c, "q2", ctx), _batch(c, ctx)
    la = crux.ParamVector([c["log_alpha"]], ctx=ctx); pi.attach_optimizer(crux.Adam(np.float32(LR)))
    info = np.zeros(L.INFO_N, np.float32)
    ctx.check(ctx.lib.crux_sac_actor_step(pi.h, q1.h, q2.h, la.h, b.h, SEED, SR.ACTOR_CTR, info.ctypes.data_as(C.c_void_p)))
    rinfo, g, p = SR.actor_step(c, _normals(SR.ACTOR_CTR, B, c["ad"]), lr=LR); gg = _grads(pi, ctx); share = SR.skipped_share(g)
    e_g = np.abs(gg - g).max() / np.abs(g).max(); keep = np.abs(g) > 1e-3 * np.abs(g).max(); e_p = np.abs(pi.get_params() - p)[keep].max()
    print("%s B=%d ascale=%g:" % (name, B, sc), info[[0, 1, L.INFO["entropy"]]], rinfo, "gradient error / scale %.2e, parameters %.2e, left out %.4f" % (e_g, e_p, share))
    assert _close(info[0], rinfo["loss"]) and _close(info[L.INFO["entropy"]], rinfo["entropy"]) and _close(info[1], rinfo["grad_norm"])
    assert e_g <= 1e-4 and share <= 0.25 and e_p <= 2e-5


def _epoch_nets(name, sc, B, ctx):
    c = _case(name, B, sc); rng = np.random.default_rng(5); n = 1500
    S, A = crux.ContinuousSpace(c["od"]), crux.ContinuousSpace(c["ad"])
    buf = crux.ExperienceBuffer(S, A, n, ctx=ctx); D = crux.buffer_like(buf, capacity=B)
    buf.push_({"s": rng.normal(0, 1, (c["od"], n)).astype(np.float32), "a": rng.uniform(-1, 1, (c["ad"], n)).astype(np.float32), "sp": rng.normal(0, 1, (c["od"], n)).astype(np.float32),
               "r": rng.normal(-1, 1, (1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.05, "episode_end": np.zeros((1, n), bool)})
    nets = [_actor(c, ctx), _qnet(c, "q1", ctx), _qnet(c, "q2", ctx), _actor(c, ctx), _qnet(c, "q1t", ctx), _qnet(c, "q2t", ctx)]
    la = crux.ParamVector([c["log_alpha"]], ctx=ctx)
    for net in nets[:3] + [la]:
        net.attach_optimizer(crux.Adam(np.float32(3e-4)))
    return c, buf, D, nets, la


@pytest.mark.parametrize("every", [(1, 1), (1, 2), (2, 1)], ids=["c1a1", "c1a2", "c2a1"])
@pytest.mark.parametrize("name,sc,B", [("4-256-256-2x2", 2.0, 257), ("5-100-100-2x3", 0.0, 37), ("17-256-256-2x6", 1.0, 37)])
def test_sac_epochs_equal_the_call_by_call_sequence(gpu_ctx, name, sc, B, every):
    """crux_sac_epoch and crux_sac_epochs (3 epochs) with a two-headed actor == rand! -> sac_target -> temperature -> [critics] -> [actor -> polyak] call by call, bit for bit"""
    ctx = gpu_ctx; ce, ae = every; E, gamma, tau, H = 3, 0.99, 0.005, -float(SR.SHAPES[name][2])

    def run(mode):
        c, buf, D, nets, la = _epoch_nets(name, sc, B, ctx); a, q1, q2, at, t1, t2 = nets
        it, ic, ia = (np.zeros((E, L.INFO_N), np.float32) for _ in range(3)); vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
        if mode == "epochs":
            ctx.check(ctx.lib.crux_sac_epochs(a.h, q1.h, q2.h, at.h, t1.h, t2.h, la.h, buf.h, D.h, gamma, H, tau, 0, 0, E, ce, ae, 70, SEED, 210, vp(it), vp(ic), vp(ia)))
        for e in range(E if mode != "epochs" else 0):
            uc, ua = e % ce == 0, e % ae == 0
            if mode == "epoch":
                ctx.check(ctx.lib.crux_sac_epoch(a.h, q1.h, q2.h, at.h, t1.h, t2.h, la.h, buf.h, D.h, gamma, H, tau, 0, int(uc), int(ua), 70 + e, SEED, 210 + 3 * e, vp(it[e]), vp(ic[e]), vp(ia[e])))
                continue
            d_y = ctx.alloc(4 * B)
            crux.uniform_sample_(D, buf, B, i=70 + e)
            ctx.check(ctx.lib.crux_sac_target(a.h, t1.h, t2.h, la.h, D.h, gamma, SEED, 210 + 3 * e, d_y))
            ctx.check(ctx.lib.crux_sac_temp_step(a.h, la.h, D.h, H, SEED, 211 + 3 * e, vp(it[e])))
            if uc:
                ctx.check(ctx.lib.crux_double_q_step(q1.h, q2.h, D.h, d_y, 0, vp(ic[e])))
            if ua:
                ctx.check(ctx.lib.crux_sac_actor_step(a.h, q1.h, q2.h, la.h, D.h, SEED, 212 + 3 * e, vp(ia[e])))
                for t, f in ((at, a), (t1, q1), (t2, q2)):
                    ctx.check(ctx.lib.crux_polyak(t.h, f.h, tau))
            ctx.sync(); ctx.free(d_y)
        return [n_.get_params() for n_ in nets + [la]] + [it, ic[::ce], ia[::ae]]
    ref = run("calls")
    assert not np.array_equal(ref[0], _case(name, B, sc)["p"]) and np.isfinite(ref[0]).all()      # the actor moved
    for mode in ("epoch", "epochs"):
        for k, (x, y) in enumerate(zip(run(mode), ref)):
            assert np.array_equal(x, y), (mode, k, np.abs(x - y).max())


def _cfg(head, explore=True, i0=0, noise=None):
    cfg = parity.rollout_cfg(explore, True, head, i0)
    if noise:
        cfg.noise_sigma, cfg.noise_eps_min, cfg.noise_eps_max, cfg.a_min, cfg.a_max = noise
    return cfg


def _rollout_normals(seed, step, E, ad):
    """the rollout kernels' draws: row q of environment e at its step-th step = randn_f32(Philox(seed, step ceil(ad / 2) + q / 2, stream e, NOISE), q & 1): cos for even q, sin for odd"""
    out = np.empty((ad, E), np.float32)
    for q in range(ad):
        x = CR.philox(seed, step * ((ad + 1) // 2) + q // 2, np.arange(E), CR.RNG_NOISE); u1, u2 = CR.u53(x[0], x[1]), CR.u53(x[2], x[3])
        rr, th = np.sqrt(-2.0 * np.log(1.0 - u1)), 2.0 * np.pi * u2
        out[q] = (rr * np.sin(th) if q & 1 else rr * np.cos(th)).astype(np.float32)
    return out


ROLLOUTS = [("pendulum-64-relu-x2", "pendulum", 3, 1, [64, 64], "relu", 2.0),      # 3-64-64-2: an instantiated register-resident shape by its dims -- must take the generic kernel
            ("pendulum-256-relu-x2", "pendulum", 3, 1, [256, 256], "relu", 2.0),    # wide: k_rollout_wide, never k_rollout_res
            ("pendulum-32-tanh-gauss", "pendulum", 3, 1, [32], "tanh", 0.0),
            ("synth-17-6-64-tanh-x1", "synth", 17, 6, [64, 64], "tanh", 1.0),
            ("synth-17-6-256-relu-gauss", "synth", 17, 6, [256, 256], "relu", 0.0)]


@pytest.mark.parametrize("row", ROLLOUTS, ids=[r[0] for r in ROLLOUTS])
def test_rollout_equals_policy_explore_and_the_yardstick(gpu_ctx, row):
    """crux_rollout (generic kernels) on Pendulum and SYNTH(17, 6) against crux_policy_explore fed the stored :s rows and step counters, bit for bit on :a and :logprob; and
    crux_policy_explore against the yardstick from the kernels' own normals"""
    _, kind, od, ad, hidden, act, sc = row; ctx = gpu_ctx
    E, T, seed, i0 = 3, 5, 515, 40
    dims = [od] + hidden + [2 * ad]; acts = [act] * len(hidden) + ["identity"]
    pi = _policy(dims, acts, ad, sc, ctx, seed=13, stream=0)
    mdp = crux.PendulumMDP(n_envs=E, seed=seed) if kind == "pendulum" else crux.SynthMDP(od, ad, n_envs=E, seed=seed)
    buf = crux.ExperienceBuffer(mdp.state_space(), mdp.action_space(), E * T, ["logprob"])
    smp = crux.Sampler(mdp, pi, max_steps=100, required_columns=["logprob"])
    crux.steps_(smp, buf, Nsteps=E * T, explore=True, i=i0)
    S, A, LP = buf["s"], buf["a"], buf["logprob"]
    assert A.shape == (ad, E * T) and np.isfinite(LP).all() and (sc == 0 or np.abs(A).max() <= sc)
    c = {"dims": tuple(dims), "acts": tuple(acts), "ad": ad, "ascale": sc, "p": pi.get_params()}
    for t in range(T):
        rows = np.arange(E) * T + t
        a, lp = crux.policy_explore(pi, _cfg("gaussian", i0=i0 + t * E), S[:, rows], seed, np.full(E, t, np.int64))
        assert a.shape == (ad, E)
        assert np.array_equal(a, A[:, rows]), "step %d: actions differ" % t
        assert np.array_equal(lp.view(np.uint32), np.ascontiguousarray(LP[0, rows]).view(np.uint32)), "step %d: logprob differs" % t
        ra, rlp, _ = SR.explore(c, S[:, rows], _rollout_normals(seed, t, E, ad))
        assert np.abs(a - ra).max() <= 1e-4 * max(1.0, np.abs(ra).max()) and np.abs(lp - rlp).max() <= 1e-4 * max(1.0, np.abs(rlp).max()), (t, np.abs(a - ra).max(), np.abs(lp - rlp).max())
    # action(pi, s): explore = false
    g, glp = crux.policy_explore(pi, _cfg("gaussian", explore=False), S[:, :E], seed, np.zeros(E, np.int64))
    assert np.isnan(glp).all() and np.abs(g - SR.action(c, S[:, :E])).max() <= 1e-4 * max(1.0, sc)


def test_deterministic_head_with_noise_on_a_squashed_actor(gpu_ctx):
    """SAC's default pi_explore: action(pi_on, s) = ascale tanh(mu(s)), then the Gaussian noise and its clamps (policies.jl:372, 510-513)"""
    ctx, E, sc, seed = gpu_ctx, 64, 2.0, 99
    pi = _policy([3, 64, 64, 2], ["relu", "relu", "identity"], 1, sc, ctx, seed=4)
    p = pi.get_params(); p[-2] = 3.0; pi.set_params(p)      # mu's bias: tanh near 1, so that the noise would leave [-2, 2] without the clamp
    obs = np.asfortranarray(np.random.default_rng(1).normal(0, 1, (3, E)).astype(np.float32))
    c = {"dims": (3, 64, 64, 2), "acts": ("relu", "relu", "identity"), "ad": 1, "ascale": sc, "p": pi.get_params()}
    det, lp = crux.policy_explore(pi, _cfg("deterministic", explore=False), obs, seed, np.zeros(E, np.int64))
    assert np.isnan(lp).all() and np.abs(det - SR.action(c, obs)).max() <= 1e-4 * sc
    noisy, _ = crux.policy_explore(pi, _cfg("deterministic", noise=(0.5, -1.0, 1.0, -sc, sc)), obs, seed, np.full(E, 3, np.int64))
    n0 = np.clip(0.5 * _rollout_normals(seed, 3, E, 1), -1.0, 1.0); ref = np.clip(SR.action(c, obs) + n0, -sc, sc)
    assert noisy.min() >= -sc and noisy.max() <= sc and (noisy == sc).any() and not np.array_equal(noisy, det)
    assert np.abs(noisy - ref).max() <= 1e-4 * sc


def test_flux_params_clone_and_polyak(gpu_ctx):
    ctx = gpu_ctx
    pi = _policy([3, 16, 4], ["relu", "identity"], 2, 1.0, ctx, seed=3)
    ps = pi.params()
    assert len(ps) == 6 and [x.shape for x in ps] == [(16, 3), (16,), (2, 16), (2,), (2, 16), (2,)]      # policy_tests.jl:295: the shared trunk once
    flat = pi.get_params(); W = flat[64:128].reshape((4, 16), order="F")
    assert np.array_equal(ps[2], W[:2]) and np.array_equal(ps[4], W[2:]) and np.array_equal(ps[3], flat[128:130]) and np.array_equal(ps[5], flat[130:132])
    # each head drawn as a layer of its own: Glorot's bound with fan_out = ad, not 2 ad
    lim = np.sqrt(6.0 / (16 + 2)); assert np.abs(W).max() <= lim * (1 + 1e-6) and np.abs(W).max() > np.sqrt(6.0 / (16 + 4)) * 0.9
    pi.set_flux_params([x + 1 for x in ps]); assert np.array_equal(np.concatenate([x.reshape(-1, order="F") for x in pi.params()]), np.concatenate([(x + 1).reshape(-1, order="F") for x in ps]))
    pi.set_params(flat); assert np.array_equal(pi.get_params(), flat)
    cl = crux.clone_policy(pi)
    assert type(cl) is type(pi) and cl.two_headed and cl.act_dim == 2 and cl.ascale == 1.0 and np.array_equal(cl.get_params(), flat)
    assert ctx.lib.crux_mlp_get_sigma_head(cl.h) == 1 and ctx.lib.crux_mlp_get_sigma_head(pi.h) == 1
    pi.set_params(flat + 1.0); crux.polyak_average_(cl, pi, 0.25)
    assert np.allclose(cl.get_params(), flat + 0.25, atol=1e-6)
    assert crux.PolicyParams(pi).space.dims == crux.ContinuousSpace(2).dims


def test_nan_gate_leaves_the_parameters_untouched(gpu_ctx):
    ctx = gpu_ctx
    for sc in (0.0, 2.0):
        c = dict(_case("5-100-100-2x3", 37, sc)); s = c["s"].copy(); s[2, 5] = np.nan; c["s"] = s
        pi, q1, q2, b = _actor(c, ctx), _qnet(c, "q1", ctx), _qnet(c, "q2", ctx), _batch(c, ctx)
        la = crux.ParamVector([c["log_alpha"]], ctx=ctx); pi.attach_optimizer(crux.Adam(np.float32(LR))); before = pi.get_params()
        with pytest.raises(crux.CruxError) as e:
            ctx.check(ctx.lib.crux_sac_actor_step(pi.h, q1.h, q2.h, la.h, b.h, SEED, 13, None))
        assert e.value.code == L.ENAN
        assert np.array_equal(pi.get_params().view(np.uint32), before.view(np.uint32)) and np.allclose(pi.adam_state()[2], [0.9, 0.999])


def test_refusals(gpu_ctx):
    ctx = gpu_ctx; acts = ["relu", "identity"]
    with pytest.raises(NotImplementedError, match="separate trunks"):
        crux.GaussianPolicy(parity.chain([3, 16, 1], acts), parity.chain([3, 16, 1], acts), ctx=ctx)
    base = crux.Dense(3, 16, "relu")
    with pytest.raises(NotImplementedError, match="identity"):
        crux.SquashedGaussianPolicy(crux.Chain(base, crux.Dense(16, 1)), crux.Chain(base, crux.Dense(16, 1, "tanh")), 1.0, ctx=ctx)
    sn = crux.DenseSN(3, 16, "relu")
    with pytest.raises(NotImplementedError, match="DenseSN"):
        crux.GaussianPolicy(crux.Chain(sn, crux.Dense(16, 1)), crux.Chain(sn, crux.Dense(16, 1)), ctx=ctx)
    pi = _policy([3, 16, 2], acts, 1, 1.0, ctx)
    q = lambda: crux.ContinuousNetwork(parity.chain([4, 16, 1], acts), ctx=ctx)      # noqa: E731
    ac = crux.ActorCritic(pi, crux.DoubleNetwork(q(), q())); S = crux.ContinuousSpace(3)
    D = crux.ExperienceBuffer(S, crux.ContinuousSpace(1), 8, ctx=ctx)
    D.push_({"s": np.zeros((3, 8), np.float32), "a": np.zeros((1, 8), np.float32), "sp": np.zeros((3, 8), np.float32), "r": np.zeros((1, 8), np.float32),
             "done": np.zeros((1, 8), bool), "episode_end": np.zeros((1, 8), bool)})
    with pytest.raises(NotImplementedError, match="CQL"):
        crux.CQL(ac, S, D)
    # the C entries themselves (the Julia shim and any other caller reach them without the constructor): check_sac takes the handle for SAC, the CQL entries refuse it by the flag
    la0 = crux.ParamVector([0.0], ctx=ctx); q1, q2 = q(), q(); out = np.zeros(4, np.float32); info = np.zeros(L.INFO_N, np.float32); d_y = ctx.alloc(4 * 8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    for sc in (0.0, 1.0):
        two = _policy([3, 16, 2], acts, 1, sc, ctx); before = two.get_params()
        assert ctx.lib.crux_cql_conservative(two.h, q1.h, q2.h, la0.h, D.h, 2, -1.0, 1.0, 10.0, 0, 0, vp(out), None, None) == L.EUNSUP
        assert ctx.lib.crux_cql_alpha_step(two.h, q1.h, q2.h, la0.h, D.h, 2, -1.0, 1.0, 10.0, 0, 0, vp(info)) == L.EUNSUP
        assert ctx.lib.crux_cql_critic_step(two.h, q1.h, q2.h, la0.h, D.h, d_y, 2, -1.0, 1.0, 10.0, 0, 0, 0, vp(info)) == L.EUNSUP
        assert np.array_equal(two.get_params(), before) and not out.any() and not info.any()
    ctx.free(d_y)
    with pytest.raises(NotImplementedError, match="BC"):
        crux.BC(pi, S, D)
    for name, make in (("SQIL", lambda: crux.SQIL(ac, S, D)), ("OffPolicyGAIL", lambda: crux.OffPolicyGAIL(ac, S, D, crux.ContinuousNetwork(parity.chain([4, 16, 2], acts), ctx=ctx))),
                       ("AdRIL", lambda: crux.AdRIL(ac, S, D))):
        with pytest.raises(NotImplementedError, match=name):
            make()
    with pytest.raises(NotImplementedError, match="two-headed"):
        crux.PPO(crux.ActorCritic(pi, crux.ContinuousNetwork(parity.chain([3, 16, 1], acts), ctx=ctx)), S)
    with pytest.raises(NotImplementedError, match="two-headed"):
        crux.MixtureNetwork([_policy([3, 16, 2], acts, 1, 0.0, ctx), _policy([3, 16, 2], acts, 1, 0.0, ctx)], np.full(2, 0.5, np.float32), ctx=ctx)
    assert crux.SAC(ac, S, N=10).P["SAC_H_target"] == np.float32(-1.0)      # -ad, not -2 ad
    # a constant-logSigma squashed actor is still refused by the SAC entries
    sq = crux.SquashedGaussianPolicy(parity.chain([3, 16, 1], acts), np.zeros(1, np.float32), 1.0, ctx=ctx)
    la = crux.ParamVector([0.0], ctx=ctx); d_y = ctx.alloc(4 * 8); q1, q2 = q(), q()
    rc = ctx.lib.crux_sac_target(sq.h, q1.h, q2.h, la.h, D.h, 0.99, 1, 1, d_y); ctx.free(d_y)
    assert rc == L.EUNSUP
    # the setter's own checks: odd last width, extras
    odd = crux.ContinuousNetwork(parity.chain([3, 16, 3], acts), ctx=ctx)
    assert ctx.lib.crux_mlp_set_sigma_head(odd.h, 1) == L.EINVAL and ctx.lib.crux_mlp_get_sigma_head(odd.h) == 0
    ext = crux.GaussianPolicy(parity.chain([3, 16, 2], acts), np.zeros(2, np.float32), ctx=ctx)
    assert ctx.lib.crux_mlp_set_sigma_head(ext.h, 1) == L.EINVAL and ctx.lib.crux_mlp_get_sigma_head(ext.h) == 0
    # a two-headed handle whose rows do not match the batch
    wrong = _policy([3, 16, 4], acts, 2, 1.0, ctx); d_y = ctx.alloc(4 * 8)
    rc = ctx.lib.crux_sac_target(wrong.h, q1.h, q2.h, la.h, D.h, 0.99, 1, 1, d_y); ctx.free(d_y)
    assert rc == L.EINVAL


def test_sac_solve_on_pendulum(gpu_ctx):
    """SAC(...) with a squashed two-headed actor through solve: it runs, every info is finite, the temperature moved, stored actions lie in [-ascale, ascale]"""
    ctx, sc = gpu_ctx, 2.0
    acts = ["relu", "relu", "identity"]
    pi = crux.ActorCritic(_policy([3, 64, 64, 2], acts, 1, sc, ctx, seed=2),
                          crux.DoubleNetwork(crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=3, ctx=ctx), crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=4, ctx=ctx)))
    sv = crux.SAC(pi, crux.ContinuousSpace(3), N=500, dN=10, buffer_size=1000, buffer_init=100, max_steps=50, c_opt={"batch_size": 64}, a_opt={"batch_size": 64},
                  SAC_alpha_opt={"batch_size": 64}, pi_explore=crux.GaussianNoiseExplorationPolicy(0.3, a_min=-sc, a_max=sc))
    p0 = pi.A.get_params()
    crux.solve(sv, crux.PendulumMDP(n_envs=1, seed=8))
    assert sv.history and all(np.isfinite(v) for h in sv.history for v in h.values() if isinstance(v, float))
    alphas = [h["SAC alpha"] for h in sv.history if "SAC alpha" in h]
    assert alphas and abs(alphas[-1] - 1.0) > 1e-3
    a = sv.buffer["a"][:, :len(sv.buffer)]
    assert np.abs(a).max() <= sc and not np.array_equal(pi.A.get_params(), p0)
    assert np.array_equal(sv.agent.pi_minus.A.get_params().shape, p0.shape) and sv.agent.pi_minus.A.two_headed
