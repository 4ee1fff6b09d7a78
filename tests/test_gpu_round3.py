"""GPU parity added in round 3: the README example (BASELINE configs[0]) through the kernel bench.py times for it, against the oracle's solve loop;
function-valued seams of OffPolicySolver; teacher-forced windows of the off-policy learners at the C4 dimensions."""
import ctypes as C

import numpy as np
import pytest

import parity
from parity import L, O, crux

pytestmark = pytest.mark.gpu


def _oracle_readme_dqn(N, dN=4, B=128, cap=1000, init=200, seed_net=1, seed_env=0, max_steps=100):
    """The oracle's restatement of solve(::OffPolicySolver) (off_policy.jl:113-150, :66-111) for DQN on SimpleGridWorld at the README's shapes
    (the loop bench_offpolicy.c1_cpu times as the CPU baseline of configs[0])."""
    o = O.OMlp([2, 8, 4], ["relu", "identity"]).init_glorot(seed_net).adam_init(float(np.float32(3e-4)))      # TrainingParams default Adam(3f-4) (training.jl:3)
    ot = O.OMlp([2, 8, 4], ["relu", "identity"]).init_glorot(seed_net)
    ob = O.OBuffer(2, 4, L.ACTION_DISCRETE, cap); obt = O.OBuffer(2, 4, L.ACTION_DISCRETE, B)
    oe = O.OEnv("gridworld", 1, max_steps, 0.95, seed_env)
    cfg = parity.rollout_cfg(True, False, "greedy_q"); cfg.eps_start, cfg.eps_stop, cfg.eps_steps = 1.0, 0.1, N // 2
    y = np.empty(B, np.float32); info = np.zeros(L.INFO_N, np.float32); losses = []
    cfg.i0 = init; oe.rollout(o, cfg, ob, init)
    i = init
    while i <= N - dN:
        cfg.i0 = i; oe.rollout(o, cfg, ob, dN)
        ep_losses = []
        for ep in range(dN):
            O.chk(O.lib().orc_uniform_sample(obt.h, ob.h, B, None, i * dN + ep, crux.api.SAMPLE_SEED))
            O.chk(O.lib().orc_dqn_target(ot.h, obt.h, 0.95, O.vpz(y)))
            O.chk(O.lib().orc_td_step(o.h, obt.h, O.vpz(y), 0, O.vpz(info)))
            ep_losses.append(float(info[0]))
        O.chk(O.lib().orc_polyak(ot.h, o.h, 0.005))
        losses.append(float(np.mean(ep_losses)))
        i += dN
    return o, ot, ob, obt, losses, i


def test_readme_dqn_gridworld_tiny_solve_kernel_matches_the_oracle_loop(gpu_ctx):
    """BASELINE configs[0] at the README's shapes (one environment, B = 128, ring of 1000, 2-8-4 relu network, dN = 4, eps 1 -> 0.1 over N/2) for 320
    iterations of solve: crux.solve takes the wave-resident k_dqn_tiny_solve<2,8,4> -- the kernel bench.py times for this config (asserted through its
    profiling slot) -- and must follow the ORACLE's loop: the same trajectories into the same ring slots (bit-exact), the same last staging batch, and the
    networks within a float tolerance after 1 280 Adam steps (the minibatch gradient is summed in another order than the oracle's scalar loop)."""
    N = 200 + 4 * 320
    S = crux.ContinuousSpace(2)
    q = crux.DiscreteNetwork(parity.chain([2, 8, 4], ["relu", "identity"]), [1, 2, 3, 4], seed=1)
    sv = crux.DQN(q, S, N=N, dN=4, max_steps=100, c_opt={"batch_size": 128})
    ctx = q.ctx
    ctx.prof_enable(True); ctx.prof_reset()
    crux.solve(sv, crux.SimpleGridWorld(n_envs=1, seed=0))
    ms, n_tiny = ctx.prof_get("tiny_solve"); _, n_other = ctx.prof_get("td_step")
    ctx.prof_enable(False)
    assert n_tiny >= 1 and n_other == 0, (n_tiny, n_other)            # the timed kernel of configs[0] ran, and nothing else trained
    o, ot, ob, obt, losses, i_end = _oracle_readme_dqn(N)
    assert sv.i == i_end and len(sv.buffer) == len(ob) == 1000 and len(sv.history) == len(losses) == 320
    for k in ("s", "a", "sp", "r", "done"):
        assert np.array_equal(sv.buffer[k], ob[k]), k                                         # eps-greedy trajectories incl. every greedy argmax, ring wrap
    assert np.array_equal(sv.batch["s"], obt["s"]) and np.array_equal(sv.batch["r"], obt["r"])          # the last uniform sample and its gather
    dq, dt = np.abs(q.get_params() - o.params).max(), np.abs(sv.agent.pi_minus.get_params() - ot.params).max()
    print("README DQN, 320 iterations: max |dtheta| %.3g (Q) %.3g (target)" % (dq, dt))
    assert dq < 1e-6 and dt < 1e-6, (dq, dt)          # measured 7.1e-8 / 6.0e-8 (profiles/r03_parity_measurements.txt)
    gl = np.array([h["critic_loss"] for h in sv.history]); ol = np.array(losses)
    assert np.abs(gl - ol).max() < 1e-4 * max(1.0, np.abs(ol).max())


# ---------------------------------------------------------------------------------------------------- teacher-forced windows of the off-policy learners (C4 dims)
def _replay_source(rng, od, ad, n):
    data = {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-2, 2, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(-1, 1, (1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.02, "episode_end": np.zeros((1, n), bool)}
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), n); gb.push_(data)
    ob = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, n); ob.push(data)
    return gb, ob


def _inject(pairs):
    """the oracle's parameters and Adam state (m, v, beta powers) of this moment into the GPU twins"""
    for g, o, trained in pairs:
        g.set_params(o.params.copy())
        if trained:
            g.set_adam_state(*o.adam_state())


# 10 x the largest measured window difference (profiles/r03_parity_measurements.txt): windows that start inside Adam's first steps (v ~ 0: lr m / (sqrt(v) + eps)
# amplifies a last-bit difference of the gradient) measured 2.5e-7 ... 7.6e-7, windows further along the trajectory 1.5e-8 ... 2.5e-7
OFFPOLICY_WINDOW_TOL = {0: 8e-6, "later": 2.5e-6}


@pytest.mark.parametrize("algo", ["sac", "ddpg", "td3"])
def test_offpolicy_teacher_forced_windows_at_c4_dims(gpu_ctx, algo):
    """BASELINE configs[3] dimensions (actor 3-256-256-1, critics 4-256-256-1, B = 256, Adam 3e-4 / 1e-3, polyak 0.005): the oracle runs 208 value_training epochs
    (off_policy.jl:69-104) from a 5 000-row ring; at epochs 0, 64, 128 and 200 the GPU networks get the oracle's exact state of that moment (parameters, Adam moments and
    beta powers, target networks, log alpha) and replay the next 8 epochs through the product path (crux_sac_epochs / crux_dpg_epochs: the chained executor epochs that
    solve() and bench.py run). The learner map is chaotic over hundreds of steps (relu kinks, Adam's normalisation), so this -- not the first steps from zero moments --
    is what pins the arithmetic of the off-policy dense engine along a trajectory."""
    ctx, rng = gpu_ctx, np.random.default_rng(17)
    B, n, od, ad, nseed, gamma, tau = 256, 5000, 3, 1, 9, 0.99, 0.005
    starts, W, total = (0, 64, 128, 200), 8, 208
    gbuf, obuf = _replay_source(rng, od, ad, n)
    D = crux.buffer_like(gbuf, capacity=B); oD = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, B)
    acts = ["relu", "relu", "identity"]; adims, qdims = [3, 256, 256, 1], [4, 256, 256, 1]
    sac, twin = algo == "sac", algo in ("sac", "td3")
    if sac:
        ga, oa = parity.make_pair(adims, acts, 5, 0, "gaussian", n_extra=1, extra_init=0.0)
    else:
        ga, oa = parity.make_pair(adims, ["relu", "relu", "tanh"], 5, 0)
    g1, o1 = parity.make_pair(qdims, acts, 5, 1); g2, o2 = parity.make_pair(qdims, acts, 5, 2)
    g1t, o1t = parity.make_pair(qdims, acts, 5, 1); g2t, o2t = parity.make_pair(qdims, acts, 5, 2)
    gat, oat = (None, None) if sac else parity.make_pair(adims, ["relu", "relu", "tanh"], 5, 0)
    gla = crux.ParamVector([0.0], ctx=ctx); ola = O.OMlp([0], [], 1); ola.params[:] = 0.0
    lr = float(np.float32(3e-4 if sac else 1e-3))
    trained = [(ga, oa), (g1, o1)] + ([(g2, o2)] if twin else []) + ([(gla, ola)] if sac else [])
    for g, o in trained:
        g.attach_optimizer(crux.Adam(np.float32(lr))); o.adam_init(lr)
    targets = [(g1t, o1t)] + ([(g2t, o2t)] if twin else []) + ([] if sac else [(gat, oat)])
    pairs = [(g, o, True) for g, o in trained] + [(g, o, False) for g, o in targets]
    sm = (np.float32(0.1), -0.5, 0.5, -1.0, 1.0) if algo == "td3" else (-1.0, 0.0, 0.0, 0.0, 0.0)
    ol, y, info = O.lib(), np.empty(B, np.float32), np.zeros(L.INFO_N, np.float32)
    pending, out = {}, []
    for e in range(total):
        if e in starts:
            _inject(pairs)
            if sac:
                ctx.check(ctx.lib.crux_sac_epochs(ga.h, g1.h, g2.h, None, g1t.h, g2t.h, gla.h, gbuf.h, D.h, gamma, -1.0, tau, 0, 0, W, 1, 1, e, nseed, 3 * e, None, None, None))
            else:
                ctx.check(ctx.lib.crux_dpg_epochs(ga.h, g1.h, g2.h if twin else None, gat.h, g1t.h, g2t.h if twin else None, gbuf.h, D.h, gamma, tau, *[float(x) for x in sm], 0, 0, W,
                                                  1, 2 if algo == "td3" else 1, e, nseed, e, None, None))
            pending[e + W] = [g.get_params() for g, _, _ in pairs]
        O.chk(ol.orc_uniform_sample(oD.h, obuf.h, B, None, e, crux.api.SAMPLE_SEED))
        if sac:
            O.chk(ol.orc_sac_target(oa.h, o1t.h, o2t.h, ola.h, oD.h, gamma, nseed, 3 * e, O.vpz(y)))
            O.chk(ol.orc_sac_temp_step(oa.h, ola.h, oD.h, -1.0, nseed, 3 * e + 1, O.vpz(info)))
            O.chk(ol.orc_double_q_step(o1.h, o2.h, oD.h, O.vpz(y), 0, O.vpz(info)))
            O.chk(ol.orc_sac_actor_step(oa.h, o1.h, o2.h, ola.h, oD.h, nseed, 3 * e + 2, O.vpz(info)))
            for t, s in ((o1t, o1), (o2t, o2)):
                O.chk(ol.orc_polyak(t.h, s.h, tau))
        else:
            O.chk(ol.orc_dpg_target(oat.h, o1t.h, o2t.h if algo == "td3" else None, oD.h, gamma, *sm, nseed, e, O.vpz(y)))
            if twin:
                O.chk(ol.orc_double_q_step(o1.h, o2.h, oD.h, O.vpz(y), 0, O.vpz(info)))
            else:
                O.chk(ol.orc_q_step(o1.h, oD.h, O.vpz(y), 0, O.vpz(info)))
            if algo != "td3" or e % 2 == 0:          # TD3's delayed policy update (a_opt.update_every = 2): actor step and target update together (off_policy.jl:96-100)
                O.chk(ol.orc_dpg_actor_step(oa.h, o1.h, oD.h, O.vpz(info)))
                for t, s in ((oat, oa), (o1t, o1)) + (((o2t, o2),) if twin else ()):
                    O.chk(ol.orc_polyak(t.h, s.h, tau))
        if e + 1 in pending:
            gp = pending.pop(e + 1)
            out.append((e + 1 - W, [float(np.abs(x - o.params).max()) for x, (_, o, _) in zip(gp, pairs)]))
    print("off-policy windows %s (start, max |dtheta| per network): %s" % (algo, out))
    assert len(out) == len(starts)
    for st, d in out:
        assert max(d) < OFFPOLICY_WINDOW_TOL[0 if st == 0 else "later"], (st, d)


# ---------------------------------------------------------------------------------------------------- function-valued seams of OffPolicySolver (off_policy.jl:53-63)
def test_offpolicy_user_target_two_sources_and_callbacks_match_the_oracle_loop(gpu_ctx):
    """solve(::OffPolicySolver) with the reference's function-valued fields set by the caller: target_fn (a double-DQN target evaluated by user code from pi and pi_minus),
    target_update (polyak with the caller's tau), extra_buffers + buffer_fractions (rand! over two sources, 3/4 + 1/4 of the minibatch), and the three callbacks. The
    solver leaves the fused chains for the call-by-call loop; the ORACLE's loop with the same user functions must give the same ring, the same staging batch and the same
    networks."""
    E, dN, B, N, cap, seed, max_steps = 1, 4, 32, 72, 96, 4, 20
    dims, acts = [2, 16, 4], ["relu", "identity"]
    g, o = parity.make_pair(dims, acts, 43, 0, "discrete", outputs=[1, 2, 3, 4])
    S, A = crux.ContinuousSpace(2), crux.DiscreteSpace(4)
    rng = np.random.default_rng(6); nx = 50
    ax = np.zeros((4, nx), bool); ax[rng.integers(0, 4, nx), np.arange(nx)] = True
    xdata = {"s": rng.integers(1, 11, (2, nx)).astype(np.float32), "a": ax, "sp": rng.integers(1, 11, (2, nx)).astype(np.float32), "r": rng.normal(0, 1, (1, nx)).astype(np.float32),
             "done": rng.random((1, nx)) < 0.1, "episode_end": np.zeros((1, nx), bool)}
    gx = crux.ExperienceBuffer(S, A, nx); gx.push_(xdata)
    ox = O.OBuffer(2, 4, L.ACTION_DISCRETE, nx); ox.push(xdata)
    calls = {"sample": 0, "batch": 0, "pre": 0, "rows": 0}

    def ddqn_target(fwd_online, fwd_target, D, gamma):
        sp, r, done = D["sp"], D["r"][0], D["done"][0]
        qo, qt = fwd_online(sp), fwd_target(sp)
        return (r + np.float32(gamma) * (1.0 - done.astype(np.float32)) * qt[np.argmax(qo, axis=0), np.arange(sp.shape[1])]).astype(np.float32)

    def target_fn(pim, P, D, gamma, i=0):
        return ddqn_target(g.forward, pim.forward, D, gamma)

    def target_update(pim, pi, i=None):
        crux.polyak_average_(pim, pi, 0.02)

    def post_sample(D, S=None, info=None):
        calls["sample"] += 1; calls["rows"] += D["s"].shape[1]; info["seen"] = 1.0

    def post_batch(D, S=None, info=None):
        calls["batch"] += 1; info["batch_r"] = float(D["r"].mean())

    def pre_train(S, info=None):
        calls["pre"] += 1

    sv = crux.DQN(g, S, N=N, dN=dN, c_opt={"batch_size": B, "optimizer": crux.Adam(np.float32(1e-3))}, buffer_size=cap, buffer_init=B, max_steps=max_steps,
                  target_fn=target_fn, target_update=target_update, extra_buffers=[gx], buffer_fractions=[0.75, 0.25],
                  post_sample_callback=post_sample, post_batch_callback=post_batch, pre_train_callback=pre_train)
    assert sv.custom_seams()
    crux.solve(sv, crux.SimpleGridWorld(n_envs=E, seed=seed))
    n_it = (N - B) // dN + 1 - 0
    # ---- the same loop on the oracle
    ot = O.OMlp(dims, acts); O.chk(O.lib().orc_mlp_copy(ot.h, o.h)); o.adam_init(float(np.float32(1e-3)))
    ob = O.OBuffer(2, 4, L.ACTION_DISCRETE, cap); obt = O.OBuffer(2, 4, L.ACTION_DISCRETE, B)
    oe = O.OEnv("gridworld", E, max_steps, 0.95, seed)
    cfg = parity.rollout_cfg(True, False, "greedy_q"); cfg.eps_start, cfg.eps_stop, cfg.eps_steps = 1.0, 0.1, N // 2
    O.chk(O.lib().orc_buffer_set_sample_stream(ob.h, 0)); O.chk(O.lib().orc_buffer_set_sample_stream(ox.h, 1))
    i = B; cfg.i0 = i; oe.rollout(o, cfg, ob, B)
    info = np.zeros(L.INFO_N, np.float32); its = 0
    while i <= N - dN:
        cfg.i0 = i; oe.rollout(o, cfg, ob, dN)
        for ep in range(dN):
            ctr = i * dN + ep
            O.chk(O.lib().orc_uniform_sample(obt.h, ob.h, 24, None, ctr, crux.api.SAMPLE_SEED)); O.chk(O.lib().orc_uniform_sample(obt.h, ox.h, 8, None, ctr, crux.api.SAMPLE_SEED))
            y = ddqn_target(o.forward, ot.forward, obt, 0.95)
            O.chk(O.lib().orc_td_step(o.h, obt.h, O.vpz(y), 0, O.vpz(info)))
        O.chk(O.lib().orc_polyak(ot.h, o.h, 0.02))
        i += dN; its += 1
    assert sv.i == i and len(sv.history) == its
    assert calls["pre"] == its and calls["batch"] == its * dN and calls["sample"] == its + 1 and calls["rows"] == B + its * dN
    assert "batch_r" in sv.history[-1] and sv.history[-1]["seen"] == 1.0                      # callback infos reach the iteration's info like log(...) gets them (:146)
    for k in ("s", "a", "sp", "r", "done"):
        assert np.array_equal(sv.buffer[k], ob[k]), k
        assert np.array_equal(sv.batch[k], obt[k]), k                                        # 24 rows of the ring + 8 of the extra buffer, in that order
    dq, dt = np.abs(g.get_params() - o.params).max(), np.abs(sv.agent.pi_minus.get_params() - ot.params).max()
    print("user-target DQN over two sources: max |dtheta| %.3g / %.3g" % (dq, dt))
    assert dq < 2e-6 and dt < 2e-6, (dq, dt)


def test_offpolicy_user_priority_fn_and_sample_callback_write_back(gpu_ctx):
    """priority_fn (off_policy.jl:60,83) supplied by the caller on a prioritized ring, and a post_sample_callback that relabels rewards in place (the GAIL-style use of
    the callback, :50): priorities, relabelled rewards and networks against the oracle's loop."""
    E, dN, B, N, cap, seed, max_steps = 1, 4, 16, 40, 64, 9, 20
    dims, acts = [2, 8, 4], ["relu", "identity"]
    g, o = parity.make_pair(dims, acts, 47, 0, "discrete", outputs=[1, 2, 3, 4])
    S = crux.ContinuousSpace(2)

    def prio(fwd, D, y):
        q = fwd(D["s"]); qa = (q * D["a"]).sum(axis=0)
        return (np.abs(qa - y) + np.float32(0.5)).astype(np.float32)

    def relabel(D, S=None, info=None):
        D["r"][...] = D["r"] * np.float32(0.5) - np.float32(0.25)

    sv = crux.DQN(g, S, N=N, dN=dN, c_opt={"batch_size": B, "optimizer": crux.Adam(np.float32(1e-3))}, buffer_size=cap, buffer_init=B, max_steps=max_steps, prioritized=True,
                  priority_fn=lambda pi, P, D, y: prio(pi.forward, D, y), post_sample_callback=relabel)
    crux.solve(sv, crux.SimpleGridWorld(n_envs=E, seed=seed))
    ot = O.OMlp(dims, acts); O.chk(O.lib().orc_mlp_copy(ot.h, o.h)); o.adam_init(float(np.float32(1e-3)))
    ob = O.OBuffer(2, 4, L.ACTION_DISCRETE, cap, ["weight"], prioritized=True, alpha=np.float32(0.6)); obt = O.OBuffer(2, 4, L.ACTION_DISCRETE, B, ["weight"], prioritized=True, alpha=np.float32(0.6))
    oe = O.OEnv("gridworld", E, max_steps, 0.95, seed)
    cfg = parity.rollout_cfg(True, False, "greedy_q"); cfg.eps_start, cfg.eps_stop, cfg.eps_steps = 1.0, 0.1, N // 2
    y, ids, info = np.empty(B, np.float32), np.empty(B, np.int64), np.zeros(L.INFO_N, np.float32)

    def orelabel(n):
        last = np.empty(n, np.int64); k = O.lib().orc_buffer_last_n_indices(ob.h, n, O.vpz(last)); assert k == n
        r = ob.col("r"); r[0, last] = r[0, last] * np.float32(0.5) - np.float32(0.25)

    i = B; cfg.i0 = i; oe.rollout(o, cfg, ob, B); orelabel(B)
    while i <= N - dN:
        cfg.i0 = i; oe.rollout(o, cfg, ob, dN); orelabel(dN)
        for ep in range(dN):
            O.chk(O.lib().orc_per_sample(obt.h, ob.h, B, None, 0.5, i * dN + ep, crux.api.SAMPLE_SEED))
            O.chk(O.lib().orc_dqn_target(ot.h, obt.h, 0.95, O.vpz(y)))
            O.chk(O.lib().orc_buffer_indices(obt.h, O.vpz(ids), B))
            v = prio(o.forward, obt, y)
            O.chk(O.lib().orc_per_update(ob.h, O.vpz(ids), O.vpz(v), 0, B))
            O.chk(O.lib().orc_td_step(o.h, obt.h, O.vpz(y), 0, O.vpz(info)))
        O.chk(O.lib().orc_polyak(ot.h, o.h, 0.005))
        i += dN
    assert np.array_equal(sv.buffer["s"], ob["s"]) and np.abs(sv.buffer["r"] - ob["r"]).max() == 0.0
    pg = sv.buffer.priority_params(); pr = np.empty(cap, np.float32); mx, mn = C.c_float(), C.c_float()
    O.chk(O.lib().orc_per_get(ob.h, O.vpz(pr), C.byref(mx), C.byref(mn), None))
    assert np.allclose(pg["priorities"], pr, rtol=2e-5, atol=1e-6) and abs(pg["max_priority"] - mx.value) < 1e-5
    assert np.abs(g.get_params() - o.params).max() < 2e-6


# ---------------------------------------------------------------------------------------------------- the feature-split learner kernel (train_fs2_kernel.h)
@pytest.mark.parametrize("family", ["cartpole", "synth_c5"])
def test_feature_split_learner_matches_the_oracle(gpu_ctx, capfd, family):
    """k_train_fs2 (four compute units x (four compute + four helper waves)) through a whole PPO iteration -- rollout, GAE, whiten, actor || critic batch_train! of 2 epochs x 8
    minibatches of 128 -- against the oracle: the same bounds as the sample-split kernel's (tests/parity.py), whatever the decomposition of a step."""
    res = parity.ppo_iteration_parity(n_envs=8, T=128, batch_size=128, epochs=2, seed=21, family=family, pair=True)
    assert res["ok"], res
    assert "outside the MFMA learner family" not in capfd.readouterr().err


def test_two_input_pendulum_shape_runs_on_the_feature_split_learner(gpu_ctx, capfd):
    """2->64->64->1 Gaussian actor + critic (the reference's own Pendulum networks, examples/rl/pendulum.jl): an instantiation of the feature-split kernel."""
    res = parity.ppo_iteration_parity(n_envs=8, T=128, batch_size=128, epochs=2, seed=5, family="synth_2_1", pair=True)
    assert res["ok"], res
    assert "outside the MFMA learner family" not in capfd.readouterr().err


def test_reference_half_cheetah_ppo_networks_run_on_the_feature_split_learner(gpu_ctx, capfd):
    """The networks of the reference's own HalfCheetah PPO example (examples/rl/half_cheetah_mujoco.jl:33-38): mu = 17 -tanh-> 64 -tanh-> 32 -> 6 with a trainable logSigma,
    V = 17 -tanh-> 64 -> 32 -> 1 (no activation on its second layer). A 32-wide second hidden layer and per-layer activations are instantiations of k_train_fs2 (a wave's half of
    the layer is one 16-feature tile); a whole PPO iteration against the oracle."""
    res = parity.ppo_iteration_parity(n_envs=8, T=128, batch_size=128, epochs=2, seed=9, family="cheetah_ref", pair=True)
    assert res["ok"], res
    err = capfd.readouterr().err
    assert "outside the MFMA learner family" not in err and "generic" not in err


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cartpole", "synth17"])
def test_lagrange_two_cu_form_still_matches_the_oracle(gpu_ctx, monkeypatch, kind):
    """lagrange_ppo_loss with full minibatches runs on the feature-split kernel's LAG instantiation by default (tests/test_gpu_lagrange.py, bs = 128); with CRUX_FS=0 the same
    call takes the two-CU kernel's (train_mfma_kernel.h) -- both against the oracle, same bounds."""
    import test_gpu_lagrange as TL
    monkeypatch.setenv("CRUX_FS", "0")
    TL.test_lagrange_batch_train_matches_oracle(gpu_ctx, kind, 128)


@pytest.mark.gpu
def test_asynchronous_solve_loop_equals_the_synchronous_one(gpu_ctx):
    """solve(::OffPolicySolver) for a wide DQN enqueues every iteration's chain without waiting for it (crux_dqn_value_training_async: no read-back, the info rows stay in a device
    ring until `history` is read) -- VERDICT r2 #5, "the host out of the solve loop". Same ring, priorities, networks and per-iteration infos as the loop that synchronises
    after every value_training call, bit for bit; the ring is still filling for the first iterations (chains cut at plain tree rebuilds) and full afterwards."""
    def run(asyn):
        S = crux.ContinuousSpace(8)
        q = crux.DiscreteNetwork(parity.chain([8, 256, 256, 4], ["relu", "relu", "identity"]), [1, 2, 3, 4], seed=3)
        mdp = crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=5, discount=0.97)
        sv = crux.DQN(q, S, N=1200, dN=4, buffer_size=1000, prioritized=True, weighted_loss=True, buffer_init=400, max_steps=40, c_opt={"batch_size": 128})
        sv.async_training = asyn
        crux.solve(sv, mdp)
        assert (len(sv._pending) == 0) and all(h is not None for h in sv._history)
        return q.get_params(), sv.agent.pi_minus.get_params(), sv.buffer["s"], sv.buffer.priority_params()["priorities"], np.array([[h["critic_loss"], h["critic_grad_norm"], h["Qavg"]] for h in sv.history])
    a, b = run(True), run(False)
    assert len(a[4]) == len(b[4]) >= 150
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_asynchronous_softq_solve_loop_equals_the_synchronous_one(gpu_ctx):
    """the same for SoftQ (rl/softq.jl:31-58): the asynchronous loop goes through crux_dqn_value_training_async with softq_alpha > 0 -- softq_target in the chain and the target
    update of off_policy.jl:108 riding in its last phase (round 6) -- the synchronous one through crux_softq_epochs followed by a stand-alone polyak_average!: same ring, same
    networks, same target networks and infos, bit for bit."""
    def run(asyn):
        S = crux.ContinuousSpace(8)
        q = crux.DiscreteNetwork(parity.chain([8, 128, 128, 4], ["relu", "relu", "identity"]), [1, 2, 3, 4], seed=4)
        mdp = crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=6, discount=0.97)
        sv = crux.SoftQ(q, S, N=700, dN=4, buffer_size=512, buffer_init=300, max_steps=40, alpha=0.5, c_opt={"batch_size": 128})
        sv.async_training = asyn
        crux.solve(sv, mdp)
        assert (len(sv._pending) == 0) and all(h is not None for h in sv._history)
        if asyn:
            assert getattr(sv, "_async_unsupported", False) is False          # it really took the asynchronous chains
        return q.get_params(), sv.agent.pi_minus.get_params(), sv.buffer["s"], np.array([[h["critic_loss"], h["critic_grad_norm"], h["Qavg"]] for h in sv.history])
    a, b = run(True), run(False)
    assert len(a[3]) == len(b[3]) >= 90
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cartpole", "synth17"])
def test_lagrange_loss_on_the_feature_split_kernel_at_rollout_size(gpu_ctx, kind):
    """lagrange_ppo_loss inside k_train_fs2<..., LAG> on a 16 x 1024 rollout, minibatches of 128: 128 (relu CartPole actor, one epoch) / 256 (tanh 17-64-64-6 actor, two
    epochs) consecutive minibatch steps, every one advancing the PID controller on its own cost statistics, free-running against the oracle (tests/test_gpu_lagrange.py
    checks 18 steps on a 384-row buffer). The relu actor stays at one epoch: measured 2.2e-6 after 128 steps and 2.5e-3 after 256 -- a free-running relu learner leaves the
    oracle's trajectory once a unit flips at its kink (the two-CU kernel shows the same 2.5e-3, the two kernels agree to 6e-8; DESIGN 6: why the long runs are pinned with
    teacher-forced windows instead)."""
    import test_gpu_lagrange as TL
    (gb, ob), (ga, oa), _, _, head = TL._pair(kind, E=16, T=1024, max_steps=12, seed=33)      # (short episodes: every minibatch holds episode ends -- one without any is a NaN step, as in the reference)
    O.chk(O.lib().orc_whiten(ob.h, L.COL["advantage"])); crux.whiten_(gb, "advantage")
    N, epochs, bs = len(gb), (1 if kind == "cartpole" else 2), 128
    rng = np.random.default_rng(9); perms = np.stack([rng.permutation(N) for _ in range(epochs)])
    glag = TL._lag(); olag = TL._copy_lag(glag)
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1, "lagrange": glag}
    info = crux.batch_train_(ga, crux.TrainingParams(loss=crux.lagrange_ppo_loss, batch_size=bs, epochs=epochs, name="actor_"), P, gb, perms=perms + 1)
    oa.adam_init(float(np.float32(3e-4)))
    cfg = parity.train_cfg("lagrange_ppo", head, bs, epochs, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32); oe_ = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train_lagrange(oa.h, ob.h, C.byref(cfg), C.byref(olag), O.vpz(np.ascontiguousarray(perms, np.int64)), O.vpz(oi), O.vpz(oe_)))
    steps = epochs * (N // bs); d = float(np.abs(ga.get_params() - oa.params).max())
    print(kind, "lagrange on k_train_fs2: max |dtheta| after %d free-running steps = %.3g; penalty %.6g / %.6g" % (steps, d, glag.penalty, olag.penalty))
    assert info["actor_batches_trained"] == steps == 128 * epochs
    assert d < 2e-5
    for f in ("I", "smooth_delta", "smooth_Jc", "penalty", "cur_cost"):
        a, b = getattr(glag, f), getattr(olag, f)
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (f, a, b)


@pytest.mark.gpu
def test_learner_dispatch_over_random_shapes_matches_the_oracle(gpu_ctx):
    """Which kernel trains a network is decided by its shape (feature-split / two-CU / one-CU register-resident kernels, the dense engine, the generic one-workgroup learner),
    and every shape list is closed. Twenty random Chain(Dense, Dense, Dense) learners -- inputs 2..20, hidden widths in and out of the 64-wide family, 1..6 outputs, relu /
    tanh / mixed activations, categorical / Gaussian / critic heads, minibatches of 32..200 -- each replay two teacher-forced windows of four minibatch steps from the oracle's
    state (steps 2..5 and 9..12 of its trajectory): whatever kernel the dispatch picks must land on the oracle's parameters.
    (Its Gaussian rows of 4..8 actions train on fully clipped, dead surrogate gradients -- logprob ~ N(-1.2, 0.05); live gradients and the row edges: test_gpu_learner_row_edges.py.)"""
    rng = np.random.default_rng(2026)
    hid = [(64, 64), (64, 32), (32, 32), (128, 128), (48, 48), (64, 16), (256, 64), (64, 64), (64, 64)]
    worst = 0.0
    for case in range(20):
        od = int(rng.choice([2, 3, 4, 5, 8, 17, 20])); h1, h2 = hid[int(rng.integers(len(hid)))]; kind = ["categorical", "gaussian", "value"][int(rng.integers(3))]
        ad = int(rng.choice([2, 4, 6])) if kind == "categorical" else int(rng.choice([1, 2, 6]))
        out = 1 if kind == "value" else ad
        a1, a2 = [("relu", "relu"), ("tanh", "tanh"), ("tanh", "identity"), ("relu", "tanh")][int(rng.integers(4))]
        bs = int(rng.choice([32, 64, 100, 128, 200])); N = bs * 14
        disc = kind == "categorical"
        if disc:
            ai = rng.integers(0, ad, N); act = np.eye(ad, dtype=bool)[:, ai]
        else:
            act = rng.normal(0, 0.7, (ad, N)).astype(np.float32)
        data0 = {"s": rng.normal(0, 1, (od, N)).astype(np.float32), "a": act, "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
                 "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": rng.normal(0, 1, (1, N)).astype(np.float32),
                 "logprob": rng.normal(-1.2, 0.05, (1, N)).astype(np.float32), "advantage": rng.normal(0, 1, (1, N)).astype(np.float32)}
        dims, acts = [od, h1, h2, out], [a1, a2, "identity"]
        if kind == "categorical":
            g, o = parity.make_pair(dims, acts, 300 + case, 0, "discrete"); loss, head = "ppo", "categorical"
        elif kind == "gaussian":
            g, o = parity.make_pair(dims, acts, 300 + case, 0, "gaussian", n_extra=ad, extra_init=-0.5); loss, head = "ppo", "gaussian"
        else:
            g, o = parity.make_pair(dims, acts, 300 + case, 0); loss, head = "value_mse", "deterministic"
        res, _ = parity.learner_window_parity(g, o, data0, od, ad, disc, loss, head, bs, 1, [2, 9], 4, seed=700 + case)
        assert len(res) == 2, (case, dims, acts, kind, bs, res)
        for start, W, d in res:
            worst = max(worst, d)
            assert d < 2e-6, (case, dims, acts, kind, bs, start, d)          # measured: worst 3e-8 over the twenty shapes
    print("learner dispatch over 20 random shapes: worst window |dtheta| = %.3g" % worst)


@pytest.mark.gpu
def test_asynchronous_sac_solve_loop_equals_the_synchronous_one(gpu_ctx):
    """The same for SAC (crux_sac_epochs_async: three info rows per epoch -- temperature, critics, actor -- copied to the device ring by the recorded lists): networks, target
    critics, temperature and the per-iteration infos bit for bit against the loop that reads back after every chain."""
    def run(asyn):
        S = crux.ContinuousSpace(3); acts = ["relu", "relu", "identity"]
        pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 256, 256, 1], acts), np.zeros(1, np.float32), seed=2),
                              crux.DoubleNetwork(crux.ContinuousNetwork(parity.chain([4, 256, 256, 1], acts), seed=3), crux.ContinuousNetwork(parity.chain([4, 256, 256, 1], acts), seed=4)))
        sv = crux.SAC(pi, S, N=360, dN=12, buffer_size=1000, buffer_init=300, max_steps=50, c_opt={"batch_size": 256}, a_opt={"batch_size": 256}, SAC_alpha_opt={"batch_size": 256})
        sv.async_training = asyn
        crux.solve(sv, crux.PendulumMDP(n_envs=1, seed=8))
        keys = sorted(sv.history[-1])
        return [n.get_params() for n in (pi.A, pi.C.N1, pi.C.N2, sv.agent.pi_minus.C.N1, sv.P["SAC_log_alpha"])], np.array([[h[k] for k in keys] for h in sv.history]), keys
    (pa, ha, ka), (pb, hb, kb) = run(True), run(False)
    assert ka == kb and len(ha) == len(hb) >= 4 and "SAC alpha" in ka and "critic_loss" in ka and "actor_loss" in ka
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert np.array_equal(ha, hb)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_asynchronous_dpg_solve_loop_equals_the_synchronous_one(gpu_ctx, algo):
    """The same for DDPG / TD3 (crux_dpg_epochs_async: two info rows per epoch, critic | actor; TD3 trains its actor every second epoch, whose rows are skipped)."""
    twin = algo == "td3"
    def run(asyn):
        S = crux.ContinuousSpace(3)
        q = lambda s: crux.ContinuousNetwork(parity.chain([4, 256, 256, 1], ["relu", "relu", "identity"]), seed=s)
        pi = crux.ActorCritic(crux.ContinuousNetwork(parity.chain([3, 256, 256, 1], ["relu", "relu", "tanh" if twin else "identity"]), seed=2), crux.DoubleNetwork(q(3), q(4)) if twin else q(3))
        ctor = crux.TD3 if twin else crux.DDPG
        a_opt = {"batch_size": 128, "update_every": 2} if twin else {"batch_size": 128}
        sv = ctor(pi, S, N=200, dN=10, buffer_size=1000, buffer_init=140, max_steps=50, c_opt={"batch_size": 128, "epochs": 10}, a_opt=a_opt, noise_seed=5,
                  pi_explore=crux.GaussianNoiseExplorationPolicy(0.3, a_min=-1.0, a_max=1.0))
        sv.async_training = asyn
        crux.solve(sv, crux.PendulumMDP(n_envs=1, seed=8))
        nets = [pi.A, sv.agent.pi_minus.A] + ([pi.C.N1, pi.C.N2, sv.agent.pi_minus.C.N1, sv.agent.pi_minus.C.N2] if twin else [pi.C, sv.agent.pi_minus.C])
        keys = sorted(sv.history[-1])
        return [n.get_params() for n in nets], np.array([[h[k] for k in keys] for h in sv.history]), keys
    (pa, ha, ka), (pb, hb, kb) = run(True), run(False)
    assert ka == kb and "critic_loss" in ka and "actor_loss" in ka and len(ha) == len(hb) >= 4
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert np.array_equal(ha, hb)


@pytest.mark.gpu
def test_asynchronous_request_on_a_narrow_dqn_falls_back_to_the_synchronous_entry(gpu_ctx):
    """A DQN narrower than the dense engine (8-64-64-4 < CRUX_DENSE_MIN_WIDTH = 128) does not take the recorded chains: crux_dqn_value_training_async answers CRUX_EUNSUP on the
    first iteration, the solver marks itself (_async_unsupported) and every iteration runs through crux_dqn_epochs call by call, followed by the stand-alone target update --
    the same loop as with async_training off: networks, target networks, ring and per-iteration infos bit for bit, and nothing left pending."""
    def run(asyn):
        S = crux.ContinuousSpace(8)
        q = crux.DiscreteNetwork(parity.chain([8, 64, 64, 4], ["relu", "relu", "identity"]), [1, 2, 3, 4], seed=3)
        mdp = crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=5, discount=0.97)
        sv = crux.DQN(q, S, N=80, dN=4, buffer_size=128, buffer_init=40, max_steps=40, c_opt={"batch_size": 32})
        sv.async_training = asyn
        crux.solve(sv, mdp)
        if asyn:
            assert sv._async_unsupported is True and sv._pending == []
        return q.get_params(), sv.agent.pi_minus.get_params(), sv.buffer["s"], np.array([[h["critic_loss"], h["critic_grad_norm"], h["Qavg"]] for h in sv.history])
    a, b = run(True), run(False)
    assert len(a[3]) == len(b[3]) == 10 and np.isfinite(a[3]).all()          # buffer_init = 40 of the N = 80 steps fill the ring: (80 - 40) / dN iterations
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_asynchronous_request_without_chained_epochs_falls_back_for_sac(gpu_ctx, monkeypatch):
    """The same fallback with several info rows per epoch: with CRUX_NO_CHAINED_EPOCHS crux_sac_epochs_async answers CRUX_EUNSUP and value_training takes crux_sac_epochs
    (three host rows per epoch); asynchronous request and synchronous loop leave the same networks, temperature and infos, bit for bit. N counts the buffer_init = 70
    steps that fill the ring (solve's `stop` is taken before the fill), so N = 70 + 16 gives the four iterations of dN = 4 steps that are compared."""
    def run(asyn):
        S = crux.ContinuousSpace(3); acts = ["relu", "relu", "identity"]
        pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 128, 128, 1], acts), np.zeros(1, np.float32), seed=2),
                              crux.DoubleNetwork(crux.ContinuousNetwork(parity.chain([4, 128, 128, 1], acts), seed=3), crux.ContinuousNetwork(parity.chain([4, 128, 128, 1], acts), seed=4)))
        sv = crux.SAC(pi, S, N=70 + 16, dN=4, buffer_size=1000, buffer_init=70, max_steps=50, c_opt={"batch_size": 64}, a_opt={"batch_size": 64}, SAC_alpha_opt={"batch_size": 64})
        sv.async_training = asyn
        crux.solve(sv, crux.PendulumMDP(n_envs=1, seed=8))
        if asyn:
            assert sv._async_unsupported is True and sv._pending == []
        keys = sorted(sv.history[-1])
        return [n.get_params() for n in (pi.A, pi.C.N1, pi.C.N2, sv.agent.pi_minus.C.N1, sv.agent.pi_minus.C.N2, sv.P["SAC_log_alpha"])], np.array([[h[k] for k in keys] for h in sv.history]), keys
    monkeypatch.setenv("CRUX_NO_CHAINED_EPOCHS", "1"); crux.reload_switches()
    try:
        (pa, ha, ka), (pb, hb, kb) = run(True), run(False)
    finally:
        monkeypatch.delenv("CRUX_NO_CHAINED_EPOCHS"); crux.reload_switches()
    assert ka == kb and len(ha) == len(hb) == 4 and "SAC alpha" in ka and "critic_loss" in ka and "actor_loss" in ka and np.isfinite(ha).all()
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert np.array_equal(ha, hb)


@pytest.mark.gpu
def test_softq_refuses_a_non_positive_alpha_before_any_device_work(gpu_ctx):
    """softq_target(alpha) needs alpha > 0, and alpha = 0 is how crux_dqn_value_training_async is told to use dqn_target: the constructor refuses such a solver, and
    value_training refuses one whose P["alpha"] was changed afterwards before it draws a sample or touches a network."""
    S = crux.ContinuousSpace(8)
    net = lambda: crux.DiscreteNetwork(parity.chain([8, 128, 128, 4], ["relu", "relu", "identity"]), [1, 2, 3, 4], seed=4)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            crux.SoftQ(net(), S, N=8, alpha=bad)
    q = net()
    sv = crux.SoftQ(q, S, N=140 + 8, dN=4, buffer_size=256, buffer_init=140, max_steps=40, alpha=0.5, c_opt={"batch_size": 128})      # the fill and two iterations
    crux.solve(sv, crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=6, discount=0.97))
    assert len(sv.history) == 2
    n, p, pm, ind = len(sv.buffer), q.get_params(), sv.agent.pi_minus.get_params(), np.array(sv.batch.indices, copy=True)
    sv.P["alpha"] = np.float32(0)
    for asyn in (False, True):
        sv._async_now = asyn
        with pytest.raises(ValueError):
            crux.value_training(sv, sv.batch, np.float32(0.97))
    sv._async_now = False
    assert len(sv.buffer) == n and np.array_equal(q.get_params(), p) and np.array_equal(sv.agent.pi_minus.get_params(), pm) and np.array_equal(sv.batch.indices, ind)


@pytest.mark.gpu
@pytest.mark.parametrize("od,ad,kind,act", [(6, 3, "categorical", "relu"), (2, 3, "categorical", "relu"), (8, 2, "gaussian", "tanh"), (11, 3, "gaussian", "tanh"), (24, 4, "gaussian", "relu"),
                                            (27, 8, "gaussian", "tanh"), (27, 8, "value", "tanh"), (24, 4, "value", "relu"), (6, 3, "value", "relu")])
def test_gym_shapes_on_the_feature_split_kernel(gpu_ctx, capfd, od, ad, kind, act):
    """The standard Gym observation / action sizes added to the feature-split learner's dispatch in round 3 (Acrobot 6 / 3, MountainCar 2 / 3, LunarLanderContinuous 8 / 2, Hopper 11 / 3,
    BipedalWalker 24 / 4, Ant 27 / 8; 64-64 hidden): two teacher-forced windows of eight full-minibatch steps each against the oracle (B = 128: the feature-split kernel;
    CRUX_FS=0 would send these shapes to the dense engine).
    (Its Gaussian rows of 4..8 actions train on fully clipped, dead surrogate gradients -- logprob ~ N(-1.2, 0.05); live gradients and the row edges: test_gpu_learner_row_edges.py.)"""
    rng = np.random.default_rng(77 + od + ad); bs = 128; N = bs * 20; disc = kind == "categorical"
    if disc:
        ai = rng.integers(0, ad, N); actn = np.eye(ad, dtype=bool)[:, ai]
    else:
        actn = rng.normal(0, 0.7, (ad, N)).astype(np.float32)
    data0 = {"s": rng.normal(0, 1, (od, N)).astype(np.float32), "a": actn, "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
             "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": rng.normal(0, 1, (1, N)).astype(np.float32),
             "logprob": rng.normal(-1.2, 0.05, (1, N)).astype(np.float32), "advantage": rng.normal(0, 1, (1, N)).astype(np.float32)}
    out = 1 if kind == "value" else ad; dims, acts = [od, 64, 64, out], [act, act, "identity"]
    if kind == "categorical":
        g, o = parity.make_pair(dims, acts, 400 + od, 0, "discrete"); loss, head = "ppo", "categorical"
    elif kind == "gaussian":
        g, o = parity.make_pair(dims, acts, 400 + od, 0, "gaussian", n_extra=ad, extra_init=-0.5); loss, head = "ppo", "gaussian"
    else:
        g, o = parity.make_pair(dims, acts, 400 + od, 0); loss, head = "value_mse", "deterministic"
    res, _ = parity.learner_window_parity(g, o, data0, od, ad, disc, loss, head, bs, 1, [2, 11], 8, seed=800 + od)
    assert len(res) == 2
    for start, W, d in res:
        assert d < 2e-6, (start, d)
    assert "outside the MFMA learner family" not in capfd.readouterr().err


@pytest.mark.gpu
def test_a_64_wide_shape_without_an_instantiation_takes_the_dense_engine_on_both_learner_streams(gpu_ctx, capfd):
    """policy_gradient_training treats every 64-wide pair as the register-resident family and launches the critic on the second learner stream; a shape none of those kernels
    instantiates (5 observations / 3 actions) used to fall to the generic one-workgroup learner there (the dense engine was bound to the main stream). It now takes the dense
    engine on either stream: oracle parity of the whole iteration, and no "outside the MFMA learner family" announcement."""
    res = parity.ppo_iteration_parity(n_envs=8, T=64, batch_size=128, epochs=2, seed=19, family="synth_5_3", pair=True)
    assert res["ok"], res
    assert "outside the MFMA learner family" not in capfd.readouterr().err
