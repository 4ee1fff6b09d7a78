"""Round 5: parity at the sizes bench.py times.

  * C1 (BASELINE configs[0], the README example) at N = 100 000 through k_dqn_tiny_solve: the eps-greedy trajectory is bit-exact with the oracle's loop until the first greedy
    argmax that flips on a last-bit difference of the two networks (the kernel sums the minibatch gradient in another order than the oracle's scalar loop); the test reports where,
    bounds the networks there, and compares the two runs statistically from there on;
  * C3 (configs[2]) `solve` on the 1 M-row prioritized ring BASELINE names: 50 iterations of steps! + 4 value_training epochs against the oracle's loop -- ring rows and sampled
    indices bit-exact, priorities and networks to the bounds of tests/test_gpu_fullsize.py."""
import ctypes as C

import numpy as np
import pytest

import parity
from parity import L, O, crux

pytestmark = pytest.mark.gpu


class _OracleReadmeDQN:
    """solve(::OffPolicySolver) (off_policy.jl:113-150, :66-111) for DQN on SimpleGridWorld at the README's shapes, advanced in pieces"""

    def __init__(self, N, dN=4, B=128, cap=1000, init=200, seed_net=1, seed_env=0, max_steps=100):
        self.o = O.OMlp([2, 8, 4], ["relu", "identity"]).init_glorot(seed_net).adam_init(float(np.float32(3e-4)))
        self.ot = O.OMlp([2, 8, 4], ["relu", "identity"]).init_glorot(seed_net)
        self.ob = O.OBuffer(2, 4, L.ACTION_DISCRETE, cap); self.obt = O.OBuffer(2, 4, L.ACTION_DISCRETE, B)
        self.oe = O.OEnv("gridworld", 1, max_steps, 0.95, seed_env)
        self.cfg = parity.rollout_cfg(True, False, "greedy_q"); self.cfg.eps_start, self.cfg.eps_stop, self.cfg.eps_steps = 1.0, 0.1, N // 2
        self.dN, self.B, self.i = dN, B, init
        self.y = np.empty(B, np.float32); self.info = np.zeros(L.INFO_N, np.float32); self.losses = []
        self.cfg.i0 = init; self.oe.rollout(self.o, self.cfg, self.ob, init)

    def run(self, n_iter):
        for _ in range(n_iter):
            self.cfg.i0 = self.i; self.oe.rollout(self.o, self.cfg, self.ob, self.dN)
            ls = []
            for ep in range(self.dN):
                O.chk(O.lib().orc_uniform_sample(self.obt.h, self.ob.h, self.B, None, self.i * self.dN + ep, crux.api.SAMPLE_SEED))
                O.chk(O.lib().orc_dqn_target(self.ot.h, self.obt.h, 0.95, O.vpz(self.y)))
                O.chk(O.lib().orc_td_step(self.o.h, self.obt.h, O.vpz(self.y), 0, O.vpz(self.info))); ls.append(float(self.info[0]))
            O.chk(O.lib().orc_polyak(self.ot.h, self.o.h, 0.005))
            self.losses.append(float(np.mean(ls))); self.i += self.dN


def test_c1_at_the_benchmarked_size_follows_the_oracle_until_the_first_argmax_flip(gpu_ctx):
    N, chunk = 100_000, 1000                       # chunk = the ring's capacity: every transition of the run is compared once
    q = crux.DiscreteNetwork(parity.chain([2, 8, 4], ["relu", "identity"]), [1, 2, 3, 4], seed=1)
    sv = crux.DQN(q, crux.ContinuousSpace(2), N=chunk + 200, dN=4, max_steps=100, c_opt={"batch_size": 128},
                  pi_explore=crux.EpsGreedyPolicy(crux.LinearDecaySchedule(1.0, 0.1, N // 2), [1, 2, 3, 4]))
    orc = _OracleReadmeDQN(N)
    mdp = crux.SimpleGridWorld(n_envs=1, seed=0)
    ctx = q.ctx; ctx.prof_enable(True); ctx.prof_reset()
    first_diff, dq_at, done_steps = None, None, 200
    while done_steps < N:
        crux.solve(sv, mdp); sv.N = chunk            # (the first call also fills the ring's first 200 rows, off_policy.jl:122-126)
        orc.run(chunk // 4); done_steps += chunk
        assert sv.i == orc.i
        if first_diff is None:
            same = all(np.array_equal(sv.buffer[k], orc.ob[k]) for k in ("s", "a", "sp", "r", "done"))
            if same:
                dq_at = float(np.abs(q.get_params() - orc.o.params).max())
            else:
                first_diff = done_steps
    ms, n_tiny = ctx.prof_get("tiny_solve"); ctx.prof_enable(False)
    assert n_tiny >= N // chunk - 1                                    # every chunk ran in the wave-resident kernel bench.py times for configs[0]
    gl = np.array([h["critic_loss"] for h in sv.history]); ol = np.array(orc.losses)
    print("C1 at N = %d: trajectories bit-exact for the first %s environment steps (the ring is compared every %d); max |dtheta| at the last identical ring %.3g; "
          "mean loss of the last 5 000 iterations %.4g (GPU) / %.4g (oracle)" % (N, "%d+" % N if first_diff is None else str(first_diff - chunk), chunk, dq_at, gl[-5000:].mean(), ol[-5000:].mean()))
    # measured (profiles/r05_parity_measurements.txt): identical trajectories for the first 77 200 environment steps = 77 000 Adam steps; the free-running networks are 4.4e-4
    # apart there (a relu DQN is a chaotic map: tests/parity.py; the arithmetic itself is pinned by the 320-iteration test of test_gpu_round3.py to 7e-8)
    assert first_diff is None or first_diff - chunk >= 20_000
    assert dq_at < 5e-3
    # after the first flip the two runs are different samples of the same training process: their losses agree statistically
    assert len(gl) == len(ol) and abs(gl[-5000:].mean() - ol[-5000:].mean()) < 0.5 * max(gl[-5000:].mean(), ol[-5000:].mean())
    assert np.isfinite(q.get_params()).all()


def _c3_problem(N, seed_data=77):
    rng = np.random.default_rng(seed_data); B, od, ad = 128, 8, 4
    dims, acts = [8, 256, 256, 4], ["relu", "relu", "identity"]
    g, o = parity.make_pair(dims, acts, 41, 0, "discrete")
    S, A = crux.ContinuousSpace(od), crux.DiscreteSpace(ad)
    buf = crux.ExperienceBuffer(S, A, N, prioritized=True)
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE, N, ["weight"], prioritized=True, alpha=np.float32(0.6)); obt = O.OBuffer(od, ad, L.ACTION_DISCRETE, B, ["weight"], prioritized=True, alpha=np.float32(0.6))
    d = {"s": rng.standard_normal((od, N)).astype(np.float32), "sp": rng.standard_normal((od, N)).astype(np.float32), "r": rng.standard_normal((1, N)).astype(np.float32),
         "done": rng.random((1, N)) < 0.05, "episode_end": rng.random((1, N)) < 0.05}
    a = np.zeros((ad, N), np.bool_); a[rng.integers(0, ad, N), np.arange(N)] = True; d["a"] = a
    buf.push_(d); ob.push(d)
    I = rng.choice(N, N // 5, replace=False).astype(np.int64); v = np.abs(rng.standard_normal(I.size)) + 1e-3          # a non-trivial priority landscape
    buf.update_priorities_(I + 1, v); O.chk(O.lib().orc_per_update(ob.h, O.vpz(I), O.vpz(v), 1, I.size))
    ot = O.OMlp(dims, acts); O.chk(O.lib().orc_mlp_copy(ot.h, o.h)); o.adam_init(float(np.float32(1e-3)))
    return g, o, ot, buf, ob, obt, S


@pytest.mark.parametrize("forced", [True, False], ids=["teacher_forced_every_iteration", "free_running"])
def test_c3_solve_on_the_one_million_row_prioritized_ring(gpu_ctx, forced):
    """BASELINE configs[2] through `solve`: DQN + prioritized ExperienceBuffer of 1 M transitions (full: every epoch searches the whole pairwise tree), 8->256->256->4, B = 128,
    dN = 4, weighted td_loss; 50 iterations of steps! (eps-greedy, push! with the maximal priority) + four value_training epochs (prioritized_sample!, dqn_target, td_error ->
    update_priorities!, train!) + polyak through crux.solve -- the chained asynchronous epochs bench.py times -- against the oracle's loop with its full cumsum rescan per epoch.

    A prioritized learner is a chaotic map twice over: Adam's first steps turn a last-bit gradient difference into an lr-sized one, and the td errors written back as priorities
    steer which rows the next epoch draws -- free-running, the sampled rows leave the oracle's after a handful of iterations (reported; the two runs then agree statistically).
    TEACHER-FORCED, every iteration starts from the oracle's state (both networks, Adam's moments, and the priorities the oracle wrote in the iteration before, replayed through
    update_priorities! with the oracle's td errors): then all 50 iterations must draw the oracle's rows, bit for bit, and stay within one iteration's float tolerance."""
    N, B, iters, dN, max_steps, seed = 1_000_000, 128, 50, 4, 200, 3
    g, o, ot, buf, ob, obt, S = _c3_problem(N)
    mdp = crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=seed)
    sv = crux.DQN(g, S, N=dN, dN=dN, buffer=buf, buffer_init=N, prioritized=True, weighted_loss=True, max_steps=max_steps, c_opt={"batch_size": B, "optimizer": crux.Adam(np.float32(1e-3))},
                  pi_explore=crux.EpsGreedyPolicy(crux.LinearDecaySchedule(1.0, 0.1, (dN * iters) // 2), [1, 2, 3, 4]))
    oe = O.OEnv("synth_discrete", 1, max_steps, 0.99, seed, so=8, sa=4)
    cfg = parity.rollout_cfg(True, False, "greedy_q"); cfg.eps_start, cfg.eps_stop, cfg.eps_steps = 1.0, 0.1, (dN * iters) // 2
    y = np.empty(B, np.float32); err = np.empty(B, np.float32); ids = np.empty(B, np.int64); info = np.zeros(L.INFO_N, np.float32)
    first_idx_diff = first_row_diff = None; worst_dq = 0.0; gl, ol = [], []
    for it in range(iters):
        i = it * dN
        if forced:      # the oracle's state of this moment into the GPU twins
            g.set_params(o.params.copy()); g.set_adam_state(*o.adam_state()); sv.agent.pi_minus.set_params(ot.params.copy())
        crux.solve(sv, mdp)                                               # one iteration (sv.N = dN): steps!, four chained epochs, polyak
        assert getattr(sv, "_async_unsupported", False) is False          # through the asynchronous chains (crux_dqn_value_training_async)
        cfg.i0 = i; oe.rollout(o, cfg, ob, dN)
        written = []
        for ep in range(dN):
            O.chk(O.lib().orc_per_sample(obt.h, ob.h, B, None, 0.5, i * dN + ep, crux.api.SAMPLE_SEED))
            O.chk(O.lib().orc_dqn_target(ot.h, obt.h, 0.99, O.vpz(y)))
            O.chk(O.lib().orc_td_error(o.h, obt.h, O.vpz(y), O.vpz(err))); O.chk(O.lib().orc_buffer_indices(obt.h, O.vpz(ids), B))
            O.chk(O.lib().orc_per_update(ob.h, O.vpz(ids), O.vpz(err), 0, B)); written.append((ids.copy(), err.copy()))
            O.chk(O.lib().orc_td_step(o.h, obt.h, O.vpz(y), 1, O.vpz(info)))
        O.chk(O.lib().orc_polyak(ot.h, o.h, 0.005))
        gl.append(sv.history[-1]["critic_loss"]); ol.append(float(info[0]))
        new = (i + np.arange(dN)) % N; rows = buf.minibatch(new + 1)
        rows_same = all(np.array_equal(rows[k], ob[k][..., new]) for k in ("s", "a", "sp", "r", "done"))
        idx_same = np.array_equal(sv.batch.indices[:B], ids)
        dq = float(np.abs(g.get_params() - o.params).max())
        if forced:
            assert rows_same and idx_same, "iteration %d: %s" % (it, "rows" if not rows_same else "sampled indices")
            worst_dq = max(worst_dq, dq)
            for w_ids, w_err in written:                                   # the priorities the oracle wrote, replayed from the same Float32 td errors
                buf.update_priorities_(w_ids + 1, w_err)
        else:
            if first_idx_diff is None and not idx_same:
                first_idx_diff = it
            if first_row_diff is None and not rows_same:
                first_row_diff = it
    assert sv.i == dN * iters and len(buf) == len(ob) == N and buf.next_ind == O.lib().orc_buffer_next_ind(ob.h) + 1
    if forced:
        ppg, maxo, mino = buf.priority_params(), np.zeros(1, np.float32), np.zeros(1, np.float32)
        pro = np.empty(N, np.float32); O.chk(O.lib().orc_per_get(ob.h, O.vpz(pro), maxo.ctypes.data_as(C.POINTER(C.c_float)), mino.ctypes.data_as(C.POINTER(C.c_float)), None))
        dpr = np.abs(ppg["priorities"][:N] - pro)
        print("C3 solve, 1 M-row ring, teacher-forced every iteration: %d iterations (%d epochs) draw the oracle's rows bit for bit; max |dtheta| after an iteration %.3g; priorities max |dp| %.3g"
              % (iters, iters * dN, worst_dq, dpr.max()))
        # (measured 2.0e-4, in Adam's first steps at lr = 1e-3: v is tiny there and lr m / (sqrt(v) + eps) turns a last-bit gradient difference into a fraction of lr -- tests/parity.py)
        assert worst_dq < 1e-3 and ((dpr <= 1e-5 * pro) | (dpr <= 1e-4)).all()
    else:
        print("C3 solve, 1 M-row ring, free-running: sampled rows leave the oracle's at iteration %s, the trajectory at iteration %s; mean loss of the last 20 iterations %.4g (GPU) / %.4g (oracle)"
              % (first_idx_diff, first_row_diff, np.mean(gl[-20:]), np.mean(ol[-20:])))
        assert first_idx_diff is None or first_idx_diff >= 2
        assert abs(np.mean(gl[-20:]) - np.mean(ol[-20:])) < 0.5 * max(np.mean(gl[-20:]), np.mean(ol[-20:])) and np.isfinite(g.get_params()).all()


def _small_per_solve(N=4096, iters=24, dN=4, seed=5):
    """a DQN + PER solve on a FULL ring of N rows (the incremental tree, crux_per_touched): parameters, priorities, the materialised cumsum and the sampled ids afterwards"""
    rng = np.random.default_rng(17); od, ad, B = 8, 4, 64
    g, _ = parity.make_pair([8, 256, 256, 4], ["relu", "relu", "identity"], 23, 0, "discrete")
    S, A = crux.ContinuousSpace(od), crux.DiscreteSpace(ad)
    buf = crux.ExperienceBuffer(S, A, N, prioritized=True)
    d = {"s": rng.standard_normal((od, N)).astype(np.float32), "sp": rng.standard_normal((od, N)).astype(np.float32), "r": rng.standard_normal((1, N)).astype(np.float32),
         "done": rng.random((1, N)) < 0.05, "episode_end": rng.random((1, N)) < 0.05}
    a = np.zeros((ad, N), np.bool_); a[rng.integers(0, ad, N), np.arange(N)] = True; d["a"] = a
    buf.push_(d)
    sv = crux.DQN(g, S, N=dN * iters, dN=dN, buffer=buf, buffer_init=N, prioritized=True, weighted_loss=True, max_steps=50, c_opt={"batch_size": B, "optimizer": crux.Adam(np.float32(1e-3))})
    crux.solve(sv, crux.SynthMDP(8, 4, discrete=True, n_envs=1, seed=seed))
    pp = buf.priority_params()
    return g.get_params(), pp["priorities"][:N].copy(), buf.cumsum()[:N].copy(), float(pp["max_priority"]), float(pp["min_priority"]), sv.batch.indices[:B].copy(), buf["s"].copy()


def test_push_bookkeeping_as_one_launch_equals_the_separate_launches(gpu_ctx, monkeypatch):
    """push!'s priority bookkeeping for the dN rows of an off-policy iteration (ring rows, max-priority snapshot, update_priorities!, leaf re-sum, root paths: k_push_touch, one
    launch) against CRUX_PUSH_FUSED=0 (the five separate launches): everything a solve leaves behind, bit for bit."""
    monkeypatch.setenv("CRUX_PUSH_FUSED", "0"); ref = _small_per_solve()
    monkeypatch.delenv("CRUX_PUSH_FUSED"); got = _small_per_solve()
    for x, y, name in zip(ref, got, ("params", "priorities", "cumsum", "max_priority", "min_priority", "indices", "s")):
        assert np.array_equal(np.asarray(x), np.asarray(y)), name
