"""GPU parity: the off-policy step heads (csrc/sac.hip) and the recorded epoch plans (csrc/exec.hip) on both sides of B = 256.

The single-block heads (k_q_head, k_td_head, k_temp_head, k_actor_head, k_mean_info, k_gail_head, k_rowsum) walk the batch with `for (j = threadIdx.x; j < B; j += 256)`,
k_gail_reward strides 64 x 256 rows, and exec.hip picks other phase plans for B > 256 (no sequential target + head group, root paths as an op of their own). Every entry runs
here on B_EDGES = 1 (one row), 37 (less than a wave), 63 / 65 (either side of a wave), 255 / 257 (either side of the block stride), 300 (ragged second trip) and 1000 (three
full trips and a ragged fourth) against the CPU oracle, and the plans run at B = 320 against the oracle's loop.

Tolerances, and where each comes from
  * targets y: 1e-4 relative (SAC / DPG), 1e-5 absolute (dqn_target, softq_target, td_error) -- tests/test_gpu_sac.py::test_sac_steps_match_oracle,
    ::test_dpg_steps_match_oracle and tests/test_gpu_components.py::test_dqn_target_td_error_td_step_match_oracle, unchanged.
  * info rows of the SAC family (loss, grad_norm, alpha, q1avg, q2avg, entropy): 2e-5 x max(1, |ref|) (test_sac_steps_match_oracle); of the DPG family 1e-4 (critic) and 2e-4
    (actor) x max(1, |ref|) (test_dpg_steps_match_oracle); of td_step 1e-5 (loss, mean Q) and 1e-4 (norm) (test_dqn_target_...); of gail_d_step 1e-4 x max(1, |ref|) and of
    gail_reward 2e-5 x max(1, |ref|) (tests/test_gpu_gail.py::test_gail_discriminator_step_and_reward_match_oracle).
  * trained networks: _step_close of tests/test_gpu_sac.py (gradient within 1e-4 of its scale; parameters: none off by 2e-4, at most 0.4 % off by more than 2e-6), log alpha 2e-6.
    No case here needed the left-out rule for Adam's first-step discontinuity: every _step_close holds as it is.
  * the float64 recomputation of the reductions (numpy, from the oracle's per-row values): the same 2e-5 x max(1, |ref|) as the info rows it checks.
  * rows the caller owns (d_y, d_err, the reward column past `elements`): exact -- every row below B is written, every row from B on keeps the sentinel 12345.0.
  * teacher-forced window at B = 320: OFFPOLICY_WINDOW_TOL[0] = 8e-6 of tests/test_gpu_round3.py, unchanged; measured 3.0e-8 (sac) and 1.5e-8 (td3).
  * crux_dqn_epoch at B = 320: identical sampled ids and rows, _step_close, priorities within 1e-5 (measured 3.2e-6).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import parity
from dense_reference import _np_mlp
from parity import crux, L, O
from test_gpu_gail import _bufs
from test_gpu_round3 import OFFPOLICY_WINDOW_TOL, _inject, _replay_source
from test_gpu_sac import _batch_pair, _grads, _sac_pair, _step_close

pytestmark = pytest.mark.gpu

B_EDGES = [1, 37, 63, 65, 255, 257, 300, 1000]
B_VARIANTS = [1, 257, 1000]
SENTINEL, PAD = np.float32(12345.0), 64
LR = float(np.float32(1e-3))

# (od, ad, hidden): the base network on every B, the other shapes on B_VARIANTS; tanh hidden layers (a relu kink that flips between the tile-ordered sum and the oracle's
# scalar loop moves a whole gradient column, see _step_close)
_NET_CASES = [(3, 1, [32], B) for B in B_EDGES] + [(od, ad, hidden, B) for (od, ad, hidden) in ((17, 6, [64, 64]), (3, 1, [64, 64]), (17, 6, [32])) for B in B_VARIANTS]


def _case_id(c):
    return "%d-%s-%d-B%d" % (c[0], "x".join(map(str, c[2])), c[1], c[3]) + ("-" + c[4] if len(c) > 4 else "")


def _acts(hidden, last="identity"):
    return ["tanh"] * len(hidden) + [last]


def _close(a, b, tol=2e-5):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


class _Guarded:
    """n floats the caller owns, followed by PAD more; all hold the sentinel until a kernel writes them"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.d = ctx.alloc(4 * (n + PAD)); self.fill()

    def fill(self):
        self.ctx.h2d(self.d, np.full(self.n + PAD, SENTINEL, np.float32))

    def read(self):
        """the n rows, after checking that each of them was written and that nothing behind them was"""
        a = self.ctx.d2h(self.d, np.empty(self.n + PAD, np.float32))
        unwritten, over = np.flatnonzero(a[:self.n] == SENTINEL), np.flatnonzero(a[self.n:] != SENTINEL)
        assert unwritten.size == 0, "rows never written: %s ..." % unwritten[:8]
        assert over.size == 0, "rows written past the batch: %s ..." % (self.n + over[:8])
        return a[:self.n].copy()

    def free(self):
        self.ctx.free(self.d)


def _randn64(seed, counter, n):
    """sac_randn (csrc/sac.hip; oracle randn_f32): Box-Muller's first output of Philox(seed, counter, stream = i, CRUX_RNG_NOISE), element i = j * ad + d"""
    out4, e = np.zeros(4, np.uint32), np.empty(n, np.float64)
    for i in range(n):
        O.lib().orc_philox(seed, counter, i, 2, O.vpz(out4))
        u1, u2 = ((int(out4[0]) << 32 | int(out4[1])) >> 11) * 1.1102230246251565e-16, ((int(out4[2]) << 32 | int(out4[3])) >> 11) * 1.1102230246251565e-16
        e[i] = np.float32(np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2))
    return e


# ---------------------------------------------------------------------------------------------------- A. SAC step family
_SAC_CASES = [c + ("tanh",) for c in _NET_CASES] + [(3, 1, [256, 256], 257, "relu")]      # relu 4-256-256-1 at 257: the first batch past the fused-pullback gate 128 <= B <= 256 (dense_fused.h)


@pytest.mark.parametrize("od,ad,hidden,B,q_act", _SAC_CASES, ids=[_case_id(c) for c in _SAC_CASES])
def test_sac_steps_match_oracle_on_batch_edges(gpu_ctx, od, ad, hidden, B, q_act):
    """crux_sac_target, crux_sac_temp_step, crux_double_q_step (unweighted, then weighted), crux_sac_actor_step against their oracle counterparts; two repetitions, so the
    second starts from non-zero Adam moments. At B in {257, 1000} the critic's and the actor's loss statistics are recomputed in numpy float64 from the oracle's per-row
    values as well (the oracle and the device could share a mistake in the reduction)."""
    ctx, rng, seed = gpu_ctx, np.random.default_rng(100 + B), 21
    a_acts = [q_act] * len(hidden) + ["identity"]
    (ga, g1, g2), (oa, o1, o2), (adims, qdims, qacts) = _sac_pair(od, ad, hidden, q_act, a_acts, 5, ctx)
    pim = crux.clone_policy(crux.ActorCritic(ga, crux.DoubleNetwork(g1, g2)))
    ot1, ot2 = O.OMlp(qdims, qacts), O.OMlp(qdims, qacts)
    for gt, ot in ((pim.C.N1, ot1), (pim.C.N2, ot2)):
        p = gt.get_params() + rng.normal(0, 0.02, gt.n_params).astype(np.float32); gt.set_params(p); ot.params[:] = p
    gla = crux.ParamVector([np.log(np.float32(0.7))], ctx=ctx); ola = O.OMlp([0], [], 1); ola.params[:] = gla.get_params()
    for g, o in ((ga, oa), (g1, o1), (g2, o2), (gla, ola)):
        g.attach_optimizer(crux.Adam(np.float32(1e-3))); o.adam_init(LR)
    gb, ob = _batch_pair(rng, od, ad, B, ctx, weight=True)
    s64, sa64, w64 = ob["s"].astype(np.float64), np.vstack([ob["s"], ob["a"]]).astype(np.float64), ob["weight"][0].astype(np.float64)
    lib, ol = ctx.lib, O.lib()
    dy = _Guarded(ctx, B); yo = np.empty(B, np.float32)
    gi, oi = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    independent = B in (257, 1000)
    for rep in range(2):
        ctr = 100 + rep
        dy.fill()
        ctx.check(lib.crux_sac_target(ga.h, pim.C.N1.h, pim.C.N2.h, gla.h, gb.h, 0.99, seed, 3 * ctr, dy.d)); y = dy.read()
        O.chk(ol.orc_sac_target(oa.h, ot1.h, ot2.h, ola.h, ob.h, 0.99, seed, 3 * ctr, O.vpz(yo)))
        assert np.abs(y - yo).max() < 1e-4 * max(1, np.abs(yo).max())
        ctx.check(lib.crux_sac_temp_step(ga.h, gla.h, gb.h, float(-ad), seed, 3 * ctr + 1, O.vpz(gi)))
        O.chk(ol.orc_sac_temp_step(oa.h, ola.h, ob.h, float(-ad), seed, 3 * ctr + 1, O.vpz(oi)))
        for k in ("loss", "grad_norm", "alpha"):
            assert _close(gi[L.INFO[k]], oi[L.INFO[k]]), ("temp", k, rep, gi, oi)
        assert np.abs(gla.get_params() - ola.params).max() < 2e-6
        p1, p2 = o1.params.copy(), o2.params.copy()
        ctx.check(lib.crux_double_q_step(g1.h, g2.h, gb.h, dy.d, rep, O.vpz(gi)))
        O.chk(ol.orc_double_q_step(o1.h, o2.h, ob.h, O.vpz(yo), rep, O.vpz(oi)))
        for k in ("loss", "grad_norm", "q1avg", "q2avg"):
            assert _close(gi[L.INFO[k]], oi[L.INFO[k]]), ("critic", k, rep, gi, oi)
        if independent:
            Q1, Q2 = _np_mlp(p1, qdims, qacts, sa64)[-1][0], _np_mlp(p2, qdims, qacts, sa64)[-1][0]; w = w64 if rep else 1.0; y64 = yo.astype(np.float64)
            ref = {"loss": 0.5 * np.mean((Q1 - y64) ** 2 * w) + 0.5 * np.mean((Q2 - y64) ** 2 * w), "q1avg": Q1.mean(), "q2avg": Q2.mean()}
            for k, v in ref.items():
                assert _close(gi[L.INFO[k]], v), ("critic vs float64", k, rep, gi[L.INFO[k]], v)
        assert _step_close(g1, o1, ctx) and _step_close(g2, o2, ctx), rep
        pa, p1, p2, la = oa.params.copy(), o1.params.copy(), o2.params.copy(), float(ola.params[0])
        ctx.check(lib.crux_sac_actor_step(ga.h, g1.h, g2.h, gla.h, gb.h, seed, 3 * ctr + 2, O.vpz(gi)))
        O.chk(ol.orc_sac_actor_step(oa.h, o1.h, o2.h, ola.h, ob.h, seed, 3 * ctr + 2, O.vpz(oi)))
        for k in ("loss", "grad_norm", "entropy"):
            assert _close(gi[L.INFO[k]], oi[L.INFO[k]]), ("actor", k, rep, gi, oi)
        if independent:      # sac_actor_loss (sac.jl:34-40) row by row: a = eps * sigma + mu, gaussian_logpdf, min(Q1, Q2)(s, a)
            n_w = pa.size - ad; mu = _np_mlp(pa[:n_w], adims, a_acts, s64)[-1]; ls = pa[n_w:].astype(np.float64)[:, None]; sg = np.exp(ls)
            eps = _randn64(seed, 3 * ctr + 2, B * ad).reshape((ad, B), order="F"); act = eps * sg + mu
            lp = (-(act - mu) ** 2 / (2 * sg * sg) - 0.9189385332046727 - ls).sum(0)
            x = np.vstack([s64, act]); mn = np.minimum(_np_mlp(p1, qdims, qacts, x)[-1][0], _np_mlp(p2, qdims, qacts, x)[-1][0])
            ref = {"loss": np.mean(np.exp(np.float32(la)) * lp - mn), "entropy": -lp.mean()}
            for k, v in ref.items():
                assert _close(gi[L.INFO[k]], v), ("actor vs float64", k, rep, gi[L.INFO[k]], v)
        assert _step_close(ga, oa, ctx), rep
    m, v, bp = ga.adam_state(); mo, vo, bpo = oa.adam_state()
    assert np.allclose(bp, bpo) and np.abs(m - mo).max() < 1e-5
    dy.free()


# ---------------------------------------------------------------------------------------------------- A. DPG step family
@pytest.mark.parametrize("od,ad,hidden,B", _NET_CASES, ids=[_case_id(c) for c in _NET_CASES])
def test_dpg_steps_match_oracle_on_batch_edges(gpu_ctx, od, ad, hidden, B):
    """crux_dpg_target (single / twin critic, with / without TD3 target smoothing), crux_q_step (unweighted, then weighted), crux_dpg_actor_step (k_mean_info) against the
    oracle, with the assertions of test_dpg_steps_match_oracle."""
    ctx, rng, seed = gpu_ctx, np.random.default_rng(200 + B), 33
    adims, qdims, aacts, qacts = [od] + hidden + [ad], [od + ad] + hidden + [1], _acts(hidden), _acts(hidden)
    ga, oa = parity.make_pair(adims, aacts, 7, 0); g1, o1 = parity.make_pair(qdims, qacts, 7, 1)
    gat, oat = parity.make_pair(adims, aacts, 8, 0); g1t, o1t = parity.make_pair(qdims, qacts, 8, 1); g2t, o2t = parity.make_pair(qdims, qacts, 8, 2)
    for g, o in ((ga, oa), (g1, o1)):
        g.attach_optimizer(crux.Adam(np.float32(1e-3))); o.adam_init(LR)
    gb, ob = _batch_pair(rng, od, ad, B, ctx, weight=True)
    lib, ol = ctx.lib, O.lib()
    dy = _Guarded(ctx, B); yo = np.empty(B, np.float32)
    gi, oi = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    smooth, plain = (0.2, -0.5, 0.5, -1.0, 1.0), (-1.0, 0.0, 0.0, 0.0, 0.0)
    for rep in range(2):
        for twin, sm in itertools.product((True, False), (smooth, plain)):      # the last one (single critic, no smoothing: ddpg_target) feeds the critic step
            dy.fill()
            ctx.check(lib.crux_dpg_target(gat.h, g1t.h, g2t.h if twin else None, gb.h, 0.99, *sm, seed, 50 + rep, dy.d)); y = dy.read()
            O.chk(ol.orc_dpg_target(oat.h, o1t.h, o2t.h if twin else None, ob.h, 0.99, *sm, seed, 50 + rep, O.vpz(yo)))
            assert np.abs(y - yo).max() < 1e-4 * max(1, np.abs(yo).max()), (twin, sm, rep)
        ctx.check(lib.crux_q_step(g1.h, gb.h, dy.d, rep, O.vpz(gi))); O.chk(ol.orc_q_step(o1.h, ob.h, O.vpz(yo), rep, O.vpz(oi)))
        for k in ("loss", "grad_norm", "q1avg"):
            assert _close(gi[L.INFO[k]], oi[L.INFO[k]], 1e-4), ("critic", k, rep, gi, oi)
        assert _step_close(g1, o1, ctx), rep
        ctx.check(lib.crux_dpg_actor_step(ga.h, g1.h, gb.h, O.vpz(gi))); O.chk(ol.orc_dpg_actor_step(oa.h, o1.h, ob.h, O.vpz(oi)))
        for k in ("loss", "grad_norm"):
            assert _close(gi[L.INFO[k]], oi[L.INFO[k]], 2e-4), ("actor", k, rep, gi, oi)
        assert _step_close(ga, oa, ctx), rep
    dy.free()


# ---------------------------------------------------------------------------------------------------- A. TD step family
def _discrete_batch(rng, od, na, n, ctx):
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(na), n, ["weight"], ctx=ctx); ob = O.OBuffer(od, na, L.ACTION_DISCRETE, n, ["weight"])
    a = np.zeros((na, n), np.bool_); a[rng.integers(0, na, n), np.arange(n)] = True
    d = {"s": rng.standard_normal((od, n)).astype(np.float32), "sp": rng.standard_normal((od, n)).astype(np.float32), "r": rng.standard_normal((1, n)).astype(np.float32),
         "done": rng.random((1, n)) < 0.2, "episode_end": rng.random((1, n)) < 0.2, "a": a, "weight": rng.random((1, n)).astype(np.float32)}
    gb.push_(d); ob.push(d)
    return gb, ob


@pytest.mark.parametrize("B", B_EDGES)
@pytest.mark.parametrize("dims,acts", [([2, 8, 4], ["relu", "identity"]),                                   # the single-workgroup learner of train.hip
                                       ([8, 256, 256, 4], ["relu", "relu", "identity"])], ids=["narrow", "dense"])      # crux_td_step_dense with k_td_head
def test_td_steps_match_oracle_on_batch_edges(gpu_ctx, dims, acts, B):
    """crux_dqn_target, crux_softq_target, crux_td_error, crux_td_step (weights off, then on) and crux_td_step_with_error on both routes, with the assertions of
    test_dqn_target_td_error_td_step_match_oracle; crux_td_step_with_error == crux_td_error followed by crux_td_step as that test states per route."""
    ctx, rng = gpu_ctx, np.random.default_rng(300 + B); n, od, na, dense = B, dims[0], dims[-1], max(dims) >= 128
    g, o = parity.make_pair(dims, acts, 31, 0, "discrete"); gt, ot = parity.make_pair(dims, acts, 32, 0, "discrete")
    gb, ob = _discrete_batch(rng, od, na, n, ctx)
    dy, de, de2 = _Guarded(ctx, n), _Guarded(ctx, n), _Guarded(ctx, n); oy, oerr = np.empty(n, np.float32), np.empty(n, np.float32)
    ctx.check(ctx.lib.crux_softq_target(gt.h, gb.h, 0.95, 0.5, dy.d)); y = dy.read()
    O.chk(O.lib().orc_softq_target(ot.h, ob.h, 0.95, 0.5, O.vpz(oy)))
    assert np.abs(y - oy).max() < 1e-5
    dy.fill()
    ctx.check(ctx.lib.crux_dqn_target(gt.h, gb.h, 0.95, dy.d)); y = dy.read()
    O.chk(O.lib().orc_dqn_target(ot.h, ob.h, 0.95, O.vpz(oy)))
    assert np.abs(y - oy).max() < 1e-5
    ctx.h2d(dy.d, oy)
    ctx.check(ctx.lib.crux_td_error(g.h, gb.h, dy.d, de.d)); err = de.read()
    O.chk(O.lib().orc_td_error(o.h, ob.h, O.vpz(oy), O.vpz(oerr)))
    assert np.abs(err - oerr).max() < 1e-5
    g.attach_optimizer(crux.Adam(np.float32(1e-3))); o.adam_init(LR)
    for use_w in (0, 1):
        raw = np.zeros(L.INFO_N, np.float32); oinfo = np.zeros(L.INFO_N, np.float32)
        ctx.check(ctx.lib.crux_td_step(g.h, gb.h, dy.d, use_w, O.vpz(raw))); O.chk(O.lib().orc_td_step(o.h, ob.h, O.vpz(oy), use_w, O.vpz(oinfo)))
        assert abs(raw[0] - oinfo[0]) < 1e-5 * max(1, abs(oinfo[0])) and abs(raw[2] - oinfo[2]) < 1e-5 and abs(raw[1] - oinfo[1]) < 1e-4 * max(1, oinfo[1]), (use_w, raw, oinfo)
        if dense:                                                                  # the dense path leaves the flat gradient in crux_mlp_grads_ptr
            assert np.abs(_grads(g, ctx) - o.grads).max() < 1e-4 * np.abs(o.grads).max()
    dp = np.abs(g.get_params() - o.params)
    assert dp.max() < (5e-4 if dense else 1e-6) and np.mean(dp > 2e-5) <= 1e-3, (dp.max(), np.mean(dp > 2e-5))
    dy.read()                                                                      # the steps read y and wrote nothing around it
    g2, _ = parity.make_pair(dims, acts, 31, 0, "discrete"); g2.attach_optimizer(crux.Adam(np.float32(1e-3)))
    g3, _ = parity.make_pair(dims, acts, 31, 0, "discrete"); g3.attach_optimizer(crux.Adam(np.float32(1e-3)))
    r2, r3 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    for _ in range(2):
        de.fill(); de2.fill()
        ctx.check(ctx.lib.crux_td_error(g2.h, gb.h, dy.d, de.d)); ctx.check(ctx.lib.crux_td_step(g2.h, gb.h, dy.d, 1, O.vpz(r2)))
        ctx.check(ctx.lib.crux_td_step_with_error(g3.h, gb.h, dy.d, 1, de2.d, O.vpz(r3)))
        e2, e3 = de.read(), de2.read()
        assert np.abs(e2 - e3).max() < 1e-6 if dense else np.array_equal(e2, e3)
        assert np.array_equal(g2.get_params(), g3.get_params()) and np.array_equal(r2, r3)
    for d in (dy, de, de2):
        d.free()


# ---------------------------------------------------------------------------------------------------- A. GAIL discriminator step and reward
@pytest.mark.parametrize("od,ad,disc", [(3, 1, False), (4, 2, True)], ids=["continuous", "discrete"])
@pytest.mark.parametrize("n_ex,n_pi", [(1, 1), (200, 100), (300, 5), (5, 300), (300, 300)])
def test_gail_d_step_matches_oracle_on_batch_edges(gpu_ctx, od, ad, disc, n_ex, n_pi):
    """crux_gail_d_step: k_gail_head's two halves are split at n_ex, not at a block boundary -- the expert half ends inside the first trip, inside the second, or is all but
    the whole batch. Non-zero row offsets; the assertions of test_gail_discriminator_step_and_reward_match_oracle."""
    ctx, rng = gpu_ctx, np.random.default_rng(400 + n_ex + 7 * n_pi)
    dims, acts = [ad + od, 32, 1], ["tanh", "identity"]
    g, o = parity.make_pair(dims, acts, 13, 0)
    g.attach_optimizer(crux.Adam(np.float32(1e-3))); o.adam_init(LR)
    gex, oex, _ = _bufs(rng, od, ad, n_ex + 9, disc, ctx); gpi, opi, _ = _bufs(rng, od, ad, n_pi + 5, disc, ctx)
    gi, oi = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    for step in range(3):
        ctx.check(ctx.lib.crux_gail_d_step(g.h, gex.h, 4, n_ex, gpi.h, 2, n_pi, O.vpz(gi)))
        O.chk(O.lib().orc_gail_d_step(o.h, oex.h, 4, n_ex, opi.h, 2, n_pi, O.vpz(oi)))
        assert abs(gi[0] - oi[0]) < 1e-4 * max(1, abs(oi[0])) and abs(gi[1] - oi[1]) < 1e-4 * max(1, abs(oi[1])), (step, gi, oi)
        assert _step_close(g, o, ctx), step
        g.set_params(o.params.copy())            # keep the two trajectories on the same point (Adam moments stay within tolerance)


@pytest.mark.parametrize("n", [1, 300, 64 * 256 + 37])      # one row; two blocks; 37 rows into the second trip of the 64 x 256 grid stride
def test_gail_reward_matches_oracle_beyond_one_grid_stride(gpu_ctx, n):
    """crux_gail_reward: every reward row and the mean against orc_gail_reward; the reward column's rows past `elements` (capacity n + 64) keep the sentinel."""
    ctx, rng, od, ad = gpu_ctx, np.random.default_rng(500 + n), 3, 1
    g, o = parity.make_pair([4, 32, 1], ["tanh", "identity"], 13, 0)
    S, A = crux.ContinuousSpace(od), crux.ContinuousSpace(ad)
    gb = crux.ExperienceBuffer(S, A, n + PAD, ctx=ctx); ob = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, n + PAD)
    d = {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
         "r": np.full((1, n), SENTINEL, np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool)}
    gb.push_(d); ob.push(d)
    assert len(gb) == n and gb.capacity == n + PAD
    tail = C.c_void_p(gb.column_ptr("r") + 4 * n)
    ctx.h2d(tail, np.full(PAD, SENTINEL, np.float32))
    gm, om = np.zeros(1, np.float32), np.zeros(1, np.float32)
    ctx.check(ctx.lib.crux_gail_reward(g.h, gb.h, 0.5, 1.5, O.vpz(gm))); O.chk(O.lib().orc_gail_reward(o.h, ob.h, 0.5, 1.5, O.vpz(om)))
    r, ro = gb["r"][0], ob["r"][0]
    assert r.shape == (n,) and not (r == SENTINEL).any()
    assert np.abs(r - ro).max() < 2e-5 * max(1, np.abs(ro).max()) and abs(gm[0] - om[0]) < 2e-5 * max(1, abs(om[0])), (np.abs(r - ro).max(), gm, om)
    assert (ctx.d2h(tail, np.empty(PAD, np.float32)) == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- A. the NaN gate beyond one stride
@pytest.mark.parametrize("entry", ["double_q_step", "q_step", "td_step"])
def test_nan_in_a_row_of_the_second_trip_is_reported_and_nothing_is_updated(gpu_ctx, entry):
    """B = 300 with y[B-1] = NaN, a row only the second trip of the head's loop reaches: CRUX_ENAN, parameters and Adam moments untouched, beta powers still [0.9, 0.999]
    (the shape of test_sac_nan_is_reported_and_nothing_is_updated; td_step on the dense route)."""
    ctx, rng, B = gpu_ctx, np.random.default_rng(2), 300
    if entry == "td_step":
        g1, _ = parity.make_pair([8, 256, 256, 4], ["relu", "relu", "identity"], 31, 0, "discrete"); nets = [g1]
        gb, _ = _discrete_batch(rng, 8, 4, B, ctx)
    else:
        (_, g1, g2), _, _ = _sac_pair(3, 1, [32], "tanh", ["tanh", "identity"], 9, ctx); nets = [g1, g2] if entry == "double_q_step" else [g1]
        gb, _ = _batch_pair(rng, 3, 1, B, ctx)
    for g in nets:
        g.attach_optimizer(crux.Adam(np.float32(1e-3)))
    d_y = ctx.alloc(4 * B); y = rng.normal(0, 1, B).astype(np.float32); y[B - 1] = np.nan; ctx.h2d(d_y, y)
    before = [(g.get_params(),) + tuple(g.adam_state()) for g in nets]
    with pytest.raises(crux.CruxError) as e:
        if entry == "double_q_step":
            ctx.check(ctx.lib.crux_double_q_step(g1.h, g2.h, gb.h, d_y, 0, None))
        elif entry == "q_step":
            ctx.check(ctx.lib.crux_q_step(g1.h, gb.h, d_y, 0, None))
        else:
            ctx.check(ctx.lib.crux_td_step(g1.h, gb.h, d_y, 0, None))
    assert e.value.code == L.ENAN
    for g, (p, m, v, bp) in zip(nets, before):
        m2, v2, bp2 = g.adam_state()
        assert np.array_equal(g.get_params(), p) and np.array_equal(m2, m) and np.array_equal(v2, v)
        assert np.allclose(bp2, [0.9, 0.999]) and np.array_equal(bp2, bp)
    ctx.free(d_y)


# ---------------------------------------------------------------------------------------------------- B. the B > 256 plans against the oracle
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_offpolicy_teacher_forced_window_at_b320(gpu_ctx, algo):
    """The chained epochs of crux_sac_epochs / crux_dpg_epochs at B = 320 -- the plans without the sequential target + critic-head group (exec.hip: sq = 0) -- against the
    oracle's loop, as test_offpolicy_teacher_forced_windows_at_c4_dims does at B = 256: actor 3-64-64-1, critics 4-64-64-1 (relu), a 2 000-row ring, one window of W = 4
    epochs from the oracle's state at epoch 0. Bound: OFFPOLICY_WINDOW_TOL[0] = 8e-6 (10 x the measured extreme of the 256-wide B = 256 windows), unchanged.
    Measured at B = 320 (largest max |dtheta| over the networks): 3.0e-8 (sac), 1.5e-8 (td3) -- the 64-wide nets of this case are far inside the bound."""
    ctx, rng = gpu_ctx, np.random.default_rng(17)
    B, n, od, ad, nseed, gamma, tau, W = 320, 2000, 3, 1, 9, 0.99, 0.005, 4
    gbuf, obuf = _replay_source(rng, od, ad, n)
    D = crux.buffer_like(gbuf, capacity=B); oD = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, B)
    acts = ["relu", "relu", "identity"]; adims, qdims = [3, 64, 64, 1], [4, 64, 64, 1]
    sac = algo == "sac"
    if sac:
        ga, oa = parity.make_pair(adims, acts, 5, 0, "gaussian", n_extra=1, extra_init=0.0)
    else:
        ga, oa = parity.make_pair(adims, ["relu", "relu", "tanh"], 5, 0)
    g1, o1 = parity.make_pair(qdims, acts, 5, 1); g2, o2 = parity.make_pair(qdims, acts, 5, 2)
    g1t, o1t = parity.make_pair(qdims, acts, 5, 1); g2t, o2t = parity.make_pair(qdims, acts, 5, 2)
    gat, oat = (None, None) if sac else parity.make_pair(adims, ["relu", "relu", "tanh"], 5, 0)
    gla = crux.ParamVector([0.0], ctx=ctx); ola = O.OMlp([0], [], 1); ola.params[:] = 0.0
    lr = float(np.float32(3e-4 if sac else 1e-3))
    trained = [(ga, oa), (g1, o1), (g2, o2)] + ([(gla, ola)] if sac else [])
    for g, o in trained:
        g.attach_optimizer(crux.Adam(np.float32(lr))); o.adam_init(lr)
    targets = [(g1t, o1t), (g2t, o2t)] + ([] if sac else [(gat, oat)])
    pairs = [(g, o, True) for g, o in trained] + [(g, o, False) for g, o in targets]
    sm = (np.float32(0.1), -0.5, 0.5, -1.0, 1.0)
    ol, y, info = O.lib(), np.empty(B, np.float32), np.zeros(L.INFO_N, np.float32)
    _inject(pairs)
    if sac:
        ctx.check(ctx.lib.crux_sac_epochs(ga.h, g1.h, g2.h, None, g1t.h, g2t.h, gla.h, gbuf.h, D.h, gamma, -1.0, tau, 0, 0, W, 1, 1, 0, nseed, 0, None, None, None))
    else:
        ctx.check(ctx.lib.crux_dpg_epochs(ga.h, g1.h, g2.h, gat.h, g1t.h, g2t.h, gbuf.h, D.h, gamma, tau, *[float(x) for x in sm], 0, 0, W, 1, 2, 0, nseed, 0, None, None))
    for e in range(W):
        O.chk(ol.orc_uniform_sample(oD.h, obuf.h, B, None, e, crux.api.SAMPLE_SEED))
        if sac:
            O.chk(ol.orc_sac_target(oa.h, o1t.h, o2t.h, ola.h, oD.h, gamma, nseed, 3 * e, O.vpz(y)))
            O.chk(ol.orc_sac_temp_step(oa.h, ola.h, oD.h, -1.0, nseed, 3 * e + 1, O.vpz(info)))
            O.chk(ol.orc_double_q_step(o1.h, o2.h, oD.h, O.vpz(y), 0, O.vpz(info)))
            O.chk(ol.orc_sac_actor_step(oa.h, o1.h, o2.h, ola.h, oD.h, nseed, 3 * e + 2, O.vpz(info)))
            for t, s in ((o1t, o1), (o2t, o2)):
                O.chk(ol.orc_polyak(t.h, s.h, tau))
        else:
            O.chk(ol.orc_dpg_target(oat.h, o1t.h, o2t.h, oD.h, gamma, *sm, nseed, e, O.vpz(y)))
            O.chk(ol.orc_double_q_step(o1.h, o2.h, oD.h, O.vpz(y), 0, O.vpz(info)))
            if e % 2 == 0:          # TD3's delayed policy update (a_opt.update_every = 2): actor step and target update together (off_policy.jl:96-100)
                O.chk(ol.orc_dpg_actor_step(oa.h, o1.h, oD.h, O.vpz(info)))
                for t, s in ((oat, oa), (o1t, o1), (o2t, o2)):
                    O.chk(ol.orc_polyak(t.h, s.h, tau))
    assert np.array_equal(D["s"], oD["s"]) and np.array_equal(D["r"], oD["r"])          # the last epoch's minibatch: the same rows
    d = [float(np.abs(g.get_params() - o.params).max()) for g, o, _ in pairs]
    print("off-policy window %s at B = 320, W = 4 (max |dtheta| per network): %s" % (algo, ["%.3g" % x for x in d]))
    assert max(d) < OFFPOLICY_WINDOW_TOL[0], d


def test_dqn_epoch_at_b320_prioritized_matches_the_oracle_composition(gpu_ctx):
    """One crux_dqn_epoch at B = 320 on a prioritized ring, 8-256-256-4: the fused epoch without the sequential target + head group (exec.hip: sq0 = 0; update_priorities!,
    leaf re-sum and root paths as phases of their own) against prioritized_sample! -> dqn_target -> td_error -> update_priorities! -> train!(td_loss, weighted) made of
    the oracle's pieces (as tests/test_gpu_fullsize.py::test_c3_full_size_value_training_epochs_replay_oracle composes them). Sampled ids identical, parameters judged by
    _step_close, priorities within 1e-5."""
    ctx, rng = gpu_ctx, np.random.default_rng(2027); N, B, od, ad, gamma, beta = 20_000, 320, 8, 4, 0.99, float(np.float32(0.6))
    dims, acts = [8, 256, 256, 4], ["relu", "relu", "identity"]
    g, o = parity.make_pair(dims, acts, 41, 0, "discrete"); gt, ot = parity.make_pair(dims, acts, 42, 0, "discrete")
    src_g = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad), N, prioritized=True, ctx=ctx)
    src_o = O.OBuffer(od, ad, L.ACTION_DISCRETE, N, prioritized=True, alpha=np.float32(0.6))
    a = np.zeros((ad, N), np.bool_); a[rng.integers(0, ad, N), np.arange(N)] = True
    d = {"s": rng.standard_normal((od, N)).astype(np.float32), "sp": rng.standard_normal((od, N)).astype(np.float32), "r": rng.standard_normal((1, N)).astype(np.float32),
         "done": rng.random((1, N)) < 0.05, "episode_end": rng.random((1, N)) < 0.05, "a": a}
    src_g.push_(d); src_o.push(d)
    I = rng.choice(N, N // 4, replace=False).astype(np.int64); v = np.abs(rng.standard_normal(I.size)) + 1e-3          # a non-trivial priority landscape
    src_g.update_priorities_(I + 1, v); O.chk(O.lib().orc_per_update(src_o.h, O.vpz(I), O.vpz(v), 1, I.size))
    tg = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad), B, ["weight"], ctx=ctx); to = O.OBuffer(od, ad, L.ACTION_DISCRETE, B, ["weight"])
    g.attach_optimizer(crux.Adam(np.float32(1e-3))); o.adam_init(LR)
    oy, oerr, oinfo, raw = np.empty(B, np.float32), np.empty(B, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    ctx.check(ctx.lib.crux_dqn_epoch(g.h, gt.h, src_g.h, tg.h, gamma, 1, beta, 1000, O.vpz(raw)))
    O.chk(O.lib().orc_per_sample(to.h, src_o.h, B, None, beta, 1000, crux.api.SAMPLE_SEED))
    O.chk(O.lib().orc_dqn_target(ot.h, to.h, gamma, O.vpz(oy)))
    O.chk(O.lib().orc_td_error(o.h, to.h, O.vpz(oy), O.vpz(oerr)))
    ids_o = np.empty(B, np.int64); O.chk(O.lib().orc_buffer_indices(to.h, O.vpz(ids_o), B))
    O.chk(O.lib().orc_per_update(src_o.h, O.vpz(ids_o), O.vpz(oerr), 0, B))
    O.chk(O.lib().orc_td_step(o.h, to.h, O.vpz(oy), 1, O.vpz(oinfo)))
    assert np.array_equal(tg.indices[:B], ids_o), "the prioritized search left the oracle's rows"
    assert np.array_equal(tg["s"], to["s"]) and np.array_equal(tg["a"], to["a"])
    assert _step_close(g, o, ctx)
    ppg, maxo, mino = src_g.priority_params(), np.zeros(1, np.float32), np.zeros(1, np.float32)
    pro = np.empty(N, np.float32); O.chk(O.lib().orc_per_get(src_o.h, O.vpz(pro), maxo.ctypes.data_as(C.POINTER(C.c_float)), mino.ctypes.data_as(C.POINTER(C.c_float)), None))
    dpr = np.abs(ppg["priorities"][:N] - pro)
    print("dqn_epoch at B = 320: max |dp| %.3g over the ring, max priority %.6g vs %.6g; loss %.6g vs %.6g" % (dpr.max(), ppg["max_priority"], maxo[0], raw[0], oinfo[0]))
    assert dpr.max() < 1e-5 and abs(ppg["max_priority"] - float(maxo[0])) < 1e-5 * max(1.0, float(maxo[0]))
