"""GPU: NDA-GAIL-JS on the dense engine (crux_gail_d_batch_train, crux_nda_reward_cost, crux_nda_gail_round in csrc/nda_gail.hip, crux_nda_advantages in
csrc/advantage.hip; crux.NDA_GAIL_JS) against the entries it replaces, bit for bit, and against the float64 restatement of tests/nda_gail_reference.py.

Reference: src/model_free/il/nda_gail_js.jl, src/training.jl:13-55, src/sampler.jl:255-281, src/utils.jl:41-42,140-143. Tolerances are the project's: 1e-4 relative on the
loss and the norm and _step_close (tests/test_gpu_sac.py) for gradient and parameters; 2e-5 max(1, |.|max) on rewards, costs and their statistics (tests/test_gpu_gail.py);
1e-4 of the column's scale on the advantage columns.

Parameters and data come from numpy, so every case runs through the yardstick alone, without a device (hinge_shares() below): the seeds were fixed that way. Share of the
rows with c = max(0, r_nda - r) > 0 under the yardstick, independently initialised D and Dnda, per (shape, data seed):
    3-1-cont [32]        seed 1   133 rows  61.7 %
    4-2-disc [64, 64]    seed 26  205 rows  41.5 %
    17-6-cont [256, 256] seed 2   261 rows  35.2 %
(between a quarter and three quarters: the hinge is live both ways; r is increasing in D_out for every ar in (0, 1), so the share is the same at ar = 0.5 and ar = 0.3. The
output offset of a freshly initialised network moves the share a long way: seed 7 gives 45 %, 90 % and 17 %).
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import nda_gail_reference as R
import parity
from parity import crux, L
from test_gpu_sac import _step_close

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR = 1e-3
SEED = 41
# (od, ad, discrete, hidden, n_expert, n_policy): the shapes of tests/test_gpu_gail.py
SHAPES = [(3, 1, False, [32], 64, 64), (4, 2, True, [64, 64], 100, 128), (17, 6, False, [256, 256], 128, 77)]
IDS = ["3-1-cont", "4-2-disc", "17-6-cont"]
CASE_SEED = {3: 1, 4: 26, 17: 2}      # per obs_dim: fixed through the yardstick (the module docstring)
EXTRAS = ["return", "advantage", "logprob", "cost", "cost_advantage", "cost_return"]
ADV_COLS = ["advantage", "return", "cost_advantage", "cost_return"]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _init(dims, rng):
    """Glorot-uniform weights, small non-negative biases (no relu unit is dead from the start), in the flat Flux order"""
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o))
        out += [rng.uniform(-lim, lim, i * o), np.abs(rng.normal(0, 0.3, o))]
    return np.concatenate(out).astype(np.float32)


def _rows(rng, od, ad, n, disc, shift=0.0):
    """n transitions with two closed episodes and a trailing open one; shift moves the state distribution (demonstrations differ from the rollout)"""
    a = np.eye(ad, dtype=bool)[:, rng.integers(0, ad, n)] if disc else rng.uniform(-1, 1, (ad, n)).astype(np.float32)
    ee = np.zeros((1, n), bool); ee[0, n // 3] = True; ee[0, (2 * n) // 3] = True
    done = ee.copy(); done[0, (2 * n) // 3] = False      # one episode ends without a terminal state
    return {"s": (rng.normal(0, 1, (od, n)) + shift).astype(np.float32), "a": a, "sp": (rng.normal(0, 1, (od, n)) + shift).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": done, "episode_end": ee}


def case(shape, B=None, seed=None):
    """dims, both discriminators' and both critics' parameters, and the three buffers' rows: everything a test and the yardstick need, from numpy alone.
    B: the batch size; the buffers hold 3 B + 9 expert rows and 2 B + 5 policy rows (an epoch ends on the shorter one with a ragged pair)."""
    od, ad, disc, hidden, n_ex, _n_pi = shape
    B = B or n_ex
    rng = np.random.default_rng(CASE_SEED[od] if seed is None else seed)
    dims, acts = [ad + od] + list(hidden) + [1], ["relu"] * len(hidden) + ["identity"]
    vdims, vacts = [od, 64, 64, 1], ["relu", "relu", "identity"]
    return {"od": od, "ad": ad, "disc": disc, "B": B, "dims": dims, "acts": acts, "vdims": vdims, "vacts": vacts,
            "pD": _init(dims, rng), "pN": _init(dims, rng), "pV": _init(vdims, rng), "pVc": _init(vdims, rng),
            "demo": _rows(rng, od, ad, 3 * B + 9, disc, 0.5), "nda": _rows(rng, od, ad, 3 * B + 9, disc, -0.5), "batch": _rows(rng, od, ad, 2 * B + 5, disc)}


def reference_reward_cost(c, alpha_r, pN=None):
    """the yardstick on a case's batch: r, c and the three statistics in float64"""
    b = c["batch"]
    z, zn = R.d_out(c["pD"], c["dims"], c["acts"], b["a"], b["s"]), R.d_out(c["pN"] if pN is None else pN, c["dims"], c["acts"], b["a"], b["s"])
    r, rn = R.reward(z, alpha_r), R.reward(zn, alpha_r); cost = R.hinge_cost(r, rn); ne = float(b["episode_end"].sum())
    return r, rn, cost, (r.mean(), cost.sum() / ne, ne)


def hinge_shares():
    """no device: the share of rows with c > 0 per (shape, alpha_r) (the docstring's table)"""
    return {(i, ar): float((reference_reward_cost(case(sh), ar)[2] > 0).mean()) for i, sh in zip(IDS, SHAPES) for ar in (0.5, 0.3)}


def _net(ctx, dims, acts, p):
    n = crux.ContinuousNetwork(parity.chain(dims, acts), ctx=ctx)
    n.set_params(p); n.attach_optimizer(crux.Adam(np.float32(LR)))
    return n


def _buffer(ctx, c, rows, extras=(), capacity=None):
    A = crux.DiscreteSpace(c["ad"]) if c["disc"] else crux.ContinuousSpace(c["ad"])
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), A, capacity or rows["s"].shape[1], list(extras), ctx=ctx)
    b.push_(rows); return b


class Setup:
    """one set of device objects of a case: D, Dnda, V, Vc, the demonstrations, the negative demonstrations, the batch and two copies of it"""

    def __init__(self, ctx, c):
        self.D, self.N = _net(ctx, c["dims"], c["acts"], c["pD"]), _net(ctx, c["dims"], c["acts"], c["pN"])
        self.V, self.Vc = _net(ctx, c["vdims"], c["vacts"], c["pV"]), _net(ctx, c["vdims"], c["vacts"], c["pVc"])
        self.demo, self.nda = _buffer(ctx, c, c["demo"]), _buffer(ctx, c, c["nda"])
        self.batch = _buffer(ctx, c, c["batch"], EXTRAS)
        self.copyD, self.copyN = _buffer(ctx, c, c["batch"], EXTRAS), _buffer(ctx, c, c["batch"], EXTRAS)


def _host_loop(D, ex, pi, B, epochs, counter, max_batches=None):
    """the composition the chain replaces: shuffle_device_ of both buffers, then crux_gail_d_step per zipped pair; returns the epoch rows and the step count"""
    ctx, rows, total = D.ctx, [], 0
    for ep in range(epochs):
        crux.shuffle_device_(ex, SEED, 2 * (counter + ep)); crux.shuffle_device_(pi, SEED, 2 * (counter + ep) + 1)
        raw = np.zeros(L.INFO_N, np.float32)
        for (_e, oe, ne, op, np_) in R.partition_plan(len(ex), len(pi), B, 1):
            ctx.check(ctx.lib.crux_gail_d_step(D.h, ex.h, oe, ne, pi.h, op, np_, _vp(raw))); total += 1
            if max_batches and total >= max_batches:
                break
        rows.append(raw)
        if max_batches and total >= max_batches:
            break
    return np.array(rows), total


def _chain(D, ex, pi, B, epochs, counter, max_batches=0):
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((epochs, L.INFO_N), np.float32)
    D.ctx.check(D.ctx.lib.crux_gail_d_batch_train(D.h, ex.h, pi.h, B, epochs, max_batches, SEED, counter, _vp(raw), _vp(rows)))
    return raw, rows


# ---- 1. the chain against the host loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batches", [0, 5], ids=["all", "stop-in-epoch-2"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chain_is_the_host_loop(gpu_ctx, shape, max_batches):
    c = case(shape); B = c["B"]
    a, b = Setup(gpu_ctx, c), Setup(gpu_ctx, c)
    assert len(R.partition_plan(len(a.demo), len(a.copyD), B, 1)) == 3      # 3 pairs per epoch: max_batches = 5 stops inside epoch 2
    raw, rows = _chain(a.D, a.demo, a.copyD, B, 3, 11, max_batches)
    want, total = _host_loop(b.D, b.demo, b.copyD, B, 3, 11, max_batches or None)
    e = want.shape[0]
    assert raw[L.INFO["batches_trained"]] == total == (max_batches or 9) and raw[L.INFO["epochs_run"]] == e == (2 if max_batches else 3)
    assert _same(rows[:e, :2], want[:, :2]) and np.all(rows[e:] == 0) and np.isfinite(want[:, :2]).all() and np.all(want[:, 1] > 0)
    assert _same(raw[:2], want[-1, :2])
    assert _same(a.D.get_params(), b.D.get_params()) and not _same(a.D.get_params(), c["pD"])
    for x, y in zip(a.D.adam_state(), b.D.adam_state()):
        assert np.array_equal(x, y)
    for k in ("s", "a"):      # both buffers were left in the same (last shuffle's) order
        assert np.array_equal(a.demo[k], b.demo[k]) and np.array_equal(a.copyD[k], b.copyD[k])
    r1, r2 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)      # a further identical step on both: the Adam state carries on identically
    gpu_ctx.check(gpu_ctx.lib.crux_gail_d_step(a.D.h, a.demo.h, 1, 33, a.copyD.h, 2, 21, _vp(r1))); gpu_ctx.check(gpu_ctx.lib.crux_gail_d_step(b.D.h, b.demo.h, 1, 33, b.copyD.h, 2, 21, _vp(r2)))
    assert _same(r1, r2) and _same(a.D.get_params(), b.D.get_params())


# ---- 2. the chain's first step against the yardstick ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chain_first_step_matches_reference(gpu_ctx, shape):
    """one epoch, one pair: buffers of n_expert and n_policy rows under a batch size that covers both"""
    od, ad, disc, hidden, n_ex, n_pi = shape
    c = case(shape); rng = np.random.default_rng(3)
    ex, pi = _buffer(gpu_ctx, c, _rows(rng, od, ad, n_ex, disc, 0.5)), _buffer(gpu_ctx, c, _rows(rng, od, ad, n_pi, disc))
    D = _net(gpu_ctx, c["dims"], c["acts"], c["pD"])
    raw, rows = _chain(D, ex, pi, max(n_ex, n_pi), 1, 0)
    assert raw[L.INFO["batches_trained"]] == 1 and raw[L.INFO["epochs_run"]] == 1 and _same(raw[:2], rows[0, :2])
    loss, g = R.d_step(c["pD"], c["dims"], c["acts"], ex["a"], ex["s"], pi["a"], pi["s"])      # a mean over each half: the shuffled order does not matter
    gn = np.linalg.norm(g)
    print("first step %s: loss %.8g (%.8g) norm %.8g (%.8g)" % (shape[:3], raw[0], loss, raw[1], gn))
    assert abs(raw[0] - loss) < 1e-4 * max(1, abs(loss)) and abs(raw[1] - gn) < 1e-4 * max(1, abs(gn))
    o = types.SimpleNamespace(grads=g.astype(np.float32), params=R.adam_first_step(c["pD"].astype(np.float64), g, lr=LR).astype(np.float32))
    assert _step_close(D, o, gpu_ctx)


# ---- 3. reward and cost ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_r", [0.5, 0.3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reward_cost_matches_gail_reward_and_reference(gpu_ctx, shape, alpha_r):
    c = case(shape); st = Setup(gpu_ctx, c)
    r64, rn64, c64, (m_r, m_c, n_ee) = reference_reward_cost(c, alpha_r)
    share = (c64 > 0).mean()
    assert 0.25 <= share <= 0.75, share      # the hinge is live both ways
    out = crux.nda_reward_cost_(st.D, st.N, st.batch, alpha_r)
    mean_r = crux.gail_reward_(st.D, st.copyD, alpha_r, 1.0)
    assert _same(st.batch["r"], st.copyD["r"]) and _same(np.float32(out[0]), np.float32(mean_r))
    r, cost = st.batch["r"][0].astype(np.float64), st.batch["cost"][0].astype(np.float64)
    tr, tc = 2e-5 * max(1, np.abs(r64).max()), 2e-5 * max(1, np.abs(c64).max())
    near = np.abs(rn64 - r64) < 2e-5      # rows on the hinge's kink: c is 0 on one side and the difference on the other, compared by absolute error only
    print("reward/cost %s ar %.1f: share %.3f, |r - ref| %.3g (tol %.3g), |c - ref| %.3g (tol %.3g), %d rows on the kink, out3 %s ref %s" % (
        shape[:3], alpha_r, share, np.abs(r - r64).max(), tr, np.abs(cost - c64).max(), tc, near.sum(), out, (m_r, m_c, n_ee)))
    assert np.abs(r - r64).max() < tr
    assert np.abs(cost - c64)[~near].max() < tc
    assert near.sum() == 0 or np.abs(cost - c64)[near].max() < tc
    assert abs(out[0] - m_r) < 2e-5 * max(1, abs(m_r)) and abs(out[1] - m_c) < 2e-5 * max(1, abs(m_c)) and out[2] == n_ee == 2.0
    assert np.all(cost >= 0)


def test_dnda_equal_to_d_gives_zero_cost_and_finite_cost_advantage(gpu_ctx):
    c = case(SHAPES[2]); st = Setup(gpu_ctx, c)
    st.N.set_params(c["pD"])
    out = crux.nda_reward_cost_(st.D, st.N, st.batch, 0.3)
    assert np.all(st.batch["cost"] == 0) and out[1] == 0.0 and np.isfinite(st.batch["r"]).all()
    out2 = crux.nda_reward_cost_(st.D, st.D, st.copyD, 0.3)      # the same handle twice
    assert np.all(st.copyD["cost"] == 0) and _same(st.copyD["r"], st.batch["r"]) and out2 == out
    crux.nda_advantages_(st.batch, st.V, st.Vc, 0.95, 0.99)
    ca = st.batch["cost_advantage"][0]
    assert np.isfinite(ca).all() and np.abs(ca).max() > 0.1 and np.all(st.batch["cost_return"] == 0)      # the GAE of a zero cost is -Vc's TD error: whitened, not 0 / 0


def test_no_episode_end_gives_the_float32_quotient(gpu_ctx):
    c = case(SHAPES[0]); c["batch"]["episode_end"][:] = False
    st = Setup(gpu_ctx, c)
    out = crux.nda_reward_cost_(st.D, st.N, st.batch, 0.5)
    assert out[2] == 0.0 and np.isinf(out[1]) and out[1] > 0 and np.isfinite(out[0])      # sum(c) / 0 with sum(c) > 0


def test_nan_input_propagates_to_reward_and_cost_without_an_error(gpu_ctx):
    c = case(SHAPES[1]); c["batch"]["s"][2, 17] = np.nan
    st = Setup(gpu_ctx, c)
    out = crux.nda_reward_cost_(st.D, st.N, st.batch, 0.5)
    r, cost = st.batch["r"][0], st.batch["cost"][0]; ok = np.arange(r.size) != 17
    assert np.isnan(r[17]) and np.isnan(cost[17]) and np.isfinite(r[ok]).all() and np.isfinite(cost[ok]).all() and np.isnan(out[0]) and np.isnan(out[1])


# ---- 4. the advantage tail ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_advantages_are_the_six_calls_and_match_reference(gpu_ctx, shape):
    c = case(shape); st = Setup(gpu_ctx, c); lam, gamma = 0.95, 0.99
    crux.nda_reward_cost_(st.D, st.N, st.batch, 0.5); crux.nda_reward_cost_(st.D, st.N, st.copyD, 0.5)
    crux.nda_advantages_(st.batch, st.V, st.Vc, lam, gamma)
    b, lib = st.copyD, gpu_ctx.lib
    gpu_ctx.check(lib.crux_fill_gae(b.h, st.V.h, lam, gamma)); gpu_ctx.check(lib.crux_fill_returns(b.h, gamma))
    gpu_ctx.check(lib.crux_fill_gae_keys(b.h, st.Vc.h, lam, gamma, L.COL["cost"], L.COL["cost_advantage"])); gpu_ctx.check(lib.crux_fill_returns_keys(b.h, gamma, L.COL["cost"], L.COL["cost_return"]))
    gpu_ctx.check(lib.crux_whiten(b.h, L.COL["advantage"])); gpu_ctx.check(lib.crux_whiten(b.h, L.COL["cost_advantage"]))
    for k in ADV_COLS:
        assert _same(st.batch[k], b[k]), k
    d = c["batch"]; v = lambda p, x: R.mlp(R.mlp_params(p, c["vdims"]), c["vacts"], R._t(x))[0].detach().numpy()
    adv, ret = R.gae_returns(st.batch["r"][0], d["done"], d["episode_end"], v(c["pV"], d["s"]), v(c["pV"], d["sp"]), lam, gamma)
    cadv, cret = R.gae_returns(st.batch["cost"][0], d["done"], d["episode_end"], v(c["pVc"], d["s"]), v(c["pVc"], d["sp"]), lam, gamma)
    for k, want in (("advantage", R.whiten(adv)), ("return", ret), ("cost_advantage", R.whiten(cadv)), ("cost_return", cret)):
        dev = np.abs(st.batch[k][0] - want).max() / np.abs(want).max()
        print("advantages %s %s: %.3g of the scale %.3g" % (shape[:3], k, dev, np.abs(want).max()))
        assert dev < 1e-4, (k, dev)


# ---- 5. the round against its parts ---------------------------------------------------------------------------------------------------------------------------------
def _round(st, B, eD, eN, cD, cN, mbD=0, mbN=0, alpha_r=0.3, lam=0.95, gamma=0.99):
    rD, rN, out3 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
    rc = st.D.ctx.lib.crux_nda_gail_round(st.D.h, st.N.h, st.demo.h, st.nda.h, st.batch.h, st.copyD.h, st.copyN.h, st.V.h, st.Vc.h, B, eD, mbD, SEED, cD, B, eN, mbN, SEED + 1, cN,
                                         alpha_r, lam, gamma, _vp(rD), _vp(rN), _vp(out3))
    return rc, rD, rN, out3


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_round_is_its_parts_in_turn(gpu_ctx, shape):
    c = case(shape); B = c["B"]; a, b = Setup(gpu_ctx, c), Setup(gpu_ctx, c)
    for k in ("r", "s"):      # stale copies: the round refills them from the batch
        a.copyD[k] = np.zeros_like(a.copyD[k]); a.copyN[k] = np.ones_like(a.copyN[k])
    rc, rD, rN, out3 = _round(a, B, 2, 3, 5, 9, mbN=7)
    gpu_ctx.check(rc)
    wD, _ = _chain(b.D, b.demo, b.copyD, B, 2, 5)
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((3, L.INFO_N), np.float32)
    gpu_ctx.check(gpu_ctx.lib.crux_gail_d_batch_train(b.N.h, b.nda.h, b.copyN.h, B, 3, 7, SEED + 1, 9, _vp(raw), _vp(rows)))
    w3 = crux.nda_reward_cost_(b.D, b.N, b.batch, 0.3); crux.nda_advantages_(b.batch, b.V, b.Vc, 0.95, 0.99)
    assert _same(rD, wD) and _same(rN, raw) and rN[L.INFO["batches_trained"]] == 7 and rD[L.INFO["batches_trained"]] == 6
    assert _same(out3, np.array(w3, np.float32))
    for x, y in ((a.D, b.D), (a.N, b.N)):
        assert _same(x.get_params(), y.get_params())
        for u, w in zip(x.adam_state(), y.adam_state()):
            assert np.array_equal(u, w)
    assert not _same(a.D.get_params(), c["pD"]) and not _same(a.N.get_params(), c["pN"])
    for k in ["r", "cost"] + ADV_COLS:
        assert _same(a.batch[k], b.batch[k]) and np.isfinite(a.batch[k]).all(), k
    for k in ("s", "a", "sp", "done", "episode_end"):      # the batch keeps its row order: only the copies were shuffled
        assert np.array_equal(a.batch[k], c["batch"][k]), k
    assert not np.array_equal(a.copyD["s"], c["batch"]["s"]) and np.array_equal(np.sort(a.copyD["s"], axis=1), np.sort(c["batch"]["s"], axis=1))
    assert np.array_equal(a.copyD["s"], b.copyD["s"]) and np.array_equal(a.copyN["s"], b.copyN["s"]) and len(a.copyD) == len(a.batch)


# ---- 6. NaN -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_nan_in_the_demonstrations_stops_the_round(gpu_ctx):
    """fed data only: one NaN entry of the demonstrations' :s. The host loop on a second set shows which step meets it and what D held before that step. Row 48 of the 201
    sits at row 194 after the first epoch's shuffle (behind the 192 rows the three pairs read) and at row 97 after the second's: the fifth step meets it."""
    c = case(SHAPES[0]); B = c["B"]; c["demo"]["s"][1, 48] = np.nan
    a, b = Setup(gpu_ctx, c), Setup(gpu_ctx, c)
    r0 = a.batch["r"].copy(); cols0 = {k: a.batch[k].copy() for k in ["cost"] + ADV_COLS}
    rc, rD, rN, out3 = _round(a, B, 3, 2, 0, 0)
    assert rc == L.ENAN and "NaN detected" in (gpu_ctx.lib.crux_last_error(gpu_ctx.h) or b"").decode()
    with pytest.raises(L.CruxError) as ei:
        _host_loop(b.D, b.demo, b.copyD, B, 3, 0)
    assert ei.value.code == L.ENAN
    assert _same(a.D.get_params(), b.D.get_params()) and not _same(a.D.get_params(), c["pD"])      # what D held before the step that saw the NaN (the host loop stopped there), four steps in
    assert rD[L.INFO["batches_trained"]] == 9 and rD[L.INFO["epochs_run"]] == 3      # everything was enqueued; the steps after the stop changed nothing
    assert np.isnan(rD[L.INFO["grad_norm"]])
    assert _same(a.N.get_params(), c["pN"]) and _same(a.batch["r"], r0)
    for k, v in cols0.items():
        assert _same(a.batch[k], v), k
    # the chain alone: the same stop, the row of the step that stopped
    a2 = Setup(gpu_ctx, c); raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((3, L.INFO_N), np.float32)
    rc = gpu_ctx.lib.crux_gail_d_batch_train(a2.D.h, a2.demo.h, a2.copyD.h, B, 3, 0, SEED, 0, _vp(raw), _vp(rows))
    assert rc == L.ENAN and np.isnan(raw[L.INFO["grad_norm"]]) and _same(a2.D.get_params(), b.D.get_params()) and _same(raw[:2], rD[:2])


def test_nan_in_the_negative_demonstrations_names_the_second_chain(gpu_ctx):
    """the other branch of the round's report: D's chain is clean, Dnda's meets the NaN. Ten rows of the negative demonstrations' :s hold one; an epoch's three pairs read
    192 of the 201 rows, so at most nine of them sit behind what the first epoch reads. D ends where the host loop over all of its epochs ends, its row is that loop's
    last, and the message names nda_discriminator."""
    c = case(SHAPES[0]); B = c["B"]; c["nda"]["s"][1, 40:50] = np.nan
    a, b = Setup(gpu_ctx, c), Setup(gpu_ctx, c)
    r0 = a.batch["r"].copy()
    rc, rD, rN, out3 = _round(a, B, 3, 2, 0, 0)
    msg = (gpu_ctx.lib.crux_last_error(gpu_ctx.h) or b"").decode()
    assert rc == L.ENAN and "NaN detected" in msg and "nda_discriminator epoch 1" in msg and "the batch is not rewritten" in msg, msg
    rows, total = _host_loop(b.D, b.demo, b.copyD, B, 3, 0)
    assert total == 9 and _same(a.D.get_params(), b.D.get_params()) and _same(rD[:2], rows[-1][:2]) and np.isfinite(rD[L.INFO["grad_norm"]])
    assert rD[L.INFO["batches_trained"]] == 9 and rD[L.INFO["epochs_run"]] == 3
    assert np.isnan(rN[L.INFO["grad_norm"]]) and rN[L.INFO["epochs_run"]] == 2
    assert _same(a.batch["r"], r0)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_without_a_launch(gpu_ctx):
    c = case(SHAPES[0]); st = Setup(gpu_ctx, c); lib = gpu_ctx.lib; out = np.zeros(3, np.float32)
    r0, p0 = st.batch["r"].copy(), st.D.get_params().copy()

    def refused(rc, word):
        msg = (lib.crux_last_error(gpu_ctx.h) or b"").decode()
        assert rc == L.EINVAL and word in msg, (rc, msg)
    wide = _net(gpu_ctx, [c["ad"] + c["od"] + 1, 32, 1], ["relu", "identity"], _init([c["ad"] + c["od"] + 1, 32, 1], np.random.default_rng(0)))
    two = _net(gpu_ctx, [c["ad"] + c["od"], 32, 2], ["relu", "identity"], _init([c["ad"] + c["od"], 32, 2], np.random.default_rng(0)))
    refused(lib.crux_nda_reward_cost(wide.h, st.N.h, st.batch.h, 0.5, _vp(out)), "must map vcat(a, s)")
    refused(lib.crux_nda_reward_cost(st.D.h, two.h, st.batch.h, 0.5, _vp(out)), "must map vcat(a, s)")
    other = crux.Context(0)
    alien = _net(other, c["dims"], c["acts"], c["pN"])
    refused(lib.crux_nda_reward_cost(st.D.h, alien.h, st.batch.h, 0.5, _vp(out)), "different contexts")
    refused(lib.crux_nda_reward_cost(st.D.h, st.N.h, st.demo.h, 0.5, _vp(out)), "no :cost column")
    A = crux.ContinuousSpace(c["ad"]); empty = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), A, 8, EXTRAS, ctx=gpu_ctx)
    refused(lib.crux_nda_reward_cost(st.D.h, st.N.h, empty.h, 0.5, _vp(out)), "empty buffer")
    raw = np.zeros(L.INFO_N, np.float32)
    refused(lib.crux_gail_d_batch_train(st.D.h, st.demo.h, st.copyD.h, 0, 1, 0, SEED, 0, _vp(raw), None), "out of range")
    refused(lib.crux_gail_d_batch_train(st.D.h, st.demo.h, empty.h, 64, 1, 0, SEED, 0, _vp(raw), None), "empty policy buffer")
    refused(lib.crux_gail_d_batch_train(wide.h, st.demo.h, st.copyD.h, 64, 1, 0, SEED, 0, _vp(raw), None), "must map vcat(a, s)")
    refused(lib.crux_nda_advantages(st.demo.h, st.V.h, st.Vc.h, 0.95, 0.99), "lacks column")
    refused(lib.crux_nda_advantages(st.batch.h, st.D.h, st.Vc.h, 0.95, 0.99), "must map obs")
    small = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), A, 8, EXTRAS, ctx=gpu_ctx)
    keep = st.copyN; st.copyN = small
    refused(_round(st, 64, 1, 1, 0, 0)[0], "copyN must be a plain buffer")
    st.copyN = keep; keepN = st.N; st.N = st.D
    refused(_round(st, 64, 1, 1, 0, 0)[0], "same handle")
    st.N = keepN
    assert _same(st.batch["r"], r0) and _same(st.D.get_params(), p0) and len(small) == 0


# ---- 8. the solver ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_nda_gail_solve_runs_and_trains_both_discriminators(gpu_ctx):
    """NDA_GAIL_JS on Pendulum with demonstrations from the committed recording (negative demonstrations: the same states with the action's sign flipped): LagrangePPO +
    the round, end to end. Mechanics only, no return threshold. lagrange_ppo_loss estimates the episode cost as sum(cost) / sum(episode_end) of EVERY minibatch (ppo.jl:86)
    and a minibatch without an episode end is a NaN loss there as here, so the episodes are short: max_steps = 8 puts 32 episode ends into the 256 rows."""
    ctx = gpu_ctx
    d = dict(np.load(os.path.join(GOLD, "pendulum_transitions.npz")))
    n = d["s"].shape[1]; S, A = crux.ContinuousSpace(3), crux.ContinuousSpace(1)
    obs3 = lambda x: np.vstack([np.cos(x[0]), np.sin(x[0]), x[1]]).astype(np.float32)      # the recording stores (theta, omega); the device env observes (cos, sin, omega)
    rows = {"s": obs3(d["s"]), "sp": obs3(d["sp"]), "a": d["a"], "r": d["r"], "done": d["done"], "episode_end": np.zeros((1, n), bool)}
    demo = crux.ExperienceBuffer(S, A, n, ctx=ctx); demo.push_(rows)
    nda = crux.ExperienceBuffer(S, A, n, ctx=ctx); nda.push_(dict(rows, a=-d["a"]))
    acts = ["relu", "relu", "identity"]
    pi = crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 64, 64, 1], acts), np.zeros(1, np.float32), seed=1, ctx=ctx), crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=2, ctx=ctx))
    Vc = crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=5, ctx=ctx)
    Dn, Nn = crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=3, ctx=ctx), crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=4, ctx=ctx)
    p0, n0, v0 = Dn.get_params().copy(), Nn.get_params().copy(), Vc.get_params().copy()
    opt = {"epochs": 2, "batch_size": 128}
    sv = crux.NDA_GAIL_JS(pi, S, demo, nda, Vc, 0.99, Dn, Nn, N=3 * 256, dN=256, max_steps=8, normalize_demo=False, a_opt=dict(opt), c_opt=dict(opt), cost_opt=dict(opt),
                          d_opt=dict(opt), d_opt_nda=dict(opt), target_kl=None)
    assert sv.d_opt.name == "discriminator_" and sv.d_opt_nda.name == "nda_discriminator_" and sv.Vc is Vc
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    assert len(sv.history) == 3
    for net, q in ((Dn, p0), (Nn, n0), (Vc, v0)):
        assert not np.array_equal(net.get_params(), q) and np.isfinite(net.get_params()).all()
    assert np.isfinite(pi.A.get_params()).all()
    assert sv.d_opt.shuffle_counter == 3 * 2 and sv.d_opt_nda.shuffle_counter == 3 * 2
    for k in ("discriminator_loss", "discriminator_grad_norm", "discriminator_batches_trained", "nda_discriminator_loss", "nda_discriminator_grad_norm", "nda_discriminator_batches_trained",
              "disc_reward", "disc_nda_cost"):
        assert k in sv.history[-1] and np.isfinite(sv.history[-1][k]), k
    assert sv.history[-1]["discriminator_batches_trained"] == 4 and sv.history[-1]["nda_discriminator_batches_trained"] == 4
    # the discriminators did not change after the callback: :r and :cost recompute from them
    x = np.vstack([sv.buffer["a"], sv.buffer["s"]])
    z, zn = Dn.forward(x)[0].astype(np.float64), Nn.forward(x)[0].astype(np.float64)
    r, rn = R.reward(z, 0.5), R.reward(zn, 0.5)
    assert np.abs(sv.buffer["r"][0] - r).max() < 1e-5 and np.abs(sv.buffer["cost"][0] - R.hinge_cost(r, rn)).max() < 1e-5
    assert len(demo) == n and np.array_equal(demo["a"], d["a"])      # the caller's buffers were copied, not shuffled
