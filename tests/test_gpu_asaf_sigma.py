"""GPU: ASAF with a two-headed policy -- crux_asaf_freeze / crux_asaf_actor_step / crux_asaf_batch_train on a handle with the sigma-head flag (csrc/asaf.hip:
k_asaf_logpdf_sigma, k_asaf_head_sigma) and ASAF(..., two_headed=True) (crux.jl_amd/il_on_policy.py) -- against the float64 yardstick of tests/asaf_sigma_reference.py (AS),
which is built on tests/sigma_head_reference.py (SR) and tests/asaf_reference.py.

Tolerances are the project's own (tests/test_gpu_asaf.py, test_gpu_sigma_head.py): 1e-4 relative on the loss, the norm and the steps' values {entropy, expert term, policy
term}, 1e-4 of the gradient scale on the raw gradient, 2e-5 absolute on parameters after one Adam step at lr 1e-3, where entries whose float64 gradient lies within 1e-3 of the
gradient scale of zero are left out (Adam's first step is lr sign(g) there). At most a quarter of the handle may be left out: tests/test_asaf_sigma_reference.py asserts that on
every case with the yardstick alone and this file asserts it again. The freeze (logpdf(pi, s, a) over the rollout rows and the demonstrations) gets an absolute tolerance by
SR.tolerance's rule, four times the largest error of the float32 restatement against float64 over the case's own columns (the margin covers the tile GEMMs' other summation
order and the device's exp / log / tanh / atanh):
    case (shape, n, ascale, N_E)          float32 error logpdf    tolerance    largest device error (MI355X, profiles/cql_asaf_sigma_tests.txt)
    2-32-2x1          37  0       21          3.801e-07               1.520e-06    3.470e-07
    2-32-2x1           1  2        5          1.785e-07               7.138e-07    2.977e-07
    2-32-2x1          37  1    16400          5.823e-06               2.329e-05    4.946e-06
    5-100-100-2x3     37  2       75          3.064e-06               1.226e-05    1.871e-06
    5-100-100-2x3    257  0       21          2.446e-06               9.782e-06    1.423e-06
    4-256-256-2x2    257  2       21          2.976e-06               1.190e-05    1.394e-06
    4-256-256-2x2      1  2       21          3.441e-06               1.376e-05    1.830e-06
    17-256-256-2x6    37  2       75          4.079e-06               1.632e-05    2.160e-06
    5-100-100-2x3     37  1       21          5.880e-05               2.352e-04    9.086e-05
(the last row is the clamp case, SR.case(..., clamp=0): its logSigma rows at -6 make sigma = exp(-5), so (u - mu)^2 / sigma^2 and with it the format's error are large.)
Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

import asaf_sigma_reference as AS
import parity
import sigma_gpu_cases as G
import sigma_head_reference as SR
from parity import crux, L

pytestmark = pytest.mark.gpu
LR = AS.LR
ALL = [(r, None) for r in AS.CASES] + [(AS.CLAMP_CASE, 0)]
IDS = ["%s-n%d-x%g-NE%d%s" % (r + ("" if k is None else "-clamp",)) for r, k in ALL]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _buffer(ctx, c, s, a, extras=()):
    m = s.shape[1]; rng = np.random.default_rng(1)
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), crux.ContinuousSpace(c["ad"]), m, list(extras), ctx=ctx)
    b.push_({"s": s, "a": a, "sp": rng.normal(0, 1, s.shape).astype(np.float32), "r": np.zeros((1, m), np.float32), "done": np.zeros((1, m), bool), "episode_end": np.zeros((1, m), bool)})
    return b


class Setup:
    """the rollout minibatch and the demonstrations of a case on the device; gG (the rollout buffer's :logprob column) and gE (a device array) are the yardstick's numbers"""

    def __init__(self, ctx, c, s=None, sE=None):
        self.b = _buffer(ctx, c, c["s"] if s is None else s, c["a"], extras=("logprob",)); self.demo = _buffer(ctx, c, c["sE"] if sE is None else sE, c["aE"])
        self.gG = self.b.column_ptr("logprob"); ctx.h2d(self.gG, np.ascontiguousarray(c["gG"], np.float32))
        self.gE = crux.il_on_policy._DeviceVec(ctx, c["NE"]); ctx.h2d(self.gE.p, np.ascontiguousarray(c["gE"], np.float32))


def _pi(c, ctx, p=None):
    pi = G.actor(c, ctx, p); pi.attach_optimizer(crux.Adam(np.float32(LR))); return pi


@pytest.mark.parametrize("row,clamp", ALL, ids=IDS)
def test_freeze_matches_the_yardstick(gpu_ctx, row, clamp):
    ctx = gpu_ctx; c = AS.case(*row, clamp); st = Setup(ctx, c); pi = _pi(c, ctx); tol = AS.logpdf_tolerance(c); worst = 0.0
    for b, s, a in ((st.b, c["s"], c["a"]), (st.demo, c["sE"], c["aE"])):
        out = crux.il_on_policy._DeviceVec(ctx, len(b)); crux.asaf_freeze_(pi, b, out.p); got = out.get(); want = SR.logpdf(c, s, a)
        worst = max(worst, float(np.abs(got - want).max())); assert np.isfinite(got).all()
        lp = pi.logpdf(s, a)      # crux_sigma_head_logpdf (SigmaLogpdfOp): the same arithmetic
        assert np.array_equal(_bits(got), _bits(lp[0]))
    print("freeze %-16s n=%-4d ascale=%g N_E=%-5d: float32 error %.3e, tolerance %.3e, device error %.3e" % (row + (AS.logpdf32_error(c), tol, worst)))
    assert worst <= tol
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"]))


def _check_step(ctx, c, clip=None):
    st = Setup(ctx, c); pi = _pi(c, ctx); n = c["B"]
    rinfo, g, p = AS.step(c, clip)
    raw, out = crux.asaf_actor_step_(pi, st.b, 0, n, st.gG, st.demo, st.gE.p, clip_value=clip)
    gg = G.grads(pi, ctx); g_used = AS.AR.clip_value(g, clip); keep = np.abs(g) > 1e-3 * np.abs(g).max(); share = SR.skipped_share(g)
    e_g, e_p = np.abs(gg - g_used).max() / np.abs(g).max(), np.abs(pi.get_params() - p)[keep].max()
    print("step %s n=%d ascale=%g N_E=%d clip %s:" % (c["name"], n, c["ascale"], c["NE"], clip), raw[[0, 1, L.INFO["entropy"]]], out, rinfo,
          "gradient error / scale %.2e, parameters %.2e, left out %.4f" % (e_g, e_p, share))
    assert G.close(raw[L.INFO["loss"]], rinfo["loss"]) and G.close(raw[L.INFO["grad_norm"]], rinfo["grad_norm"]) and G.close(raw[L.INFO["entropy"]], rinfo["entropy"])
    for k, key in enumerate(("entropy", "expert", "policy")):
        assert G.close(out[k], rinfo[key]), (key, out[k], rinfo[key])
    assert e_g <= 1e-4 and share <= 0.25 and e_p <= 2e-5
    return g


@pytest.mark.parametrize("row,clamp", ALL, ids=IDS)
def test_actor_step_matches_float64(gpu_ctx, row, clamp):
    _check_step(gpu_ctx, AS.case(*row, clamp))


@pytest.mark.parametrize("row", [AS.CASES[3], AS.CASES[4]], ids=["squashed", "gaussian"])
def test_clip_value_clamps_after_the_norm(gpu_ctx, row):
    c = AS.case(*row); g = AS.step(c)[1]; clip = float(np.median(np.abs(g[np.abs(g) > 1e-3 * np.abs(g).max()])))
    assert 0.02 < (np.abs(g) > clip).mean() < 0.98      # the clamp is live and not everything
    _check_step(gpu_ctx, c, clip)


def _stub(pi, st, bs, epochs, clip=None, seed=21):
    class _S:
        pass
    sv = _S(); sv.agent = crux.PolicyParams(pi, space=crux.ContinuousSpace(pi.act_dim)); sv.demo, sv.gE, sv.clip_value = st.demo, st.gE, clip
    sv.a_opt = crux.TrainingParams(loss=crux.asaf_loss, optimizer=pi.optimizer, batch_size=bs, epochs=epochs, name="actor_", shuffle_seed=seed)
    return sv


@pytest.mark.parametrize("row", [AS.CASES[5], AS.CASES[4]], ids=["squashed", "gaussian"])
def test_batch_train_is_the_shuffle_and_step_loop(gpu_ctx, row):
    ctx = gpu_ctx; c = AS.case(*row); n, bs, epochs = c["B"], 100, 3; runs = []      # minibatches of 100, 100, 57
    for manual in (False, True):
        st = Setup(ctx, c); pi = _pi(c, ctx)
        if not manual:
            info = crux.batch_train_asaf_(_stub(pi, st, bs, epochs), st.b); rows, total = info["_epoch_infos"], info["actor_batches_trained"]
        else:
            rows, total = [], 0
            for ep in range(epochs):
                crux.shuffle_device_(st.b, 21, ep)
                for k0 in range(0, n, bs):
                    raw, out = crux.asaf_actor_step_(pi, st.b, k0, min(bs, n - k0), st.b.column_ptr("logprob"), st.demo, st.gE.p); total += 1
                rows.append(np.concatenate([raw, out, [0.0]]).astype(np.float32))
            rows = np.stack(rows)
        runs.append((pi.get_params(), rows, total, st.b["s"], st.b["logprob"]) + pi.adam_state())
    a, b = runs
    assert a[2] == b[2] == 9 and a[1].shape == b[1].shape == (3, L.INFO_N + 4)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[5]), _bits(b[5])) and np.array_equal(_bits(a[6]), _bits(b[6])) and np.array_equal(a[7], b[7])
    for k in (L.INFO["loss"], L.INFO["grad_norm"], L.INFO["entropy"], L.INFO_N, L.INFO_N + 1, L.INFO_N + 2):
        assert np.array_equal(_bits(a[1][:, k]), _bits(b[1][:, k])), k
    assert np.array_equal(_bits(a[3]), _bits(b[3])) and np.array_equal(_bits(a[4]), _bits(b[4]))
    assert not np.array_equal(a[0], c["p"]) and np.all(np.isfinite(a[1]))


def test_steps_are_deterministic(gpu_ctx):
    ctx = gpu_ctx; c = AS.case(*AS.CASES[2]); outs = []      # N_E = 16400: the second sweep of the head blocks
    for _ in range(2):
        st = Setup(ctx, c); pi = _pi(c, ctx)
        r1, o1 = crux.asaf_actor_step_(pi, st.b, 0, 37, st.gG, st.demo, st.gE.p, clip_value=0.02)
        r2, o2 = crux.asaf_actor_step_(pi, st.b, 5, 30, st.gG, st.demo, st.gE.p)
        out = crux.il_on_policy._DeviceVec(ctx, c["NE"]); crux.asaf_freeze_(pi, st.demo, out.p)
        outs.append((pi.get_params(), out.get(), r1, o1, r2, o2) + pi.adam_state()[:2])
    assert all(np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])) for k in range(8))
    assert not np.array_equal(outs[0][0], c["p"])


@pytest.mark.parametrize("which", ["roll", "demo"])
@pytest.mark.parametrize("sc", [0.0, 2.0])
def test_nan_state_raises_and_leaves_everything(gpu_ctx, sc, which):
    ctx = gpu_ctx; c = AS.case("5-100-100-2x3", 37, sc, 75)
    s, sE = c["s"].copy(), c["sE"].copy(); (s if which == "roll" else sE)[2, 5] = np.nan
    st = Setup(ctx, c, s=s, sE=sE); pi = _pi(c, ctx); m0, v0, bp0 = pi.adam_state()
    with pytest.raises(L.CruxError) as e:
        crux.asaf_actor_step_(pi, st.b, 0, 37, st.gG, st.demo, st.gE.p)
    assert e.value.code == L.ENAN and "NaN detected" in str(e.value)
    m1, v1, bp1 = pi.adam_state()
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"])) and np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(bp0, bp1) and not m1.any() and not v1.any()
    with pytest.raises(L.CruxError) as e:
        crux.batch_train_asaf_(_stub(pi, st, 37, 3), st.b)
    assert e.value.code == L.ENAN
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"])) and np.array_equal(pi.adam_state()[2], bp0)
    # the freeze of a NaN state is NaN in that row alone (the chain's first shuffle has moved the rollout rows)
    b = st.b if which == "roll" else st.demo; out = crux.il_on_policy._DeviceVec(ctx, len(b)); crux.asaf_freeze_(pi, b, out.p); got = out.get()
    row = np.flatnonzero(np.isnan(b["s"][:, :len(b)]).any(0)); assert row.size == 1
    assert np.isnan(got[row[0]]) and np.isfinite(np.delete(got, row[0])).all()


def test_refusals(gpu_ctx):
    ctx = gpu_ctx; c = AS.case(*AS.CASES[3]); st = Setup(ctx, c); pi = _pi(c, ctx); S = crux.ContinuousSpace(c["od"])
    with pytest.raises(NotImplementedError, match=r"ASAF.*two_headed=True"):
        crux.ASAF(pi, S, st.demo)
    sv = crux.ASAF(pi, S, st.demo, two_headed=True)
    assert sv.agent.space.dims == crux.ContinuousSpace(c["ad"]).dims and sv.a_opt.loss is crux.asaf_loss
    # a handle with neither logSigma extras nor the flag: CRUX_EUNSUP, as before
    det = crux.ContinuousNetwork(parity.chain(list(c["dims"]), list(c["acts"])), ctx=ctx); det.attach_optimizer(crux.Adam(np.float32(LR)))
    for call in (lambda: crux.asaf_actor_step_(det, st.b, 0, 37, st.gG, st.demo, st.gE.p), lambda: crux.asaf_freeze_(det, st.b, st.gG)):
        with pytest.raises(L.CruxError) as e:
            call()
        assert e.value.code == L.EUNSUP
    # a two-headed handle whose rows do not fit the buffer: 2 x 2 rows against ad = 3
    wrong = G.policy([5, 16, 4], ["relu", "identity"], 2, 2.0, ctx); wrong.attach_optimizer(crux.Adam(np.float32(LR)))
    for call in (lambda: crux.asaf_actor_step_(wrong, st.b, 0, 37, st.gG, st.demo, st.gE.p), lambda: crux.asaf_freeze_(wrong, st.b, st.gG)):
        with pytest.raises(L.CruxError) as e:
            call()
        assert e.value.code == L.EINVAL
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"])) and np.array_equal(_bits(st.b["logprob"][0]), _bits(c["gG"]))


def test_solve_on_pendulum(gpu_ctx):
    """solve(ASAF(pi, S, demo, two_headed=True)) on the device Pendulum with a squashed 3-64-64-2x1 actor: two iterations of dN = 256, minibatches of 64. Infos finite, the
    parameters moved, and the buffer's :logprob column (gG, carried through the shuffles) equals a fresh freeze of the policy as it was before the last update"""
    ctx, dN, iters, sc = gpu_ctx, 256, 2, 2.0; acts = ["relu", "relu", "identity"]; rng = np.random.default_rng(12)
    pi = G.policy([3, 64, 64, 2], acts, 1, sc, ctx, seed=2); p0 = pi.get_params().copy()
    sE = rng.normal(0, 1, (3, 75)).astype(np.float32); aE = (sc * np.tanh(0.8 * np.tanh(rng.normal(0, 1, (1, 3)) @ sE) + rng.normal(0, 0.1, (1, 75)))).astype(np.float32)
    demo = crux.ExperienceBuffer(crux.ContinuousSpace(3), crux.ContinuousSpace(1), 75, ctx=ctx)
    demo.push_({"s": sE, "a": aE, "sp": sE, "r": np.zeros((1, 75), np.float32), "done": np.zeros((1, 75), bool), "episode_end": np.zeros((1, 75), bool)})
    S = crux.ContinuousSpace(3)
    sv = crux.ASAF(pi, S, demo, dN=dN, N=iters * dN, max_steps=50, clip_value=1.0, two_headed=True,
                   a_opt={"batch_size": 64, "epochs": 2, "optimizer": crux.Adam(np.float32(LR)), "shuffle_seed": 31})
    frozen, freeze = [], sv.post_batch_callback

    def spy(D, info):
        frozen.append(pi.get_params().copy()); freeze(D, info)
    sv.post_batch_callback = spy
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=3))
    assert len(sv.history) == iters == len(frozen)
    for h in sv.history:
        assert all(np.isfinite(h[k]) for k in ("actor_loss", "actor_grad_norm", "entropy")), h
    assert not np.array_equal(pi.get_params(), p0) and not np.array_equal(frozen[1], frozen[0]) and np.isfinite(pi.get_params()).all()
    a = sv.buffer["a"][:, :len(sv.buffer)]; assert np.abs(a).max() <= sc
    piG = G.policy([3, 64, 64, 2], acts, 1, sc, ctx); piG.set_params(frozen[-1])
    fresh = crux.il_on_policy._DeviceVec(ctx, len(sv.buffer)); crux.asaf_freeze_(piG, sv.buffer, fresh.p)
    assert np.array_equal(_bits(sv.buffer["logprob"][0][:len(sv.buffer)]), _bits(fresh.get()))
