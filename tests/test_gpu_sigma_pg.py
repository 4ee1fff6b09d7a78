"""GPU: the policy-gradient learners on two-headed Gaussian actors -- ppo_loss, a2c_loss, reinforce_loss and logpdf_bc_loss of GaussianPolicy / SquashedGaussianPolicy whose
logSigma is a network on mu's trunk (csrc/train_dense.hip: k_pg_head_sigma, k_pg_info_sigma; the routing and refusals of csrc/train.hip) -- against the float64 yardstick of
tests/sigma_pg_reference.py, and the chained calls, the pair call, the refusals and the solvers against each other.

Tolerances are the project's own (tests/test_gpu_sigma_head.py): 1e-4 relative on loss, entropy, kl and norm, 1e-4 of the gradient scale on the raw gradient
(crux_mlp_grads_ptr), 2e-5 absolute on the parameters after one Adam step at lr 1e-3, where parameters whose float64 gradient lies within 1e-3 of the gradient scale of zero
are left out (Adam's first step is lr sign(g) there); at most a quarter may be left out -- tests/test_sigma_pg_reference.py asserts that with the yardstick alone, this file on
the share it sees. Every test prints its figures before it asserts.

Dispatch: a 3-64-64-2 two-headed actor has the dimensions of an instantiated register-resident learner shape and must still train on the dense engine at batch_size = 128
(the register-resident kernels read constant logSigma extras this handle does not have: their result could not match the yardstick). The constant-logSigma 3-64-64-1 handle
keeps its path: launch_train is entered as before for every handle without the flag, which the existing tests (test_gpu_ppo_parity.py, test_gpu_fs2*.py, smoke) pin bit for bit
against the oracle; it is not repeated here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import parity
import replica_group as RG
import sigma_head_reference as SR
import sigma_pg_reference as PR
from parity import crux, L, O

pytestmark = pytest.mark.gpu
LR = 1e-3
vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
CASES = PR.STEP_CASES
IDS = ["%s-B%d-a%g%s" % (n, B, sc, "" if k is None else "-clamp%d" % k) for n, B, sc, k in CASES]


@functools.lru_cache(maxsize=None)
def _batch(name, B, sc, kind, clamp=None):
    return PR.batch(name, B, sc, kind, clamp)


@functools.lru_cache(maxsize=None)
def _ref_step(name, B, sc, kind, clamp=None):
    return PR.pg_step(_batch(name, B, sc, kind, clamp), kind, lr=LR)


def _policy(dims, acts, ad, sc, ctx, **kw):
    base = [crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(dims) - 2)]
    mu, ls = crux.Chain(*base, crux.Dense(dims[-2], ad)), crux.Chain(*base, crux.Dense(dims[-2], ad))
    return crux.SquashedGaussianPolicy(mu, ls, sc, ctx=ctx, **kw) if sc > 0 else crux.GaussianPolicy(mu, ls, ctx=ctx, **kw)


def _actor(c, ctx, lr=LR):
    pi = _policy(c["dims"], c["acts"], c["ad"], c["ascale"], ctx); pi.set_params(c["p"]); pi.attach_optimizer(crux.Adam(np.float32(lr))); return pi


def _buffer(c, ctx, extras=("return", "logprob", "advantage")):
    B = c["B"]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), crux.ContinuousSpace(c["ad"]), B, list(extras), ctx=ctx)
    d = {"s": c["s"], "a": c["a"], "sp": c["sp"], "r": c["r"].reshape(1, B), "done": c["done"].reshape(1, B), "episode_end": np.zeros((1, B), bool)}
    d.update({k: np.asarray(c[k], np.float32).reshape(1, B) for k in extras})
    b.push_(d); return b


def _cfg(c, kind, bs=None, epochs=1, **kw):
    return parity.train_cfg(PR.LOSS_OF[kind], "gaussian", c["B"] if bs is None else bs, epochs, eps=c["eps_clip"], lp=c["lambda_p"], le=c["lambda_e"], **kw)


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _grads(net, ctx):
    g = np.empty(net.n_params, np.float32); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def _state(pi):
    m, v, bp = pi.adam_state()
    return [pi.get_params().view(np.uint32), np.asarray(m).view(np.uint32), np.asarray(v).view(np.uint32), np.asarray(bp, np.float64)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _info_close(raw, rinfo, kind):
    keys = ["loss", "entropy", "kl", "grad_norm"] + (["clip_fraction", "avg_advantage", "avg_return"] if kind == "ppo" else [])
    return all(_close(raw[L.INFO[k]], rinfo[k]) for k in keys)


def _call(ctx, fn, pi, b, cfg, ids):
    raw = np.zeros(L.INFO_N, np.float32); ids = np.ascontiguousarray(ids, np.int64)
    ctx.check(fn(pi.h, b.h, C.byref(cfg), vp(ids), ids.size, vp(raw))); return raw


# ---- 1. gradient and step parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_loss_grad_and_train_step_match_float64(gpu_ctx, case, kind):
    """crux_loss_grad (info, raw gradient, nothing moves) and crux_train_step (info, parameters after one Adam step) against the yardstick"""
    ctx = gpu_ctx; name, B, sc, clamp = case; c = _batch(name, B, sc, kind, clamp); pi, b = _actor(c, ctx), _buffer(c, ctx); cfg = _cfg(c, kind); ids = np.arange(B)
    rinfo, g, p = _ref_step(name, B, sc, kind, clamp); share = PR.skipped_share(g); before = _state(pi)
    raw = _call(ctx, ctx.lib.crux_loss_grad, pi, b, cfg, ids); gg = _grads(pi, ctx); untouched = _same(_state(pi), before)
    raw2 = _call(ctx, ctx.lib.crux_train_step, pi, b, cfg, ids)
    e_g = np.abs(gg - g).max() / np.abs(g).max(); keep = np.abs(g) > 1e-3 * np.abs(g).max(); e_p = np.abs(pi.get_params() - p)[keep].max()
    print("%s %s:" % (IDS[CASES.index(case)], kind), raw[:7], {k: v for k, v in rinfo.items() if np.isscalar(v)}, "gradient error / scale %.2e, parameters %.2e, left out %.4f" % (e_g, e_p, share))
    assert untouched and np.array_equal(raw.view(np.uint32), raw2.view(np.uint32))
    assert _info_close(raw, rinfo, kind)
    assert e_g <= 1e-4 and share <= 0.25 and e_p <= 2e-5


ROLLOUTS = [("3-64-64-2x1", "pendulum", 2.0), ("3-64-64-2x1-tanh", "pendulum", 0.0), ("17-256-256-2x6", "synth", 1.0)]


@pytest.mark.parametrize("row", ROLLOUTS, ids=[r[0] for r in ROLLOUTS])
def test_rollout_head_and_learner_head_agree(gpu_ctx, row):
    """the first-minibatch kl = mean(:logprob - logpdf(s, a)) of a buffer whose :logprob the rollout kernel wrote: 0 within the shape's logprob tolerance"""
    name, kind, sc = row; ctx = gpu_ctx; dims, acts, ad = SR.SHAPES[name]; E, T = 4, 32; n = E * T
    pi = _policy(dims, acts, ad, sc, ctx, seed=13, stream=0); pi.attach_optimizer(crux.Adam(np.float32(LR)))
    mdp = crux.PendulumMDP(n_envs=E, seed=5) if kind == "pendulum" else crux.SynthMDP(dims[0], ad, n_envs=E, seed=5)
    buf = crux.ExperienceBuffer(mdp.state_space(), mdp.action_space(), n, ["logprob", "return"], ctx=ctx)
    smp = crux.Sampler(mdp, pi, max_steps=100, required_columns=["logprob"])
    crux.steps_(smp, buf, Nsteps=n, explore=True, i=0)
    cfg = parity.train_cfg("reinforce", "gaussian", n, 1); tol = SR.tolerance(name)[0]
    raw = _call(ctx, ctx.lib.crux_loss_grad, pi, buf, cfg, np.arange(n))
    lp = pi.logpdf(buf["s"], buf["a"]); worst = np.abs(lp[0] - buf["logprob"][0]).max()
    print("%s ascale %g: kl %.3e, largest |logprob - logpdf| %.3e (tolerance %.3e)" % (name, sc, raw[L.INFO["kl"]], worst, tol))
    assert np.isfinite(buf["logprob"]).all() and abs(float(raw[L.INFO["kl"]])) <= tol


# ---- 2. grid edges ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37, 256, 257, 300, 4200])
def test_head_grid_edges_and_identical_bits(gpu_ctx, B):
    """one block, a ragged block, exactly one block, one column into the second, many blocks (4200: the reference's HalfCheetah minibatch); two identical calls: identical bits"""
    ctx = gpu_ctx; c = _batch("2-32-2x1", B, 2.0, "ppo"); pi, b = _actor(c, ctx), _buffer(c, ctx); cfg = _cfg(c, "ppo"); ids = np.arange(B)
    _, rinfo, g, _ = PR.pg_loss(c, "ppo")
    raw = _call(ctx, ctx.lib.crux_loss_grad, pi, b, cfg, ids); gg = _grads(pi, ctx)
    raw2 = _call(ctx, ctx.lib.crux_loss_grad, pi, b, cfg, ids); gg2 = _grads(pi, ctx)
    e_g = np.abs(gg - g).max() / np.abs(g).max()
    print("2-32-2x1 B=%d:" % B, raw[:7], {k: v for k, v in rinfo.items() if np.isscalar(v)}, "gradient error / scale %.2e" % e_g)
    assert np.array_equal(raw.view(np.uint32), raw2.view(np.uint32)) and np.array_equal(gg.view(np.uint32), gg2.view(np.uint32))
    assert _info_close(raw, rinfo, "ppo") and e_g <= 1e-4


# ---- 3, 4. dispatch and the chain ------------------------------------------------------------------------------------------------------------------------------
def _orders(n, epochs, seed, counter=0):
    """the composed epoch orders of batch_train!: o_e[j] = o_(e-1)[perm_e[j]], perm_e = the library's permutation stream (include/crux_rng.h) at (seed, counter + e)"""
    out, prev = [], np.arange(n)
    for e in range(epochs):
        perm = np.zeros(n, np.int64); O.lib().orc_perm(seed, counter + e, n, O.vpz(perm)); prev = prev[perm]; out.append(prev)
    return out


def _minibatches(n, bs, epochs, seed):
    return [o[q:q + bs] for o in _orders(n, epochs, seed) for q in range(0, n, bs)]


def _batch_train(ctx, pi, b, cfg):
    raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((cfg.epochs, L.INFO_N), np.float32)
    ctx.check(ctx.lib.crux_batch_train(pi.h, b.h, C.byref(cfg), None, vp(raw), vp(ep))); return raw, ep


@pytest.mark.parametrize("kind", ["ppo", "bc"])
def test_register_resident_window_trains_on_the_dense_engine(gpu_ctx, capfd, kind):
    """the relu 3-64-64-2x1 at batch_size = 128 (the register-resident kernels' window): one crux_batch_train epoch over 300 rows == the yardstick's loop over the same
    minibatches (128, 128, 44). Tolerance: parity.relu_free_tol (2e-5 up to 64 free-running steps of a relu learner) on the parameters whose gradient every step keeps; the
    epoch's info row (the third minibatch's loss, entropy, kl, norm) at the project's 1e-4 relative, as everywhere in this file"""
    ctx = gpu_ctx; n, bs, seed = 300, 128, 23; c = _batch("3-64-64-2x1", n, 2.0, kind); pi, b = _actor(c, ctx), _buffer(c, ctx)
    mbs = _minibatches(n, bs, 1, seed); p, infos, grads = PR.pg_chain(c, kind, mbs, lr=LR)
    raw, ep = _batch_train(ctx, pi, b, _cfg(c, kind, bs=bs, epochs=1, seed=seed))
    keep = np.all([np.abs(g) > 1e-3 * np.abs(g).max() for g in grads], 0); e_p = np.abs(pi.get_params() - p)[keep].max()
    rel = {k: abs(float(raw[L.INFO[k]]) - infos[-1][k]) / max(1.0, abs(infos[-1][k])) for k in ("loss", "entropy", "kl", "grad_norm")}
    err = capfd.readouterr().err
    with capfd.disabled():      # (capfd holds this test's output even under -s: the figures are printed past it, before the assertions)
        print("3-64-64-2x1 %s, one epoch of 3 minibatches:" % kind, raw[:9], {k: v for k, v in infos[-1].items() if np.isscalar(v)}, "parameters %.2e, compared %.4f" % (e_p, keep.mean()),
              "info differences / max(1, |yardstick|):", {k: "%.2e" % v for k, v in rel.items()})
    assert raw[L.INFO["batches_trained"]] == 3 and raw[L.INFO["epochs_run"]] == 1 and keep.mean() >= 0.75
    assert e_p <= parity.relu_free_tol(3) and all(v <= 1e-4 for v in rel.values())
    assert np.array_equal(b["s"], c["s"][:, _orders(n, 1, seed)[-1]])      # the buffer is left in the epoch's order
    assert "generic single-workgroup learner" not in err


def _step_loop(ctx, c, kind, mbs, lr=LR):
    """crux_train_step per minibatch on a fresh actor and buffer: (states after every step, infos)"""
    pi, b = _actor(c, ctx, lr), _buffer(c, ctx); states, infos = [], []
    for idx in mbs:
        infos.append(_call(ctx, ctx.lib.crux_train_step, pi, b, _cfg(c, kind, bs=len(idx)), idx)); states.append(_state(pi))
    return states, infos


@pytest.mark.parametrize("sc", [0.0, 2.0])
def test_batch_train_equals_the_step_by_step_chain(gpu_ctx, sc):
    """crux_batch_train over 3 epochs of 300 rows at batch_size 128 (ragged last minibatch) == crux_train_step called with the ids of the same minibatches, bit for bit:
    parameters, Adam state and every epoch's info row; and the call stops where the step-by-step loop's kl first exceeds target_kl (training.jl:46, 49) / at max_batches (:45, 50).
    Both routes of a two-headed handle are the same chain of launches of the dense-engine learner, hence bit for bit. The constant-logSigma form of the same shape
    (GaussianPolicy 3-64-64-1, 9 steps at lr 1e-2) does NOT have this property, on the parent commit as now (its path is untouched): tools/sigma_pg_chain_probe.py measures
    it, profiles/sigma_pg_chain_probe.txt holds the result -- close, not the same bits. There the batch runs the feature-split register-resident kernel and a single step with
    ids the one-CU kernel (learner_route.h: k_train_fs2 takes no ids), two kernels with different summation orders. For that form the 2e-5 parameter tolerance would be the
    comparison; this form is held to the bits because it has them by construction."""
    ctx = gpu_ctx; n, bs, E, seed, kind, lr = 300, 128, 3, 29, "ppo", 1e-2; c = _batch("3-64-64-2x1", n, sc, kind); mbs = _minibatches(n, bs, E, seed)
    states, infos = _step_loop(ctx, c, kind, mbs, lr); kls = [float(i[L.INFO["kl"]]) for i in infos]
    pi, b = _actor(c, ctx, lr), _buffer(c, ctx); raw, ep = _batch_train(ctx, pi, b, _cfg(c, kind, bs=bs, epochs=E, seed=seed))
    print("ascale %g: kl per step" % sc, np.round(kls, 5))
    assert raw[L.INFO["batches_trained"]] == 9 and raw[L.INFO["epochs_run"]] == E and _same(_state(pi), states[-1])
    for e in range(E):
        assert np.array_equal(ep[e, :7].view(np.uint32), infos[3 * e + 2][:7].view(np.uint32)), e
    # target_kl between the running maximum and a later, larger kl (the such step nearest the middle of the run): the call must stop right after that step
    k = min((j for j in range(1, len(kls)) if kls[j] > max(kls[:j])), key=lambda j: abs(j - 4), default=0); tk = 0.5 * (kls[k] + max(kls[:k])) if k else kls[0] - 1e-4
    first = next(j for j, v in enumerate(kls) if v > np.float32(tk))
    pi, b = _actor(c, ctx, lr), _buffer(c, ctx); raw, _ = _batch_train(ctx, pi, b, _cfg(c, kind, bs=bs, epochs=E, seed=seed, target_kl=float(tk)))
    print("target_kl %.5f: stopped after %d batches, %d epochs (step loop: first kl above it at step %d)" % (tk, raw[L.INFO["batches_trained"]], raw[L.INFO["epochs_run"]], first))
    assert raw[L.INFO["batches_trained"]] == first + 1 and raw[L.INFO["epochs_run"]] == first // 3 + 1 and _same(_state(pi), states[first])
    pi, b = _actor(c, ctx, lr), _buffer(c, ctx); raw, _ = _batch_train(ctx, pi, b, _cfg(c, kind, bs=bs, epochs=E, seed=seed, max_batches=5))
    assert raw[L.INFO["batches_trained"]] == 5 and raw[L.INFO["epochs_run"]] == 2 and _same(_state(pi), states[4])


# ---- 5. the pair call ------------------------------------------------------------------------------------------------------------------------------------------
def test_pair_call_equals_the_two_sequential_calls(gpu_ctx):
    """crux_policy_gradient_training(two-headed actor, critic) -- both chains on the dense engine, one per learner stream -- against crux_batch_train(actor) then
    crux_batch_train(critic). Tolerance: that of test_gpu_dense_learner.py's pair test, parity.relu_free_tol of the steps taken (2e-5 up to 64)."""
    ctx = gpu_ctx; n, bs, E = 300, 128, 2; c = _batch("3-64-64-2x1", n, 2.0, "ppo"); acts = ["relu", "relu", "identity"]
    ca, cc = _cfg(c, "ppo", bs=bs, epochs=E, seed=31), parity.train_cfg("value_mse", "deterministic", bs, E, seed=37)

    def run(pair):
        pi, b = _actor(c, ctx), _buffer(c, ctx); cr = crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=7, ctx=ctx); cr.attach_optimizer(crux.Adam(np.float32(LR)))
        ra, rc = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
        if pair:
            ctx.check(ctx.lib.crux_policy_gradient_training(pi.h, cr.h, b.h, C.byref(ca), C.byref(cc), None, None, vp(ra), vp(rc), None, None))
        else:
            ctx.check(ctx.lib.crux_batch_train(pi.h, b.h, C.byref(ca), None, vp(ra), None)); ctx.check(ctx.lib.crux_batch_train(cr.h, b.h, C.byref(cc), None, vp(rc), None))
        return pi.get_params(), cr.get_params(), ra, rc, b["s"], b["a"]
    x, y = run(True), run(False); tol = parity.relu_free_tol(E * 3)
    print("pair against sequential: actor %.2e critic %.2e (tolerance %.1e)" % (np.abs(x[0] - y[0]).max(), np.abs(x[1] - y[1]).max(), tol), x[2][:9], x[3][:9])
    assert not np.array_equal(x[0], c["p"]) and x[2][L.INFO["batches_trained"]] == y[2][L.INFO["batches_trained"]] == E * 3 == x[3][L.INFO["batches_trained"]]
    assert np.abs(x[0] - y[0]).max() <= tol and np.abs(x[1] - y[1]).max() <= tol
    assert np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5])      # the buffer ends in the critic's last order either way


# ---- 6. refusals and the NaN gate ------------------------------------------------------------------------------------------------------------------------------
def _small(ctx, sc=1.0):
    c = _batch("2-32-2x1", 37, sc, "ppo"); pi, b = _actor(c, ctx), _buffer(c, ctx)
    _call(ctx, ctx.lib.crux_train_step, pi, b, _cfg(c, "ppo"), np.arange(37))      # a real step first: the Adam state is not all zeros
    return c, pi, b


def test_c_entries_refuse_by_name_and_touch_nothing(gpu_ctx):
    ctx = gpu_ctx; lib = ctx.lib; raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((2, L.INFO_N), np.float32)
    for sc in (0.0, 1.0):
        c, pi, b = _small(ctx, sc); before = _state(pi); cfg = _cfg(c, "ppo", bs=16, epochs=2); seen = {}

        def refused(what, rc, code=L.EUNSUP):
            msg = (lib.crux_last_error(ctx.h) or b"").decode(); seen[what] = msg; print("%s -> %d: %s" % (what, rc, msg))
            assert rc == code and ("two-headed" in msg) and _same(_state(pi), before), (what, rc, msg)
        lag = L.Lagrange(); cl = _cfg(c, "ppo", bs=16, epochs=2); cl.loss = L.LOSS["lagrange_ppo"]
        refused("lagrange_ppo_loss", lib.crux_batch_train_lagrange(pi.h, b.h, C.byref(cl), C.byref(lag), None, vp(raw), vp(ep)))
        fh = C.c_void_p(); ctx.check(lib.crux_fisher_create(pi.h, 1.0, C.byref(fh)))
        refused("crux_batch_train_fisher", lib.crux_batch_train_fisher(pi.h, fh, b.h, C.byref(cfg), None, vp(raw), vp(ep))); ctx.check(lib.crux_fisher_destroy(fh))
        cm = _cfg(c, "ppo", bs=16); cm.loss = L.LOSS["mse_action"]; ids = np.arange(37, dtype=np.int64)
        refused("mse_action (loss_grad)", lib.crux_loss_grad(pi.h, b.h, C.byref(cm), vp(ids), 37, vp(raw)))
        refused("mse_action (batch_train)", lib.crux_batch_train(pi.h, b.h, C.byref(cm), None, vp(raw), vp(ep)))
        cr = crux.ContinuousNetwork(parity.chain([2, 32, 1], ["relu", "identity"]), ctx=ctx); cr.attach_optimizer(crux.Adam(np.float32(LR))); cc = parity.train_cfg("value_mse", "deterministic", 16, 2)
        ca = _cfg(c, "ppo", bs=16, epochs=2); ra, rcr = np.zeros((1, L.INFO_N), np.float32), np.zeros((1, L.INFO_N), np.float32)
        ha, hc, hb = (C.c_void_p * 1)(pi.h), (C.c_void_p * 1)(cr.h), (C.c_void_p * 1)(b.h)
        refused("policy_gradient_training_multi", lib.crux_policy_gradient_training_multi(1, ha, hc, hb, C.byref(ca), C.byref(cc), vp(ra), vp(rcr)))
        refused("policy_gradient_training_synced", lib.crux_policy_gradient_training_synced(pi.h, cr.h, b.h, C.byref(ca), C.byref(cc), 1, vp(ra), vp(rcr)))
        cols = (C.c_void_p * L.NCOLS)(); first = C.c_int64(0)
        refused("steps_push (nominal)", lib.crux_steps_push(b.h, 0, cols, 1, 0, None, 0.95, 0.99, None, pi.h, L.HEAD["gaussian"], C.byref(first)))
        refused("importance_weight_rows (nominal)", lib.crux_importance_weight_rows(b.h, pi.h, L.HEAD["gaussian"], 0, 1))
        # the handle's rows against the batch's: CRUX_EINVAL with a message of its own
        wide = _policy([2, 32, 4], ["relu", "identity"], 2, sc, ctx); wide.attach_optimizer(crux.Adam(np.float32(LR)))
        rc = lib.crux_loss_grad(wide.h, b.h, C.byref(_cfg(c, "ppo")), vp(ids), 37, vp(raw)); msg = (lib.crux_last_error(ctx.h) or b"").decode(); print("rows ->", rc, msg)
        assert rc == L.EINVAL and "two-headed" in msg
        assert len(set(seen.values())) >= 6      # by name: the messages differ


@pytest.fixture()
def two_contexts(gpu_ctx):
    c1 = crux.Context(0)
    RG.attach_or_skip([gpu_ctx, c1], owned=[c1])
    yield gpu_ctx, c1
    gpu_ctx.peer_detach(); c1.peer_detach(); c1.close()


def test_replica_group_refuses_a_two_headed_actor(two_contexts):
    """need_px: crux_batch_train with a replica group attached returns CRUX_EUNSUP before anything is enqueued (no exchange is ever waited for); single steps stay local"""
    ctx, _ = two_contexts; c, pi, b = _small(ctx); before = _state(pi); raw = np.zeros(L.INFO_N, np.float32)
    rc = ctx.lib.crux_batch_train(pi.h, b.h, C.byref(_cfg(c, "ppo", bs=16, epochs=2)), None, vp(raw), None); msg = (ctx.lib.crux_last_error(ctx.h) or b"").decode(); print(rc, msg)
    assert rc == L.EUNSUP and "two-headed" in msg and "replica group" in msg and _same(_state(pi), before)


def test_host_mirror_refuses_by_name(gpu_ctx):
    ctx = gpu_ctx; c, pi, b = _small(ctx); before = _state(pi); S = crux.ContinuousSpace(2); acts = ["relu", "identity"]
    cr = lambda: crux.ContinuousNetwork(parity.chain([2, 32, 1], acts), ctx=ctx)      # noqa: E731
    ac = crux.ActorCritic(pi, cr())
    with pytest.raises(NotImplementedError, match="lagrange_ppo"):
        crux.LagrangePPO(ac, cr(), S, two_headed=True)
    with pytest.raises(NotImplementedError, match="ASAF"):
        crux.ASAF(pi, S, b)
    with pytest.raises(NotImplementedError, match="mse_action"):
        crux.BC(pi, S, b, loss=crux.mse_action_loss, two_headed=True)
    with pytest.raises(NotImplementedError, match="DiagonalFisherRegularizer"):
        crux.DiagonalFisherRegularizer(pi)
    with pytest.raises(NotImplementedError, match="CustomLoss"):
        crux.batch_train_(pi, crux.TrainingParams(loss=crux.CustomLoss(lambda y, D, P: (0.0, np.zeros_like(y)))), {}, b)
    with pytest.raises(NotImplementedError, match="mse_action"):
        crux.train_(pi, crux.TrainingParams(loss=crux.mse_action_loss), {}, b, np.arange(1, 9))
    sv = crux.PPO(ac, S, a_opt={"epochs": 1, "batch_size": 16}, c_opt={"epochs": 1, "batch_size": 16}, target_kl=None, two_headed=True)
    with pytest.raises(NotImplementedError, match="policy_gradient_training_synced"):
        crux.policy_gradient_training_synced(sv, b)
    with pytest.raises(NotImplementedError, match="policy_gradient_training_multi"):
        crux.policy_gradient_training_multi([ac], sv.a_opt, sv.c_opt, sv.P, [b])
    with pytest.raises(NotImplementedError, match="critic"):
        crux.PPO(crux.ActorCritic(cr(), pi), S, two_headed=True)      # a two-headed network anywhere but in the actor's place
    # without two_headed=True the solver constructors refuse such an actor by name, as before
    for make in (lambda: crux.PPO(ac, S), lambda: crux.A2C(ac, S), lambda: crux.REINFORCE(pi, S), lambda: crux.BC(pi, S, b)):
        with pytest.raises(NotImplementedError, match="two_headed=True"):
            make()
    assert _same(_state(pi), before)


@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_nan_advantage_is_reported_and_nothing_moves(gpu_ctx, kind):
    ctx = gpu_ctx
    for sc in (0.0, 2.0):
        c = dict(_batch("5-100-100-2x3", 37, sc, kind)); pi, b = _actor(c, ctx), _buffer(c, ctx); cfg = _cfg(c, kind)
        _call(ctx, ctx.lib.crux_train_step, pi, b, cfg, np.arange(37))      # a real step first: the Adam state is not all zeros
        adv = c["advantage"].copy(); adv[5] = np.nan; b["advantage"] = adv.reshape(1, 37); before = _state(pi)
        for fn in (lambda: _call(ctx, ctx.lib.crux_train_step, pi, b, cfg, np.arange(37)), lambda: _batch_train(ctx, pi, b, _cfg(c, kind, bs=64, epochs=2))):      # (one minibatch per epoch: it holds the NaN row)
            with pytest.raises(crux.CruxError) as e:
                fn()
            assert e.value.code == L.ENAN and _same(_state(pi), before)


# ---- 7. solvers ------------------------------------------------------------------------------------------------------------------------------------------------
def _pendulum_actor(ctx, seed):
    return _policy([3, 64, 64, 2], ["relu", "relu", "identity"], 1, 2.0, ctx, seed=seed)


@pytest.mark.parametrize("algo", ["PPO", "A2C", "REINFORCE"])
def test_on_policy_solvers_run_on_pendulum(gpu_ctx, algo):
    """two iterations of dN = 512 at batch_size 128 on the device Pendulum with a two-headed SquashedGaussianPolicy 3-64-64-2x1: infos finite, parameters moved"""
    ctx = gpu_ctx; acts = ["relu", "relu", "identity"]; A = _pendulum_actor(ctx, 2); S = crux.ContinuousSpace(3); o = {"epochs": 4, "batch_size": 128}
    cr = crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=3, ctx=ctx)
    if algo == "PPO":
        sv = crux.PPO(crux.ActorCritic(A, cr), S, N=1024, dN=512, max_steps=100, a_opt=o, c_opt=o, two_headed=True)
    elif algo == "A2C":
        sv = crux.A2C(crux.ActorCritic(A, cr), S, N=1024, dN=512, max_steps=100, a_opt=o, c_opt=o, two_headed=True)
    else:
        sv = crux.REINFORCE(A, S, N=1024, dN=512, max_steps=100, a_opt=o, two_headed=True)
    p0 = A.get_params()
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=8))
    print(algo, sv.history)
    assert len(sv.history) == 2 and all(np.isfinite(v) for h in sv.history for v in h.values() if isinstance(v, float))
    assert all(h["actor_batches_trained"] >= 1 for h in sv.history) and not np.array_equal(A.get_params(), p0) and np.isfinite(A.get_params()).all()


def test_bc_from_a_two_headed_teacher(gpu_ctx):
    """BC (logpdf_bc_loss) on 512 demonstrations drawn from a two-headed teacher: the validation error after 30 epochs is below the one before training"""
    ctx = gpu_ctx; n = 512; S = crux.ContinuousSpace(3); rng = np.random.default_rng(4)
    teacher, pi = _pendulum_actor(ctx, 11), _pendulum_actor(ctx, 12)
    s = np.asfortranarray(rng.normal(0, 1, (3, n)).astype(np.float32)); a, _ = teacher.exploration(s, 77, 0)
    D = crux.ExperienceBuffer(S, crux.ContinuousSpace(1), n, ctx=ctx)
    D.push_({"s": s, "a": a, "sp": s, "r": np.zeros((1, n), np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool)})
    sv = crux.BC(pi, S, D, normalize_demo=False, opt={"epochs": 29, "batch_size": 128, "optimizer": crux.Adam(np.float32(1e-3))}, window=100, two_headed=True)
    p0 = pi.get_params(); v0 = {}; sv.early_stopping([v0]); crux.solve(sv)      # (the stopping rule writes the validation error -- loss_value -- into the last info)
    errs = [h["validation_error"] for h in sv.history]
    print("BC validation error before %.5f, after %d epochs %.5f" % (v0["validation_error"], len(errs), errs[-1]))
    assert len(errs) == 30 and np.isfinite(errs).all() and errs[-1] < v0["validation_error"] and not np.array_equal(pi.get_params(), p0)
