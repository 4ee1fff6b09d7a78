"""GPU: ASAF on the dense engine (crux_asaf_freeze, crux_asaf_actor_step, crux_asaf_batch_train, csrc/asaf.hip; crux.ASAF) against the float64 restatement of
tests/asaf_reference.py; the chain against the manual loop of shuffle + step; the carried gG against a fresh freeze; solve(ASAF) against the manual composition of
steps!, freeze and batch train; and a learning check on the committed Pendulum demonstrations.

Reference: src/model_free/il/asaf.jl, src/policies.jl:333-398, src/training.jl:13-55. Tolerances are those of tests/test_gpu_advil.py and tests/test_gpu_cql.py: 1e-4
relative on losses, norms, log-densities and the steps' values, 1e-4 of the gradient scale on the gradient buffer, 2e-5 absolute on parameters after one Adam step at
lr = 1e-3. Entries whose float64 gradient is within 1e-3 of the gradient scale of zero are not compared after Adam (the first step is lr sign(g) there); at most a quarter
of the parameters may be left out that way. Parameters and data come from numpy, so every case runs through the yardstick alone, without a device
(left_out_shares() below): the seeds were fixed that way. Share of the parameters left out per (shape, activation, head), the larger of n = 256 and n = 37:
    2-64-64-1  relu  gaussian 16.0 %, squashed 16.0 %      2-64-64-1  tanh  gaussian 2.3 %, squashed 2.3 %
    17-64-64-6 relu  gaussian 5.0 %, squashed 5.0 %        17-64-64-6 tanh  gaussian 3.9 %, squashed 3.6 %
(the relu network with one output keeps second-layer units that no column activates: their weights have a gradient of exactly zero and stay where they are).
"""
import ctypes as C
import os

import numpy as np
import pytest

import asaf_reference as R
import parity
from parity import crux, L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR = 1e-3
MAX_LEFT_OUT = 0.25
SHAPES = {"2-64-64-1": (2, 1, [64, 64]), "17-64-64-6": (17, 6, [64, 64])}
ASCALE = 2.0


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _init(dims, rng, logsigma):
    """Glorot-uniform weights, small non-negative biases (no relu unit is dead from the start), then logSigma, in the flat Flux order"""
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o))
        out += [rng.uniform(-lim, lim, i * o), np.abs(rng.normal(0, 0.3, o))]
    out.append(np.asarray(logsigma, np.float64))
    return np.concatenate(out).astype(np.float32)


def case(shape, act, head, n, nE, seed):
    """dims, activations, the frozen copy's and the current parameters (pi != piG: every parameter perturbed, so the sigmoid weights vary), a rollout block and the
    demonstrations: everything a test and the yardstick need, from numpy alone. The rollout actions are samples of piG (squashed: ascale tanh of them), the
    demonstrations follow a fixed smooth function of the state, so the gradient carries a signal and not only sampling noise. Squashed: the first two demonstration
    columns and the first rollout column sit on +-ascale (the clamp is live)."""
    od, ad, hidden = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(seed)
    dims, acts = [od] + list(hidden) + [ad], [act] * len(hidden) + ["identity"]
    ascale = ASCALE if head == "squashed" else 0.0
    pG = _init(dims, rng, rng.normal(-0.5, 0.2, ad))
    p = (pG + rng.normal(0, 0.03, pG.size)).astype(np.float32)
    V = rng.normal(0, 1.0, (ad, od))

    def block(m, expert):
        s = rng.normal(0, 1, (od, m)).astype(np.float32)
        if expert:
            u = 0.8 * np.tanh(V @ s) + rng.normal(0, 0.1, (ad, m))
        else:
            layers, _ls = R.params(pG, dims)
            u = R.mlp(layers, acts, R._t(s)).detach().numpy() + np.exp(pG[-ad:].astype(np.float64))[:, None] * rng.normal(0, 1, (ad, m))
        a = (ascale * np.tanh(u) if ascale > 0 else u).astype(np.float32)
        return {"s": s, "a": a, "sp": rng.normal(0, 1, (od, m)).astype(np.float32), "r": rng.normal(0, 1, (1, m)).astype(np.float32), "done": rng.random((1, m)) < 0.1}
    roll, demo = block(n, False), block(nE, True)
    if ascale > 0:
        demo["a"][:, 0] = ascale; demo["a"][:, 1] = -ascale; roll["a"][:, 0] = -ascale
    return {"dims": dims, "acts": acts, "ascale": ascale, "pG": pG, "p": p, "roll": roll, "demo": demo}


def reference_step(c):
    """the yardstick on a case: loss, parts and the flat float64 gradient of the current parameters"""
    gG = R.frozen(c["pG"], c["dims"], c["acts"], c["roll"]["s"], c["roll"]["a"], c["ascale"])
    gE = R.frozen(c["pG"], c["dims"], c["acts"], c["demo"]["s"], c["demo"]["a"], c["ascale"])
    layers, ls = R.params(c["p"], c["dims"])
    loss, parts = R.asaf_loss(layers, c["acts"], ls, c["roll"]["s"], c["roll"]["a"], gG, c["demo"]["s"], c["demo"]["a"], gE, c["ascale"])
    loss.backward()
    return loss.item(), parts, R.flat(layers, ls)


STEP_CASES = [(sh, act, head, n) for sh in SHAPES for act in ("relu", "tanh") for head in ("gaussian", "squashed") for n in (256, 37)]


def _step_case(sh, act, head, n):
    return case(sh, act, head, n, 157 if n == 256 else 75, seed=7)


def left_out_shares():
    """no device: the share of parameters each step case leaves out of the Adam comparison (the docstring's table)"""
    out = {}
    for sc in STEP_CASES:
        g = reference_step(_step_case(*sc))[2]
        out[sc] = float(1.0 - (np.abs(g) > 1e-3 * np.abs(g).max()).mean())
    return out


def _policy(c, p, ctx):
    ch = parity.chain(c["dims"], c["acts"]); ad = c["dims"][-1]
    pi = crux.SquashedGaussianPolicy(ch, np.zeros(ad, np.float32), c["ascale"], ctx=ctx) if c["ascale"] > 0 else crux.GaussianPolicy(ch, np.zeros(ad, np.float32), ctx=ctx)
    pi.set_params(p); pi.attach_optimizer(crux.Adam(np.float32(LR)))
    return pi


def _buffer(ctx, data, discrete=False, extras=("logprob",), capacity=None):
    od, ad, B = data["s"].shape[0], data["a"].shape[0], data["s"].shape[1]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if discrete else crux.ContinuousSpace(ad), capacity or B, extras, ctx=ctx)
    b.push_(data); return b


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


class Setup:
    """the two buffers of a case on the device with gG (the rollout buffer's :logprob column) and gE (a device array) frozen from piG"""

    def __init__(self, ctx, c, extras=("logprob",)):
        self.b, self.demo = _buffer(ctx, c["roll"], extras=extras), _buffer(ctx, c["demo"], extras=())
        self.gE = crux.il_on_policy._DeviceVec(ctx, len(self.demo))
        G = _policy(c, c["pG"], ctx)
        crux.asaf_freeze_(G, self.b, self.b.column_ptr("logprob")); crux.asaf_freeze_(G, self.demo, self.gE.p)
        self.gG = self.b.column_ptr("logprob")


# ---- 1. the freeze pass ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["gaussian", "squashed"])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_freeze_matches_reference(gpu_ctx, shape, act, head):
    c = case(shape, act, head, 256, 157, seed=3)
    st = Setup(gpu_ctx, c)
    for name, got, d in (("gG", st.b["logprob"][0], c["roll"]), ("gE", st.gE.get(), c["demo"])):
        want = R.frozen(c["pG"], c["dims"], c["acts"], d["s"], d["a"], c["ascale"])
        dev = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print("freeze %s %s %s %s: max relative deviation %.3g over %d rows, range [%.4g, %.4g]" % (shape, act, head, name, dev.max(), want.size, want.min(), want.max()))
        assert np.isfinite(got).all() and dev.max() <= 1e-4, (name, dev.max())
    # a sub-range lands where it belongs and changes nothing else; parameters and the gradient buffer are not touched
    G = _policy(c, c["pG"], gpu_ctx); g0 = _grads(G)
    out = crux.il_on_policy._DeviceVec(gpu_ctx, 40); gpu_ctx.h2d(out.p, np.full(40, 7.0, np.float32))
    crux.asaf_freeze_(G, st.b, out.p, first_row=100, n_rows=37)
    got = out.get()
    assert np.array_equal(_bits(got[:37]), _bits(st.b["logprob"][0][100:137])) and np.all(got[37:] == 7.0)
    assert np.array_equal(_bits(G.get_params()), _bits(c["pG"])) and np.array_equal(_bits(_grads(G)), _bits(g0))


# ---- 2. the actor step against the yardstick ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [None, 0.02], ids=["noclip", "clip"])
@pytest.mark.parametrize("shape,act,head,n", STEP_CASES, ids=["%s-%s-%s-n%d" % sc for sc in STEP_CASES])
def test_actor_step_matches_reference(gpu_ctx, shape, act, head, n, clip):
    c = _step_case(shape, act, head, n)
    assert c["demo"]["s"].shape[1] % 16 != 0
    loss, parts, g_ref = reference_step(c)
    st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx)
    raw, out = crux.asaf_actor_step_(pi, st.b, 0, n, st.gG, st.demo, st.gE.p, clip_value=clip)
    gn = np.linalg.norm(g_ref)
    print("step %s %s %s n %d clip %s: loss %.8g (%.8g) norm %.8g (%.8g) out %s ref %s" % (shape, act, head, n, clip, raw[0], loss, raw[1], gn, out, parts))
    assert _close(raw[L.INFO["loss"]], loss), (raw[0], loss)
    assert _close(raw[L.INFO["grad_norm"]], gn), (raw[1], gn)                      # the norm is the raw gradient's, clip or not
    assert _close(raw[L.INFO["entropy"]], parts["entropy"])
    for k, key in enumerate(("entropy", "expert", "policy")):
        assert _close(out[k], parts[key]), (key, out[k], parts[key])
    g_used = R.clip_value(g_ref, clip)
    if clip is not None:
        assert 0.02 < (np.abs(g_ref) > clip).mean() < 0.98                          # the clamp is live and not everything
    assert np.abs(_grads(pi).astype(np.float64) - g_used).max() <= 1e-4 * np.abs(g_ref).max()
    want = R.adam_first_step(c["p"].astype(np.float64), g_used, lr=LR)
    ok = np.abs(g_ref) > 1e-3 * np.abs(g_ref).max()
    left_out = 1.0 - ok.mean(); p_new = pi.get_params()
    print("    %.1f %% of %d parameters left out, max deviation %.3g" % (100 * left_out, g_ref.size, np.abs(p_new[ok] - want[ok]).max()))
    assert left_out <= MAX_LEFT_OUT, left_out
    assert np.abs(p_new[ok] - want[ok]).max() < 2e-5


def test_pi_equal_to_its_frozen_copy_gives_two_ln2(gpu_ctx):
    """the known answer of tests/test_asaf_reference.py on the device: the step's log-densities are the freeze's, so both softplus terms are ln 2 to float32 rounding"""
    for head in ("gaussian", "squashed"):
        c = case("17-64-64-6", "tanh", head, 64, 75, seed=5); c["p"] = c["pG"]
        st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx)
        raw, out = crux.asaf_actor_step_(pi, st.b, 0, 64, st.gG, st.demo, st.gE.p)
        assert abs(out[1] - np.log(2.0)) < 1e-6 and abs(out[2] - np.log(2.0)) < 1e-6, out
        assert _close(raw[0], 2 * np.log(2.0) - 0.1 * out[0])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------------------------------
def test_steps_are_deterministic(gpu_ctx):
    c = case("17-64-64-6", "relu", "squashed", 256, 157, seed=4)
    outs = []
    for _ in range(2):
        st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx)
        r1, o1 = crux.asaf_actor_step_(pi, st.b, 0, 256, st.gG, st.demo, st.gE.p, clip_value=0.02)
        r2, o2 = crux.asaf_actor_step_(pi, st.b, 19, 200, st.gG, st.demo, st.gE.p)
        outs.append((pi.get_params(), st.b["logprob"], st.gE.get(), r1, o1, r2, o2) + pi.adam_state()[:2])
    assert all(np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])) for k in range(9))
    assert not np.array_equal(outs[0][0], c["p"])


# ---- 4. NaN ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", ["s", "a"])
@pytest.mark.parametrize("which", ["roll", "demo"])
def test_nan_raises_and_leaves_parameters(gpu_ctx, which, col):
    c = case("2-64-64-1", "relu", "gaussian", 64, 37, seed=6)
    st = Setup(gpu_ctx, c)                                             # gG and gE from clean data: the NaN enters through the step's own reads
    bad = {k: v.copy() for k, v in c[which].items()}; bad[col][0, 29] = np.nan
    if which == "roll":
        b, demo = _buffer(gpu_ctx, bad), st.demo
        gpu_ctx.h2d(b.column_ptr("logprob"), np.ascontiguousarray(st.b["logprob"][0]))
    else:
        b, demo = st.b, _buffer(gpu_ctx, bad, extras=())
    pi = _policy(c, c["p"], gpu_ctx); m0, v0, bp0 = pi.adam_state()
    with pytest.raises(L.CruxError) as e:
        crux.asaf_actor_step_(pi, b, 0, 64, b.column_ptr("logprob"), demo, st.gE.p)
    assert e.value.code == L.ENAN and "NaN detected" in str(e.value)
    m1, v1, bp1 = pi.adam_state()
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"])) and np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(bp0, bp1)
    # the chain (one minibatch per epoch, so the first step meets the NaN): the same error, nothing updated by any later step either
    class _S:
        pass
    sv = _S(); sv.agent = crux.PolicyParams(pi); sv.demo, sv.gE, sv.clip_value = demo, st.gE, None
    sv.a_opt = crux.TrainingParams(loss=crux.asaf_loss, optimizer=pi.optimizer, batch_size=64, epochs=3, name="actor_")
    with pytest.raises(L.CruxError) as e:
        crux.batch_train_asaf_(sv, b)
    assert e.value.code == L.ENAN
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"])) and np.array_equal(pi.adam_state()[2], bp0)


# ---- 5. rejections -----------------------------------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    c = case("2-64-64-1", "relu", "gaussian", 32, 21, seed=8)
    st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx)
    step = lambda pi_, b_, demo_, n_=32: crux.asaf_actor_step_(pi_, b_, 0, n_, st.gG, demo_, st.gE.p)      # noqa: E731
    disc = dict(c["roll"]); disc["a"] = np.ones((1, 32), bool)
    for args in ((pi, _buffer(gpu_ctx, disc, discrete=True), st.demo), (pi, st.b, _buffer(gpu_ctx, {k: v[:, :21] for k, v in disc.items()}, discrete=True, extras=()))):
        with pytest.raises(L.CruxError) as e:                          # a discrete action column in either buffer
            step(*args)
        assert e.value.code == L.EINVAL
    det = crux.ContinuousNetwork(parity.chain(c["dims"], c["acts"]), ctx=gpu_ctx); det.attach_optimizer(crux.Adam(np.float32(LR)))
    with pytest.raises(L.CruxError) as e:                              # no logSigma extras
        step(det, st.b, st.demo)
    assert e.value.code == L.EUNSUP
    with pytest.raises(L.CruxError) as e:
        crux.asaf_freeze_(det, st.b, st.gG)
    assert e.value.code == L.EUNSUP
    empty = crux.ExperienceBuffer(crux.ContinuousSpace(2), crux.ContinuousSpace(1), 8, ctx=gpu_ctx)
    with pytest.raises(L.CruxError) as e:                              # empty demonstrations
        step(pi, st.b, empty)
    assert e.value.code == L.EINVAL
    wide = case("17-64-64-6", "relu", "gaussian", 32, 21, seed=8)
    for args in ((_policy(wide, wide["p"], gpu_ctx), st.b, st.demo), (pi, st.b, _buffer(gpu_ctx, wide["demo"], extras=()))):
        with pytest.raises(L.CruxError) as e:                          # widths that do not fit
            step(*args)
        assert e.value.code == L.EINVAL
    for n_ in (0, 33):                                                 # n < 1, rows outside the buffer
        with pytest.raises(L.CruxError) as e:
            step(pi, st.b, st.demo, n_)
        assert e.value.code == L.EINVAL
    assert np.array_equal(_bits(pi.get_params()), _bits(c["p"]))
    S = crux.ContinuousSpace(2)
    dn = crux.DiscreteNetwork(parity.chain([2, 16, 3], ["relu", "identity"]), [1, 2, 3], ctx=gpu_ctx)
    with pytest.raises(NotImplementedError) as e:
        crux.ASAF(dn, S, st.demo)
    assert "categorical" in str(e.value)
    with pytest.raises(TypeError):
        crux.ASAF(det, S, st.demo)
    nolp = _buffer(gpu_ctx, c["roll"], extras=())                      # the chain needs the :logprob column that carries gG
    class _S:
        pass
    sv = _S(); sv.agent = crux.PolicyParams(pi); sv.demo, sv.gE, sv.clip_value = st.demo, st.gE, None
    sv.a_opt = crux.TrainingParams(loss=crux.asaf_loss, optimizer=pi.optimizer, batch_size=16, epochs=1, name="actor_")
    with pytest.raises(L.CruxError) as e:
        crux.batch_train_asaf_(sv, nolp)
    assert e.value.code == L.EINVAL


# ---- 6. the chain against the manual loop --------------------------------------------------------------------------------------------------------------------------
def _solver_stub(pi, st, bs, epochs, clip, seed=21, max_batches=np.inf):
    class _S:
        pass
    sv = _S(); sv.agent = crux.PolicyParams(pi); sv.demo, sv.gE, sv.clip_value = st.demo, st.gE, clip
    sv.a_opt = crux.TrainingParams(loss=crux.asaf_loss, optimizer=pi.optimizer, batch_size=bs, epochs=epochs, name="actor_", shuffle_seed=seed, max_batches=max_batches)
    return sv


@pytest.mark.parametrize("head,clip,max_batches", [("gaussian", None, np.inf), ("squashed", 0.02, np.inf), ("squashed", None, 7)], ids=["gaussian", "squashed-clip", "max_batches"])
def test_batch_train_matches_manual_loop(gpu_ctx, head, clip, max_batches):
    n, bs, epochs = 150, 64, 3                                        # minibatches of 64, 64, 22
    c = case("17-64-64-6", "tanh", head, n, 75, seed=9)
    runs = []
    for manual in (False, True):
        st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx)
        if not manual:
            sv = _solver_stub(pi, st, bs, epochs, clip, max_batches=max_batches)
            info = crux.batch_train_asaf_(sv, st.b)
            assert sv.a_opt.shuffle_counter == info["_epochs_run"]
            rows, total = info["_epoch_infos"], info["actor_batches_trained"]
        else:
            rows, total, stop = [], 0, False
            for ep in range(epochs):
                crux.shuffle_device_(st.b, 21, ep)
                for k0 in range(0, n, bs):
                    raw, out = crux.asaf_actor_step_(pi, st.b, k0, min(bs, n - k0), st.b.column_ptr("logprob"), st.demo, st.gE.p, clip_value=clip)
                    total += 1
                    if total >= max_batches:
                        stop = True; break
                rows.append(np.concatenate([raw, out, [0.0]]).astype(np.float32))
                if stop:
                    break
            rows = np.stack(rows)
        runs.append((pi.get_params(), rows, total, st.b["s"], st.b["logprob"]) + pi.adam_state())
    a, b = runs
    assert a[2] == b[2] == (7 if max_batches == 7 else 9) and a[1].shape == b[1].shape == (3, L.INFO_N + 4)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[5]), _bits(b[5])) and np.array_equal(_bits(a[6]), _bits(b[6])) and np.array_equal(a[7], b[7])
    for k in (L.INFO["loss"], L.INFO["grad_norm"], L.INFO["entropy"], L.INFO_N, L.INFO_N + 1, L.INFO_N + 2):
        assert np.array_equal(_bits(a[1][:, k]), _bits(b[1][:, k])), k
    assert np.array_equal(_bits(a[3]), _bits(b[3])) and np.array_equal(_bits(a[4]), _bits(b[4]))
    assert not np.array_equal(a[0], c["p"]) and np.all(np.isfinite(a[1]))


# ---- 7. gG rides the buffer's permutation --------------------------------------------------------------------------------------------------------------------------
def test_carried_gG_equals_a_fresh_freeze_after_the_shuffles(gpu_ctx):
    c = case("2-64-64-1", "relu", "squashed", 150, 75, seed=10)
    st = Setup(gpu_ctx, c); pi = _policy(c, c["p"], gpu_ctx); G = _policy(c, c["pG"], gpu_ctx)
    s0 = st.b["s"].copy()
    crux.batch_train_asaf_(_solver_stub(pi, st, 64, 2, None), st.b)
    assert not np.array_equal(st.b["s"], s0) and not np.array_equal(pi.get_params(), c["p"])
    fresh = crux.il_on_policy._DeviceVec(gpu_ctx, 150); crux.asaf_freeze_(G, st.b, fresh.p)
    assert np.array_equal(_bits(st.b["logprob"][0]), _bits(fresh.get()))
    crux.shuffle_device_(st.b, 5, 0); crux.asaf_freeze_(G, st.b, fresh.p)
    assert np.array_equal(_bits(st.b["logprob"][0]), _bits(fresh.get()))


# ---- 8. the solver against the manual composition ------------------------------------------------------------------------------------------------------------------
def test_solve_matches_manual_composition(gpu_ctx):
    ctx, dN, bs, epochs, iters = gpu_ctx, 96, 40, 2, 2               # minibatches of 40, 40, 16
    c = case((3, 1, [64, 64]), "tanh", "squashed", 8, 75, seed=12)      # the library's Pendulum observes (cos, sin, thetadot)
    S = crux.ContinuousSpace(3, mu=np.array([0.1, -0.2, 0.0], np.float32), sigma=np.array([1.5, 1.0, 4.0], np.float32))
    runs = []
    for manual in (False, True):
        pi = _policy(c, c["p"], ctx); demo = _buffer(ctx, c["demo"], extras=())
        mdp = crux.PendulumMDP(n_envs=4, seed=3)
        opt = {"batch_size": bs, "epochs": epochs, "optimizer": crux.Adam(np.float32(LR)), "shuffle_seed": 31}
        if not manual:
            sv = crux.ASAF(pi, S, demo, dN=dN, N=iters * dN, a_opt=opt, clip_value=1.0, max_steps=50)
            assert sv.c_opt is None and sv.a_opt.name == "actor_" and sv.a_opt.loss is crux.asaf_loss and sv.dN == dN
            crux.solve(sv, mdp)
            assert sv.demo is not demo and all(np.array_equal(demo[k], c["demo"][k]) for k in ("s", "a", "sp"))      # the caller's buffer: as it was
            assert not np.array_equal(sv.demo["s"], c["demo"]["s"])
            runs.append((pi.get_params(), sv.history, sv.buffer["s"], sv.buffer["logprob"])); continue
        p = crux.TrainingParams(loss=crux.asaf_loss, name="actor_", **opt); pi.attach_optimizer(p.optimizer)
        Dn = crux.normalize_(crux.copy_buffer(demo), S, crux.ContinuousSpace(1))
        gE = crux.il_on_policy._DeviceVec(ctx, len(Dn))
        buf = crux.ExperienceBuffer(S, crux.ContinuousSpace(1), dN, ["logprob"], ctx=ctx)
        smp = crux.Sampler(mdp, crux.PolicyParams(pi), S=S, required_columns=["logprob"], max_steps=50)
        hist = []
        for it in range(iters):
            crux.steps_(smp, buf, Nsteps=dN, explore=True, i=it * dN, reset=True)
            crux.asaf_freeze_(pi, buf, buf.column_ptr("logprob")); crux.asaf_freeze_(pi, Dn, gE.p)
            infos = []
            for ep in range(epochs):
                crux.shuffle_device_(buf, 31, it * epochs + ep)
                for k0 in range(0, dN, bs):
                    raw, out = crux.asaf_actor_step_(pi, buf, k0, min(bs, dN - k0), buf.column_ptr("logprob"), Dn, gE.p, clip_value=1.0)
                infos.append({"actor_loss": float(raw[0]), "actor_grad_norm": float(raw[1]), "entropy": float(out[0])})
            h = {k: float(np.mean(np.array([d[k] for d in infos], np.float32))) for k in infos[0]}; h["actor_batches_trained"] = 3 * epochs
            hist.append(h)
        runs.append((pi.get_params(), hist, buf["s"], buf["logprob"]))
    a, b = runs
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
    assert len(a[1]) == len(b[1]) == iters
    for h0, h1 in zip(a[1], b[1]):
        assert {"actor_loss", "actor_grad_norm", "entropy", "actor_batches_trained"} <= set(h0)
        assert all(h0[k] == h1[k] for k in h1), (h0, h1)
    assert not np.array_equal(a[0], c["p"])


# ---- 9. learning -------------------------------------------------------------------------------------------------------------------------------------------------
LEARN = {"seed": 0, "iterations": 30, "dN": 512, "batch_size": 128, "epochs": 4, "n_envs": 8, "max_steps": 64, "dims": [2, 64, 64, 1], "act": "tanh", "logsigma": -0.5,
         "ascale": 2.0, "clip_value": 1.0, "lr": 1e-3, "mdp": "SynthMDP(2, 1)"}      # profiles/asaf_learning.txt


def learning_setup():
    """the Pendulum demonstrations (512 rows; the actions reach +-2, so with ascale = 2 the clamp is live), whitened by their own statistics; the last 30 % of a fixed
    permutation held out"""
    d = dict(np.load(os.path.join(GOLD, "pendulum_transitions.npz")))
    mu, sg = d["s"].mean(1).astype(np.float32), d["s"].std(1).astype(np.float32)
    n = d["s"].shape[1]; order = np.random.default_rng(LEARN["seed"]).permutation(n); cut = int(round(0.7 * n))
    rng = np.random.default_rng(LEARN["seed"] + 1)
    return d, mu, sg, order[:cut], order[cut:], _init(LEARN["dims"], rng, [LEARN["logsigma"]])


def test_asaf_raises_the_held_out_demonstration_log_density(gpu_ctx):
    """ASAF on the Pendulum demonstrations with the settings of LEARN: the mean logpdf(pi, s_E, a_E) on the held-out 30 % of the demonstrations must be higher after
    training than before. The direction is the whole assertion. The demonstrations store the reference's (theta, thetadot) states, the library's Pendulum observes
    (cos, sin, thetadot), so the rollouts come from the two-observation SYNTH dynamics (parity.FAMILIES["synth_2_1"]). Measured on the GPU (profiles/asaf_learning.txt)."""
    d, mu, sg, tr, va, p0 = learning_setup()
    assert np.abs(d["a"]).max() >= LEARN["ascale"]
    S = crux.ContinuousSpace(2, mu=mu, sigma=sg)
    acts = [LEARN["act"]] * 2 + ["identity"]
    pi = crux.SquashedGaussianPolicy(parity.chain(LEARN["dims"], acts), np.zeros(1, np.float32), LEARN["ascale"], ctx=gpu_ctx); pi.set_params(p0)
    cols = ("s", "a", "sp", "r", "done")
    demo = _buffer(gpu_ctx, {k: np.ascontiguousarray(d[k][:, tr]) for k in cols}, extras=())
    held = crux.normalize_(_buffer(gpu_ctx, {k: np.ascontiguousarray(d[k][:, va]) for k in cols}, extras=()), S, crux.ContinuousSpace(1))
    out = crux.il_on_policy._DeviceVec(gpu_ctx, len(held))

    def score():
        crux.asaf_freeze_(pi, held, out.p); return float(np.mean(out.get().astype(np.float64)))
    before = score()
    sv = crux.ASAF(pi, S, demo, dN=LEARN["dN"], N=LEARN["iterations"] * LEARN["dN"], max_steps=LEARN["max_steps"], clip_value=LEARN["clip_value"],
                   a_opt={"batch_size": LEARN["batch_size"], "epochs": LEARN["epochs"], "optimizer": crux.Adam(np.float32(LEARN["lr"])), "shuffle_seed": LEARN["seed"]})
    crux.solve(sv, crux.SynthMDP(2, 1, n_envs=LEARN["n_envs"], seed=LEARN["seed"]))
    after = score()
    print("asaf pendulum: held-out mean logpdf(pi, s_E, a_E) %.6f -> %.6f over %d rows; last iteration %s" % (before, after, len(held), {k: v for k, v in sv.history[-1].items() if not k.startswith("_")}))
    assert len(sv.history) == LEARN["iterations"] and all(np.isfinite(h[k]) for h in sv.history for k in ("actor_loss", "actor_grad_norm", "entropy"))
    assert after > before, (before, after)
