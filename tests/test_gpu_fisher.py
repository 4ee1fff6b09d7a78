"""DiagonalFisherRegularizer on the device (csrc/fisher.hip, crux_batch_train_fisher) against the float64 yardstick of tests/fisher_reference.py, numpy's Float32 running
mean, and -- for the regularised batch_train! step -- the oracle's loss gradient plus the yardstick's gradient, then the oracle's Adam.

Primitive shapes: 3-5-2 with 2 extras (34 parameters, five arrays at offsets 0, 15, 20, 30, 32: less than one block) and 17-128-128-6 with 6 extras (19 596 parameters, more
than 64 x 256: every grid-stride loop runs more than once). Tolerances: the primitives 1e-6 relative (non-negative terms, at most eight Float32 roundings per term and
scale, 8 x 2^-24 = 4.8e-7); the regularised step the ones tests/test_gpu_dense_learner.py asserts for unregularised steps (gradient 1e-4 x scale, loss and grad_norm 1e-4,
parameters 2e-5, Adam moments 1e-5)."""
import ctypes as C

import numpy as np
import pytest

import crux_jl_amd as crux
from crux_jl_amd import _lib as L
from crux_jl_amd import core
import dense_reference as DR
import fisher_reference as FR
import oracle as O
import parity

pytestmark = pytest.mark.gpu
P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
EXTRAS = ["return", "logprob", "advantage"]
PRIM = [([3, 5, 2], 2), ([17, 128, 128, 6], 6)]
PRIM_IDS = ["3-5-2+2", "17-128-128-6+6"]


def _not_generic(capfd):
    assert "outside the MFMA learner family" not in capfd.readouterr().err


def _gauss(dims, n_extra, seed=3):
    acts = ["tanh"] * (len(dims) - 2) + ["identity"]
    return crux.GaussianPolicy(parity.chain(dims, acts), np.full(n_extra, -0.3, np.float32), seed=seed, stream=0)


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def _set_grads(net, g):
    net.ctx.h2d(net.ctx.lib.crux_mlp_grads_ptr(net.h), np.ascontiguousarray(g, np.float32))


def _loaded(dims, n_extra, rng, lam=0.7):
    """a handle with drawn parameters and a regulariser with drawn F and theta_prev"""
    net = _gauss(dims, n_extra); theta, prev, F = FR.draw(rng, dims, n_extra)
    net.set_params(theta)
    R = crux.DiagonalFisherRegularizer(net, lam); R.set_(F=F, theta_prev=prev)
    return net, R, theta, prev, F


# ---------------------------------------------------------------------------------------------------------------- 1. crux_fisher_add
@pytest.mark.parametrize("dims,n_extra", PRIM, ids=PRIM_IDS)
def test_fisher_add_is_numpys_float32_running_mean_bit_for_bit(gpu_ctx, dims, n_extra):
    rng = np.random.default_rng(11); net = _gauss(dims, n_extra); n = net.n_params
    R = crux.DiagonalFisherRegularizer(net)
    assert R.N == 0 and not R.F.any() and np.array_equal(R.theta_prev, net.get_params())
    F = np.zeros(n, np.float32)
    for k in range(3):                                                  # three adds from N = 0 with different gradients
        g = rng.standard_normal(n).astype(np.float32)
        crux.add_fisher_information_diagonal_(R, grad=g)
        F = FR.add_f32(F, g, k)
        assert R.N == k + 1 and np.array_equal(R.F, F), k
    R.set_(N=1000)                                                      # one add at N0 = 1000
    g = rng.standard_normal(n).astype(np.float32)
    crux.add_fisher_information_diagonal_(R, grad=g)
    F = FR.add_f32(F, g, 1000)
    assert R.N == 1001 and np.array_equal(R.F, F)
    R2 = crux.DiagonalFisherRegularizer(net); R2.set_(F=F, N=5)         # times = 3 against three single adds
    crux.add_fisher_information_diagonal_(R2, grad=g, times=3)
    R.set_(N=5)
    for _ in range(3):
        crux.add_fisher_information_diagonal_(R, grad=g)
    assert R2.N == R.N == 8 and np.array_equal(R2.F, R.F) and np.array_equal(R.F, FR.add_f32(F, g, 5, times=3))
    assert not np.array_equal(R.F, F)


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. crux_fisher_reg
@pytest.mark.parametrize("dims,n_extra", PRIM, ids=PRIM_IDS)
def test_fisher_reg_value_and_gradient_match_the_yardstick(gpu_ctx, dims, n_extra):
    rng = np.random.default_rng(12); lam = 0.7; tab = FR.array_table(dims, n_extra)
    net, R, theta, prev, F = _loaded(dims, n_extra, rng, lam)
    v0, g0 = FR.value(theta, prev, F, lam, tab), FR.gradient(theta, prev, F, lam, tab)
    _set_grads(net, np.zeros(net.n_params, np.float32))
    v = R(accumulate=True); r = _grads(net)
    ev = abs(v - v0) / abs(v0); eg = float(np.max(np.abs(r - g0) / np.abs(g0)))
    print("FISHER reg %s: value %.3g, gradient %.3g relative" % (dims, ev, eg))
    assert ev < 1e-6 and eg < 1e-6
    flat = lam * float(np.mean(F.astype(np.float64) * (theta.astype(np.float64) - prev) ** 2))      # a mean over the flat vector is another number
    assert abs(flat - v0) > 1e-3 * abs(v0)
    assert R(accumulate=True) == v and R() == v                                                    # identical calls, identical bits
    # 3. accumulate: a prefilled gradient becomes exactly float32(g + r); accumulate = 0 leaves it bitwise unchanged
    g = rng.standard_normal(net.n_params).astype(np.float32)
    _set_grads(net, g); R(accumulate=True)
    assert np.array_equal(_grads(net), (g + r).astype(np.float32))
    _set_grads(net, g); assert R(accumulate=False) == v and np.array_equal(_grads(net), g)
    # F = 0 and lambda = 0 give the value 0 and no gradient
    R.lam = 0.0
    _set_grads(net, g); assert R(accumulate=True) == 0.0 and np.array_equal(_grads(net), g)
    R.lam = lam; R.set_(F=np.zeros(net.n_params, np.float32))
    assert R(accumulate=True) == 0.0 and np.array_equal(_grads(net), g)


# ---------------------------------------------------------------------------------------------------------------- 4. get / set / snapshot
def test_fisher_state_round_trip_and_snapshot(gpu_ctx):
    rng = np.random.default_rng(13); dims, n_extra = PRIM[0]
    net, R, theta, prev, F = _loaded(dims, n_extra, rng)
    R.set_(N=17)
    assert np.array_equal(R.F, F) and np.array_equal(R.theta_prev, prev) and R.N == 17 and R.lam == float(np.float32(0.7))
    R.set_(theta_prev=theta + 1)                                        # NULL = keep
    assert np.array_equal(R.F, F) and R.N == 17 and np.array_equal(R.theta_prev, (theta + 1).astype(np.float32))
    R.snapshot_()
    assert np.array_equal(R.theta_prev, net.get_params()) and R() == 0.0


# ---------------------------------------------------------------------------------------------------------------- 5. the regularised step
def _pair(kind, dims, acts, n, rng, seed=21):
    """the data of tests/test_gpu_dense_learner.py::_pair on a GPU network / buffer and their oracle twins"""
    od = dims[0]; ad = dims[-1] if kind != "value" else 2
    g, o = parity.make_pair(dims, acts, seed, 0, "gaussian" if kind == "gaussian" else "continuous", n_extra=dims[-1] if kind == "gaussian" else 0, extra_init=-0.3)
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), n, EXTRAS); ob = O.OBuffer(od, ad, L.ACTION_CONTINUOUS, n, EXTRAS)
    d = {"s": rng.standard_normal((od, n)).astype(np.float32), "sp": rng.standard_normal((od, n)).astype(np.float32), "r": rng.standard_normal((1, n)).astype(np.float32),
         "done": rng.random((1, n)) < 0.2, "episode_end": rng.random((1, n)) < 0.2}
    if "relu" in acts:
        d["s"] = np.ascontiguousarray(DR.kink_free_inputs(o.params, dims, acts, n, rng, 1e-4))
    d["a"] = rng.standard_normal((ad, n)).astype(np.float32)
    for k in EXTRAS:
        d[k] = rng.standard_normal((1, n)).astype(np.float32)
    d["logprob"] = (-1.2 * ad + 0.1 * rng.standard_normal((1, n))).astype(np.float32)
    gb.push_(d); ob.push(d)
    return g, o, gb, ob, d


def _oracle_reg_step(o, ob, cfg, ids, prev, F, lam, tab):
    """train!(pi, loss + R) in the oracle: its loss gradient, + the yardstick's gradient (Float32), its Adam. Returns (info row, the whole gradient, R's value)."""
    oinfo = np.zeros(L.INFO_N, np.float32); ids = np.ascontiguousarray(ids, np.int64)
    O.chk(O.lib().orc_loss_grad(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(oinfo)))
    val = FR.value(o.params, prev, F, lam, tab)
    o.grads[:] = (o.grads + FR.gradient(o.params, prev, F, lam, tab).astype(np.float32)).astype(np.float32)
    og = o.grads.copy()
    O.chk(O.lib().orc_adam_apply(o.h, 1.0))
    return oinfo, og, val


STEP_CASES = [("gaussian", [3, 32, 128, 1], "tanh", 128, 2 * 128 + 37),      # df_bwd_ok: the fused pullback would defer layer 0 -- the slots a wrong ordering loses; 37-row tail unfused
              ("value", [5, 48, 40, 1], "relu", 32, 70)]                    # 32, 32, 6


@pytest.mark.parametrize("kind,dims,act,bs,n", STEP_CASES, ids=["gaussian_ppo_3-32-128-1_bs128", "value_mse_5-48-40-1_bs32"])
def test_regularised_step_matches_oracle_plus_yardstick(gpu_ctx, capfd, kind, dims, act, bs, n):
    rng = np.random.default_rng(7); acts = [act] * (len(dims) - 2) + ["identity"]; lam = 0.7
    g, o, gb, ob, _ = _pair(kind, dims, acts, n, rng)
    tab = FR.array_table(dims, dims[-1] if kind == "gaussian" else 0)
    theta = o.params.copy(); prev = (theta + 0.1 * rng.standard_normal(o.n)).astype(np.float32); F = (rng.standard_normal(o.n) ** 2).astype(np.float32)
    R = crux.DiagonalFisherRegularizer(g, lam); R.set_(F=F, theta_prev=prev)
    loss = crux.value_mse_loss if kind == "value" else crux.ppo_loss
    lname, head = ("value_mse", "deterministic") if kind == "value" else ("ppo", "gaussian")
    o.adam_init(float(np.float32(3e-4)))
    perm = rng.permutation(n).astype(np.int64); cfg = parity.train_cfg(lname, head, bs, 1, max_batches=1)
    oinfo, og, val = _oracle_reg_step(o, ob, cfg, perm[:bs], prev, F, lam, tab)
    p1 = crux.TrainingParams(loss=loss, batch_size=bs, epochs=1, max_batches=1, name="x_", regularizer=R)
    info = crux.batch_train_(g, p1, P, gb, perms=perm[None, :] + 1)
    assert info["x_batches_trained"] == 1
    gg = _grads(g); scale = max(1.0, np.abs(og).max())
    first = slice(0, dims[0] * dims[1] + dims[1])
    print("FISHER STEP %s grad %.3g (layer 0: %.3g) of scale %.3g" % (dims, np.abs(gg - og).max(), np.abs(gg[first] - og[first]).max(), scale))
    assert np.abs(gg - og).max() < 1e-4 * scale
    want_loss = float(oinfo[L.INFO["loss"]]) + val; want_norm = float(np.sqrt(np.sum(og.astype(np.float64) ** 2)))
    print("FISHER STEP %s loss %.6g vs %.6g (R = %.4g), grad_norm %.6g vs %.6g" % (dims, info["x_loss"], want_loss, val, info["x_grad_norm"], want_norm))
    assert val > 1e-4                                                                   # the regulariser is a visible part of the loss
    assert abs(info["x_loss"] - want_loss) < 1e-4 * max(1.0, abs(want_loss))
    assert abs(info["x_grad_norm"] - want_norm) < 1e-4 * max(1.0, want_norm)
    assert np.abs(g.get_params() - o.params).max() < 2e-5
    m, v, bp = g.adam_state(); om, ov, obp = o.adam_state()
    assert np.abs(m - om).max() < 1e-5 * max(1, np.abs(om).max()) and np.abs(v - ov).max() < 1e-5 * max(1, np.abs(ov).max()) and np.allclose(bp, obp, rtol=1e-12)
    ob.permute(perm + 1)                                                                # the device left the buffer in the epoch's order
    # three more steps on the minibatches of another permutation, the last one ragged
    perm2 = rng.permutation(n).astype(np.int64); ob.permute(perm2 + 1)
    for st in range(0, n, bs):
        _oracle_reg_step(o, ob, cfg, np.arange(st, min(n, st + bs)), prev, F, lam, tab)
    p3 = crux.TrainingParams(loss=loss, optimizer=p1.optimizer, batch_size=bs, epochs=1, max_batches=3, name="x_", regularizer=R)
    info3 = crux.batch_train_(g, p3, P, gb, perms=perm2[None, :] + 1)
    assert info3["x_batches_trained"] == 3
    d = np.abs(g.get_params() - o.params).max(); print("FISHER STEP %s params after 4 steps %.3g" % (dims, d))
    assert d < 2e-5
    for k in gb.keys():
        assert np.array_equal(gb[k], ob[k]), k
    _not_generic(capfd)


# ---------------------------------------------------------------------------------------------------------------- 6. / 7. / 8. on 5-48-40-1
def _value_twin(rng_seed, n=70):
    rng = np.random.default_rng(rng_seed); dims, acts = [5, 48, 40, 1], ["relu", "relu", "identity"]
    g, o, gb, ob, d = _pair("value", dims, acts, n, rng)
    return g, gb, o, d, rng


def test_fresh_regulariser_changes_nothing(gpu_ctx, capfd):
    """F = 0: the chain with the regulariser and crux_batch_train on the same permutations agree bit for bit (the same dense launches; the hook adds zeros)."""
    n, bs, epochs = 70, 32, 2
    g1, b1, _, _, rng = _value_twin(31); g2, b2, _, _, _ = _value_twin(31)
    assert np.array_equal(g1.get_params(), g2.get_params()) and np.array_equal(b1["s"], b2["s"])
    perms = np.stack([rng.permutation(n) + 1 for _ in range(epochs)])
    R = crux.DiagonalFisherRegularizer(g1, 0.7)
    i1 = crux.batch_train_(g1, crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=epochs, name="c_", regularizer=R), {}, b1, perms=perms)
    i2 = crux.batch_train_(g2, crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=epochs, name="c_"), {}, b2, perms=perms)
    assert i1["c_batches_trained"] == i2["c_batches_trained"] == 6
    assert np.array_equal(g1.get_params(), g2.get_params())
    for a, b in zip(g1.adam_state(), g2.adam_state()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.array_equal(i1["_epoch_infos"], i2["_epoch_infos"]) and i1["c_loss"] == i2["c_loss"]
    assert not np.array_equal(R.theta_prev, g1.get_params())          # it did train
    _not_generic(capfd)


def test_chain_and_host_seam_agree(gpu_ctx):
    """The same three regularised steps through crux_batch_train_fisher and through core._batch_train_seam (crux_loss_grad on another learner, crux_fisher_reg, crux_adam_apply)."""
    n, bs = 70, 32; out = []
    for seam in (False, True):
        g, gb, o, _, rng = _value_twin(32)
        prev = (o.params + 0.1 * rng.standard_normal(o.n)).astype(np.float32); F = (rng.standard_normal(o.n) ** 2).astype(np.float32)
        perm = rng.permutation(n)[None, :] + 1
        R = crux.DiagonalFisherRegularizer(g, 0.7); R.set_(F=F, theta_prev=prev)
        p = crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=1, max_batches=3, name="c_", regularizer=R)
        if seam:
            core._ensure_opt(g, p); info = core._batch_train_seam(g, p, {}, gb, None, perm)
        else:
            info = crux.batch_train_(g, p, {}, gb, perms=perm)
        assert info["c_batches_trained"] == 3
        out.append((g.get_params(), info["c_loss"]))
    d = np.abs(out[0][0] - out[1][0]).max(); print("FISHER chain vs seam: params %.3g, loss %.6g vs %.6g" % (d, out[0][1], out[1][1]))
    assert d < 2e-5 and abs(out[0][1] - out[1][1]) < 1e-4 * max(1.0, abs(out[1][1]))


def test_nan_from_the_regulariser_is_reported_and_nothing_moves(gpu_ctx):
    """F[0] = Inf with theta = theta_prev: 0 x Inf is a NaN gradient entry -- the norm is NaN, CRUX_ENAN (training.jl:20), parameters and Adam state untouched."""
    n, bs = 70, 32
    g, gb, _, _, _ = _value_twin(33)
    opt = crux.Adam(np.float32(3e-4))
    crux.batch_train_(g, crux.TrainingParams(loss=crux.value_mse_loss, optimizer=opt, batch_size=bs, epochs=1, name="c_"), {}, gb)      # real steps first: the Adam state is not all zeros
    R = crux.DiagonalFisherRegularizer(g, 0.7)
    F = np.zeros(g.n_params, np.float32); F[0] = np.inf; R.set_(F=F)
    before = g.get_params(); m0, v0, bp0 = g.adam_state()
    assert np.abs(m0).max() > 0 and np.array_equal(R.theta_prev, before)
    with pytest.raises(crux.CruxError) as e:
        crux.batch_train_(g, crux.TrainingParams(loss=crux.value_mse_loss, optimizer=opt, batch_size=bs, epochs=2, name="c_", regularizer=R), {}, gb)
    assert e.value.code == L.ENAN and np.array_equal(g.get_params(), before)
    m1, v1, bp1 = g.adam_state()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(np.asarray(bp0), np.asarray(bp1))


# ---------------------------------------------------------------------------------------------------------------- 9. update_fisher_
def _loss_grad(g, gb, p, ids0):
    raw = np.zeros(L.INFO_N, np.float32); cfg = core._train_cfg(g, p, {}); ids0 = np.ascontiguousarray(ids0, np.int64)
    g.ctx.check(g.ctx.lib.crux_loss_grad(g.h, gb.h, C.byref(cfg), ids0.ctypes.data_as(C.c_void_p), ids0.size, raw.ctypes.data_as(C.c_void_p)))
    return _grads(g)


def test_update_fisher_literal_and_per_minibatch(gpu_ctx):
    n, bs = 70, 32
    g, gb, _, _, rng = _value_twin(34)
    p = crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=1, name="c_")
    R = crux.DiagonalFisherRegularizer(g, 1.0); R.set_(theta_prev=np.zeros(g.n_params, np.float32))
    s0 = gb["s"].copy(); perm = rng.permutation(n) + 1
    crux.update_fisher_(R, gb, p, {}, bs, perm=perm)                                    # the literal form: one whole-buffer gradient, three times
    assert np.array_equal(gb["s"], s0[:, perm - 1])                                     # shuffle!(D)
    gall = _loss_grad(g, gb, p, np.arange(n))
    assert R.N == 3 and np.array_equal(R.F, FR.add_f32(np.zeros(g.n_params, np.float32), gall, 0, times=3)) and np.abs(R.F).max() > 0
    assert np.array_equal(R.theta_prev, g.get_params())
    R2 = crux.DiagonalFisherRegularizer(g, 1.0); perm2 = rng.permutation(n) + 1
    crux.update_fisher_(R2, gb, p, {}, bs, per_minibatch=True, perm=perm2)
    F = np.zeros(g.n_params, np.float32)
    for k, st in enumerate(range(0, n, bs)):                                            # each partition's own gradient, the ragged last one included
        F = FR.add_f32(F, _loss_grad(g, gb, p, np.arange(st, min(n, st + bs))), k)
    assert R2.N == 3 and np.array_equal(R2.F, F) and not np.array_equal(R2.F, R.F)


# ---------------------------------------------------------------------------------------------------------------- 10. refusals and the fallback
def test_refusals_and_the_seam_fallback(gpu_ctx):
    sn = crux.ContinuousNetwork(crux.Chain(crux.DenseSN(4, 16, "relu"), crux.Dense(16, 1)), seed=1)
    with pytest.raises(crux.CruxError) as e:
        crux.DiagonalFisherRegularizer(sn)
    assert e.value.code == L.EUNSUP
    rng = np.random.default_rng(35); n, bs, lam = 70, 32, 0.7; dims = [3, 16, 2]; acts = ["tanh", "identity"]; tab = FR.array_table(dims, 2)
    out = []
    for reg in (False, True):
        g, o, gb, ob, _ = _pair("gaussian", dims, acts, n, np.random.default_rng(36))
        p = crux.TrainingParams(loss=crux.logpdf_bc_loss, batch_size=bs, epochs=1, max_batches=1)
        if reg:
            theta = g.get_params(); prev = (theta + 0.1 * rng.standard_normal(theta.size)).astype(np.float32); F = (rng.standard_normal(theta.size) ** 2).astype(np.float32)
            R = crux.DiagonalFisherRegularizer(g, lam); R.set_(F=F, theta_prev=prev); p.regularizer = R
            val = FR.value(theta, prev, F, lam, tab)
            # a foreign handle: R belongs to g, the call trains `other`
            other = _gauss(dims, 2); core._ensure_opt(other, p); cfg = core._train_cfg(other, p, P); raw = np.zeros(L.INFO_N, np.float32)
            assert g.ctx.lib.crux_batch_train_fisher(other.h, R.h, gb.h, C.byref(cfg), None, raw.ctypes.data_as(C.c_void_p), None) == L.EUNSUP
        info = crux.batch_train_(g, p, P, gb, perms=np.arange(1, n + 1)[None, :])
        assert info["batches_trained"] == 1
        out.append(info["loss"])
    print("FISHER logpdf_bc through the seam: loss %.6g vs %.6g + %.6g" % (out[1], out[0], val))
    assert val > 1e-4 and abs((out[1] - out[0]) - val) < 1e-4
