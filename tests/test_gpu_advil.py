"""GPU: AdVIL on the batch solver (crux_orthogonal_reg, crux_advil_d_step, crux_advil_actor_step, csrc/advil.hip; crux.AdVIL, crux.OrthogonalRegularizer) against the
float64 restatement of tests/advil_reference.py; solve(AdVIL) against the manual composition of the entry points; the device regularizer through the host seam of
train!; and a learning check on the committed Pendulum demonstrations.

Reference: src/model_free/il/AdVIL.jl, src/extras/orthogonal_regularization.jl, src/extras/gradient_penalty.jl, src/model_free/batch.jl. Tolerances are those of
tests/test_gpu_cql.py and tests/test_gpu_iq.py: 1e-4 relative on losses, norms and the steps' values, 1e-4 of the gradient scale on accumulated gradients, 2e-5
absolute on parameters after one Adam step. Entries whose float64 gradient is within 1e-3 of the gradient scale of zero are not compared after Adam (the first step
is lr sign(g) there); at most a quarter of the parameters may be left out that way. Network parameters are set from numpy, so every case can be run through the
yardstick alone, without a device: seeds and activations were fixed that way (no case leaves out more than 4.1 % of its parameters).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import advil_reference as R
import parity
from parity import crux, L

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LR = 1e-3
MAX_LEFT_OUT = 0.25


def _close(a, b, tol=1e-4):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _init(dims, rng, extra=0):
    """Glorot-uniform weights, small biases, in the flat Flux order"""
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o))
        out += [rng.uniform(-lim, lim, i * o), rng.normal(0, 0.1, o)]
    if extra:
        out.append(rng.normal(0, 0.1, extra))
    return np.concatenate(out).astype(np.float32)


def _acts(dims, act):
    return [act] * (len(dims) - 2) + ["identity"]


def case(od, ad, a_hidden, d_hidden, a_act, d_act, B, seed):
    """dims, activations, float32 parameters and a minibatch: everything a test and the yardstick need, from numpy alone"""
    rng = np.random.default_rng(seed)
    a_dims, d_dims = [od] + list(a_hidden) + [ad], [od + ad] + list(d_hidden) + [1]
    c = {"a_dims": a_dims, "d_dims": d_dims, "a_acts": _acts(a_dims, a_act), "d_acts": _acts(d_dims, d_act), "pa": _init(a_dims, rng), "pd": _init(d_dims, rng)}
    c["data"] = {"s": rng.normal(0, 1, (od, B)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, B)).astype(np.float32), "sp": rng.normal(0, 1, (od, B)).astype(np.float32),
                 "r": rng.normal(0, 1, (1, B)).astype(np.float32), "done": rng.random((1, B)) < 0.1}
    return c


def _nets(c):
    A = crux.ContinuousNetwork(parity.chain(c["a_dims"], c["a_acts"])); A.set_params(c["pa"])
    D = crux.ContinuousNetwork(parity.chain(c["d_dims"], c["d_acts"])); D.set_params(c["pd"])
    A.attach_optimizer(crux.Adam(np.float32(LR))); D.attach_optimizer(crux.Adam(np.float32(LR)))
    return A, D


def _buffer(ctx, data, discrete=False):
    od, ad, B = data["s"].shape[0], data["a"].shape[0], data["s"].shape[1]
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if discrete else crux.ContinuousSpace(ad), B, ctx=ctx)
    b.push_(data); return b


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def _set_grads(net, g):
    net.ctx.h2d(net.ctx.lib.crux_mlp_grads_ptr(net.h), np.ascontiguousarray(g, np.float32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _adam_check(p_new, p0, g_ref, what):
    want = R.adam_first_step(p0.astype(np.float64), g_ref, lr=LR)
    ok = np.abs(g_ref) > 1e-3 * np.abs(g_ref).max()
    left_out = 1.0 - ok.mean()
    print("%s: %.1f %% of %d parameters left out, max deviation %.3g" % (what, 100 * left_out, g_ref.size, np.abs(p_new[ok] - want[ok]).max()))
    assert left_out <= MAX_LEFT_OUT, left_out
    assert np.abs(p_new[ok] - want[ok]).max() < 2e-5


# ---- 1. the regularizer ------------------------------------------------------------------------------------------------------------------------------------------
def _orth(net, beta, accumulate):
    out = np.zeros(1, np.float32)
    net.ctx.check(net.ctx.lib.crux_orthogonal_reg(net.h, float(np.float32(beta)), int(accumulate), _vp(out)))
    return out[0]


def _weight_mask(dims, extra=0):
    m = []
    for i, o in zip(dims[:-1], dims[1:]):
        m += [np.ones(i * o, bool), np.zeros(o, bool)]
    return np.concatenate(m + [np.zeros(extra, bool)])


@pytest.mark.parametrize("beta", [1e-4, 1.0])
@pytest.mark.parametrize("dims,extra", [([17, 64, 64, 6], 6), ([3, 256, 256, 1], 0), ([5, 48, 40, 3], 0)], ids=["17-64-64-6+logsigma", "3-256-256-1", "5-48-40-3"])
def test_orthogonal_reg_value_and_gradient(gpu_ctx, dims, extra, beta):
    rng = np.random.default_rng(7)
    acts = _acts(dims, "relu"); p = _init(dims, rng, extra)
    if extra:
        net = crux.GaussianPolicy(parity.chain(dims, acts), np.zeros(extra, np.float32))
    else:
        net = crux.ContinuousNetwork(parity.chain(dims, acts))
    net.set_params(p)
    layers = R.mlp_params(p, dims)
    v_ref = R.orth_reg(layers, beta); v_ref.backward(); g_ref = np.concatenate([R.flat_grad(layers), np.zeros(extra)])
    assert _close(crux.orthogonal_regularizer(net, beta), v_ref.item())
    g0 = rng.normal(0, 1, net.n_params).astype(np.float32); _set_grads(net, g0)
    v = _orth(net, beta, True)
    print("orth %s beta %g: value %.8g (float64 %.8g)" % (dims, beta, v, v_ref.item()))
    assert _close(v, v_ref.item()), (v, v_ref.item())
    g = _grads(net); w = _weight_mask(dims, extra)
    assert np.array_equal(_bits(g[~w]), _bits(g0[~w]))                      # bias and extra slots: untouched
    scale = max(1.0, np.abs(g_ref).max())
    assert np.abs((g.astype(np.float64) - g0) - g_ref).max() <= 1e-4 * scale
    # onto a zero buffer the sum is the gradient itself: two float32 products of depth <= 256 keep 1e-4 of its scale whatever beta is
    _set_grads(net, np.zeros_like(g0)); _orth(net, beta, True)
    assert np.abs(_grads(net).astype(np.float64) - g_ref).max() <= 1e-4 * np.abs(g_ref).max()
    # two identical calls: identical bits
    _set_grads(net, g0); v2 = _orth(net, beta, True)
    assert np.array_equal(_bits(_grads(net)), _bits(g)) and _bits(np.array([v2]))[0] == _bits(np.array([v]))[0]
    # value only: the buffer stays; beta = 0: value 0, buffer untouched
    _set_grads(net, g0)
    assert _bits(np.array([_orth(net, beta, False)]))[0] == _bits(np.array([v]))[0] and np.array_equal(_bits(_grads(net)), _bits(g0))
    assert _orth(net, 0.0, True) == 0.0 and np.array_equal(_bits(_grads(net)), _bits(g0))


# ---- 2. / 3. the two steps against the yardstick -----------------------------------------------------------------------------------------------------------------
D_CASES = [("relu", 128), ("relu", 37), ("tanh", 128), ("tanh", 37)]


@pytest.mark.parametrize("d_act,B", D_CASES, ids=["%s-B%d" % c for c in D_CASES])
def test_d_step_matches_reference(gpu_ctx, d_act, B):
    seed, ctr, lam = 11, 8 * 3 + 5, 10.0
    c = case(6, 3, [32, 32], [48, 48], "tanh", d_act, B, seed=2)
    A, D = _nets(c); b = _buffer(gpu_ctx, c["data"])
    al, dl = R.mlp_params(c["pa"], c["a_dims"]), R.mlp_params(c["pd"], c["d_dims"])
    loss, ref = R.advil_d_loss(al, c["a_acts"], dl, c["d_acts"], c["data"]["s"], c["data"]["a"], lam, seed, ctr)
    loss.backward(); g_ref = R.flat_grad(dl)
    ga0 = np.random.default_rng(1).normal(0, 1, A.n_params).astype(np.float32); _set_grads(A, ga0)
    raw, adv = crux.advil_d_step_(A, D, b, lam, seed, ctr)
    print("d step %s B %d: loss %.8g (%.8g) norm %.8g (%.8g) adv %s ref %s" % (d_act, B, raw[0], loss.item(), raw[1], np.linalg.norm(g_ref), adv, ref))
    assert _close(raw[L.INFO["loss"]], loss.item()), (raw[0], loss.item())
    assert _close(raw[L.INFO["grad_norm"]], np.linalg.norm(g_ref)), (raw[1], np.linalg.norm(g_ref))
    for k, key in enumerate(("D_expert", "D_policy", "grad_pen", "gp_loss")):
        assert _close(adv[k], ref[key]), (key, adv[k], ref[key])
    _adam_check(D.get_params(), c["pd"], g_ref, "discriminator")
    assert np.array_equal(_bits(A.get_params()), _bits(c["pa"])) and np.array_equal(_bits(_grads(A)), _bits(ga0))      # the actor: untouched


@pytest.mark.parametrize("beta", [1e-4, 1.0])
def test_actor_step_matches_reference(gpu_ctx, beta):
    lam = 0.2
    c = case(6, 3, [32, 32], [48, 48], "tanh", "tanh", 128, seed=3)
    A, D = _nets(c); b = _buffer(gpu_ctx, c["data"])
    al, dl = R.mlp_params(c["pa"], c["a_dims"]), R.mlp_params(c["pd"], c["d_dims"])
    lp, ref = R.advil_pi_loss(al, c["a_acts"], dl, c["d_acts"], c["data"]["s"], c["data"]["a"], lam)
    reg = R.orth_reg(al, beta); tot = lp + reg
    tot.backward(); g_ref = R.flat_grad(al)
    raw, adv = crux.advil_actor_step_(A, D, b, lam, beta)
    print("actor step beta %g: loss %.8g (%.8g) norm %.8g (%.8g) adv %s ref %s reg %.8g" % (beta, raw[0], tot.item(), raw[1], np.linalg.norm(g_ref), adv, ref, reg.item()))
    assert _close(raw[L.INFO["loss"]], tot.item()), (raw[0], tot.item())
    assert _close(raw[L.INFO["grad_norm"]], np.linalg.norm(g_ref)), (raw[1], np.linalg.norm(g_ref))
    assert _close(adv[0], ref["D_policy"]) and _close(adv[1], ref["bc_mse"]) and _close(adv[2], reg.item()), (adv, ref, reg.item())
    _adam_check(A.get_params(), c["pa"], g_ref, "actor")
    assert np.array_equal(_bits(D.get_params()), _bits(c["pd"]))                                                        # the discriminator: untouched


def test_actor_step_relu_networks(gpu_ctx):
    """relu in both networks (the dense engine's fused pullback pair), a short minibatch"""
    c = case(6, 3, [32, 32], [64, 64], "relu", "relu", 37, seed=5)
    A, D = _nets(c); b = _buffer(gpu_ctx, c["data"])
    al, dl = R.mlp_params(c["pa"], c["a_dims"]), R.mlp_params(c["pd"], c["d_dims"])
    lp, ref = R.advil_pi_loss(al, c["a_acts"], dl, c["d_acts"], c["data"]["s"], c["data"]["a"], 0.2)
    tot = lp + R.orth_reg(al, 1.0); tot.backward(); g_ref = R.flat_grad(al)
    raw, adv = crux.advil_actor_step_(A, D, b, 0.2, 1.0)
    assert _close(raw[0], tot.item()) and _close(raw[1], np.linalg.norm(g_ref)) and _close(adv[1], ref["bc_mse"]), (raw[:2], tot.item(), adv, ref)
    _adam_check(A.get_params(), c["pa"], g_ref, "actor (relu)")


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------------------------------
def test_steps_are_deterministic(gpu_ctx):
    c = case(17, 6, [64, 64], [256, 256], "tanh", "tanh", 256, seed=4)
    outs = []
    for _ in range(2):
        A, D = _nets(c); b = _buffer(gpu_ctx, c["data"])
        r1, a1 = crux.advil_d_step_(A, D, b, 10.0, 5, 13)
        r2, a2 = crux.advil_actor_step_(A, D, b, 0.2, 1e-4)
        outs.append((D.get_params(), A.get_params(), r1, a1, r2, a2))
    assert all(np.array_equal(_bits(outs[0][k]), _bits(outs[1][k])) for k in range(6))
    assert not np.array_equal(outs[0][0], c["pd"]) and not np.array_equal(outs[0][1], c["pa"])


# ---- 5. NaN ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", ["d", "actor"])
@pytest.mark.parametrize("col", ["s", "a"])
def test_nan_raises_and_leaves_parameters(gpu_ctx, col, step):
    c = case(4, 2, [32, 32], [64, 64], "relu", "relu", 32, seed=6)
    c["data"][col][1, 29] = np.nan
    A, D = _nets(c); b = _buffer(gpu_ctx, c["data"])
    with pytest.raises(L.CruxError) as e:
        if step == "d":
            crux.advil_d_step_(A, D, b, 10.0, 1, 5)
        else:
            crux.advil_actor_step_(A, D, b, 0.2, 1e-4)
    assert e.value.code == L.ENAN and "NaN detected" in str(e.value)
    assert np.array_equal(_bits(A.get_params()), _bits(c["pa"])) and np.array_equal(_bits(D.get_params()), _bits(c["pd"]))


# ---- 6. rejections -----------------------------------------------------------------------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    c = case(4, 2, [16], [16], "relu", "relu", 16, seed=8)
    A, D = _nets(c)
    disc = dict(c["data"]); disc["a"] = np.eye(2, dtype=bool)[np.random.default_rng(0).integers(0, 2, 16)].T.copy()
    bd = _buffer(gpu_ctx, disc, discrete=True)
    for call in (lambda b_, D_: crux.advil_d_step_(A, D_, b_, 10.0, 1, 5), lambda b_, D_: crux.advil_actor_step_(A, D_, b_, 0.2, 1e-4)):
        with pytest.raises(L.CruxError) as e:
            call(bd, D)
        assert e.value.code == L.EINVAL
        wrong = crux.ContinuousNetwork(parity.chain([5, 16, 1], ["relu", "identity"])); wrong.attach_optimizer(crux.Adam(np.float32(LR)))
        with pytest.raises(L.CruxError) as e:
            call(_buffer(gpu_ctx, c["data"]), wrong)
        assert e.value.code == L.EINVAL
    assert np.array_equal(_bits(A.get_params()), _bits(c["pa"])) and np.array_equal(_bits(D.get_params()), _bits(c["pd"]))
    S, demo = crux.ContinuousSpace(4), _buffer(gpu_ctx, c["data"])
    G = crux.GaussianPolicy(parity.chain([4, 16, 2], ["relu", "identity"]), np.zeros(2, np.float32))
    with pytest.raises(TypeError):
        crux.AdVIL(crux.ActorCritic(G, D), S, demo)
    with pytest.raises(TypeError):
        crux.AdVIL(crux.ActorCritic(A, crux.DoubleNetwork(D, D)), S, demo)
    sv = crux.AdVIL(crux.ActorCritic(A, D), S, demo, a_opt={"regularizer": lambda theta: (0.0, np.zeros_like(theta)), "epochs": 0})
    with pytest.raises(NotImplementedError):
        crux.solve(sv)
    assert np.array_equal(_bits(A.get_params()), _bits(c["pa"]))


# ---- 7. the solver against the manual composition ------------------------------------------------------------------------------------------------------------------
def test_solve_matches_manual_composition(gpu_ctx):
    ctx, n, B, nseed = gpu_ctx, 300, 128, 17
    c = case(5, 2, [32, 32], [64, 64], "tanh", "tanh", n, seed=9)
    S = crux.ContinuousSpace(5, mu=np.linspace(-0.5, 0.5, 5).astype(np.float32), sigma=np.linspace(0.5, 2.0, 5).astype(np.float32))
    keys = {"discriminator_loss", "discriminator_grad_norm", "actor_loss", "actor_grad_norm", "D_expert", "D_policy", "grad_pen", "bc_mse", "orth_reg"}
    runs = []
    for manual in (False, True):
        A, D = _nets(c); demo = _buffer(ctx, c["data"])
        if not manual:
            sv = crux.AdVIL(crux.ActorCritic(A, D), S, demo, a_opt={"epochs": 1, "batch_size": B}, noise_seed=nseed)
            crux.solve(sv)
            assert sv.D_train is not demo and all(np.array_equal(demo[k], c["data"][k]) for k in ("s", "a", "sp"))      # the caller's buffer: as it was
            assert not np.array_equal(sv.D_train["s"], c["data"]["s"])
            runs.append((A.get_params(), D.get_params(), sv.history)); continue
        opt_a, opt_d = crux.Adam(np.float32(3e-4)), crux.Adam(np.float32(3e-4))
        A.attach_optimizer(opt_a); D.attach_optimizer(opt_d)
        Dn = crux.normalize_(crux.copy_buffer(demo), S, crux.ContinuousSpace(2))
        mb = crux.buffer_like(Dn, capacity=B)
        hist, g = [], 0
        for ep in range(2):
            crux.shuffle_device_(Dn, 0, ep)
            infos = []
            for k0 in range(0, n, B):
                m = min(B, n - k0)
                mb.clear_(); mb.push_(Dn, ids=np.arange(k0 + 1, k0 + m + 1))
                rd, ad_ = crux.advil_d_step_(A, D, mb, 10.0, nseed, 8 * g + 5)
                ra, aa = crux.advil_actor_step_(A, D, mb, 0.2, 1e-4)
                infos.append({"D_expert": float(ad_[0]), "D_policy": float(ad_[1]), "grad_pen": float(ad_[2]), "discriminator_loss": float(rd[0]),
                              "discriminator_grad_norm": float(rd[1]), "actor_loss": float(ra[0]), "actor_grad_norm": float(ra[1]), "bc_mse": float(aa[1]), "orth_reg": float(aa[2])})
                g += 1
            assert [len(range(k0, min(n, k0 + B))) for k0 in range(0, n, B)] == [128, 128, 44]
            hist.append(crux.aggregate_info(infos))
        runs.append((A.get_params(), D.get_params(), hist))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert len(runs[0][2]) == len(runs[1][2]) == 2
    for h0, h1 in zip(runs[0][2], runs[1][2]):
        assert set(h0) == keys and all(h0[k] == h1[k] for k in keys), (h0, h1)
    assert not np.array_equal(runs[0][0], c["pa"]) and not np.array_equal(runs[0][1], c["pd"])


# ---- 8. the regularizer through the host seam ----------------------------------------------------------------------------------------------------------------------
def test_regularizer_through_the_host_seam(gpu_ctx):
    n, dims = 96, [6, 32, 32, 3]
    c = case(6, 3, [32, 32], [8], "tanh", "tanh", n, seed=10)
    s, a = c["data"]["s"], c["data"]["a"]
    layers = R.mlp_params(c["pa"], dims)
    tot = ((R.mlp(layers, c["a_acts"], torch.as_tensor(s.astype(np.float64))) - torch.as_tensor(a.astype(np.float64))) ** 2).mean() + R.orth_reg(layers, 1.0)
    tot.backward(); g_ref = R.flat_grad(layers)

    def host_reg(theta):
        ls = R.mlp_params(theta, dims); v = R.orth_reg(ls, 1.0); v.backward()
        return v.item(), R.flat_grad(ls)
    outs = []
    for reg in (crux.OrthogonalRegularizer(1.0), host_reg):
        A = crux.ContinuousNetwork(parity.chain(dims, c["a_acts"])); A.set_params(c["pa"])
        p = crux.TrainingParams(loss=crux.mse_action_loss, regularizer=reg, batch_size=n, epochs=1, optimizer=crux.Adam(np.float32(LR)))
        info = crux.batch_train_(A, p, {}, _buffer(gpu_ctx, c["data"]))
        assert info["batches_trained"] == 1
        assert _close(info["loss"], tot.item()) and _close(info["grad_norm"], np.linalg.norm(g_ref)), (info, tot.item(), np.linalg.norm(g_ref))
        _adam_check(A.get_params(), c["pa"], g_ref, "seam (%s)" % type(reg).__name__)
        outs.append((A.get_params(), info))
    assert np.abs(outs[0][0] - outs[1][0]).max() < 2e-5
    assert _close(outs[0][1]["loss"], outs[1][1]["loss"]) and _close(outs[0][1]["grad_norm"], outs[1][1]["grad_norm"])


# ---- 9. learning -------------------------------------------------------------------------------------------------------------------------------------------------
LEARN = {"seed": 0, "epochs": 60, "batch_size": 128, "a_dims": [2, 64, 64, 1], "d_dims": [3, 64, 64, 1], "act": "tanh"}      # profiles/advil_learning.txt


def learning_setup():
    """the Pendulum demonstrations, whitened by their own statistics; the last 30 % of a fixed permutation held out"""
    d = dict(np.load(os.path.join(GOLD, "pendulum_transitions.npz")))
    mu, sg = d["s"].mean(1).astype(np.float32), d["s"].std(1).astype(np.float32)
    n = d["s"].shape[1]; order = np.random.default_rng(LEARN["seed"]).permutation(n); cut = int(round(0.7 * n))
    tr, va = order[:cut], order[cut:]
    rng = np.random.default_rng(LEARN["seed"] + 1)
    return d, mu, sg, tr, va, _init(LEARN["a_dims"], rng), _init(LEARN["d_dims"], rng)


def test_advil_lowers_the_held_out_bc_error(gpu_ctx):
    """AdVIL's defaults (lambda_GP 10, lambda_orth 1e-4, lambda_BC 0.2, Adam(3e-4)) for LEARN["epochs"] + 1 epochs over 358 demonstration rows: the held-out
    mean((pi(s) - a)^2) must fall. The float64 loop of advil_reference.py at this setting and the values measured on the GPU are in profiles/advil_learning.txt."""
    d, mu, sg, tr, va, pa, pd = learning_setup()
    S = crux.ContinuousSpace(2, mu=mu, sigma=sg)
    acts = _acts(LEARN["a_dims"], LEARN["act"])
    A = crux.ContinuousNetwork(parity.chain(LEARN["a_dims"], acts)); A.set_params(pa)
    D = crux.ContinuousNetwork(parity.chain(LEARN["d_dims"], acts)); D.set_params(pd)
    cols = ("s", "a", "sp", "r", "done")
    demo = _buffer(gpu_ctx, {k: np.ascontiguousarray(d[k][:, tr]) for k in cols})
    held = crux.normalize_(_buffer(gpu_ctx, {k: np.ascontiguousarray(d[k][:, va]) for k in cols}), S, crux.ContinuousSpace(1))
    sv, av = held["s"], held["a"]
    err = lambda: float(np.mean((A.forward(sv).astype(np.float64) - av) ** 2))      # noqa: E731
    before = err()
    sv_ = crux.AdVIL(crux.ActorCritic(A, D), S, demo, a_opt={"epochs": LEARN["epochs"], "batch_size": LEARN["batch_size"]})
    crux.solve(sv_)
    after = err()
    print("advil pendulum: held-out bc mse %.6f -> %.6f; last epoch %s" % (before, after, sv_.history[-1]))
    assert len(sv_.history) == LEARN["epochs"] + 1 and all(np.isfinite(v) for h in sv_.history for v in h.values())
    assert after < before, (before, after)
