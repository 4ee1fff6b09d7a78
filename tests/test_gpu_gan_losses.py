"""GPU: the LS, hinge, W and WGP discriminator losses of the on-policy GAIL family (src/extras/gans.jl; GanHeadOp in csrc/sac.hip, crux_gail_d_step_gan,
crux_gail_d_batch_train_gan and crux_nda_gail_round_gan in csrc/nda_gail.hip, the shared Wasserstein + penalty sequence in csrc/advil.hip; crux.GANLosses,
OnPolicyGAIL(gan_loss=...), NDA_GAIL_JS(gan_loss=...)) against the float64 yardstick of tests/gan_reference.py and, where an entry replaces a composition, against that
composition bit for bit.

Tolerances are the project's (tests/test_gpu_cql.py, test_gpu_iq.py): 1e-4 relative on losses and norms; the raw gradient (crux_mlp_grads_ptr) to 1e-4 of its largest
entry; 2e-5 absolute on parameters after one Adam step at lr = 1e-3, where entries whose float64 gradient is non-zero but within 1e-3 of the gradient's scale of zero are
not compared (the first Adam step is lr sign(g) there) and entries that are exactly zero in float64 are. Inputs come from tests/gan_cases.py (numpy alone);
tests/test_gan_reference.py asserts on the yardstick that no output sits within 1e-3 of a hinge kink, that both sides of each kink are populated and that at most 5 % of
the entries fall under the exclusion rule.
"""
import ctypes as C
import os

import numpy as np
import pytest

import gan_cases as GC
import gan_reference as GR
import iq_reference as IQ
import parity
from parity import crux, L

pytestmark = pytest.mark.gpu

LR = 1e-3
SEED = 41
KIND = GR.KINDS
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _net(ctx, c, p=None):
    n = crux.ContinuousNetwork(parity.chain(list(c["dims"]), list(c["acts"])), ctx=ctx)
    n.set_params(c["p"] if p is None else p); n.attach_optimizer(crux.Adam(np.float32(LR)))
    return n


def _buffer(ctx, c, rows, n=None):
    n = rows["s"].shape[1] if n is None else n
    A = crux.DiscreteSpace(c["ad"]) if c["disc"] else crux.ContinuousSpace(c["ad"])
    b = crux.ExperienceBuffer(crux.ContinuousSpace(c["od"]), A, n, [], ctx=ctx)
    b.push_({k: v[:, :n] for k, v in rows.items()}); return b


def _grads(net):
    g = np.empty(net.n_params, np.float32); net.ctx.d2h(net.ctx.lib.crux_mlp_grads_ptr(net.h), g); return g


def _step(net, ex, n_ex, pi, n_pi, kind, lam=GC.LAM, seed=GC.GP_SEED, counter=GC.GP_COUNTER, off_ex=0, off_pi=0):
    info = np.zeros(L.INFO_N, np.float32)
    rc = net.ctx.lib.crux_gail_d_step_gan(net.h, ex.h, off_ex, n_ex, pi.h, off_pi, n_pi, KIND[kind], lam, seed, counter, _vp(info))
    return rc, info


def _err(ctx):
    return (ctx.lib.crux_last_error(ctx.h) or b"").decode()


def _check_against_yardstick(net, info, c, loss, g, tag):
    gn = np.linalg.norm(g); got_g = _grads(net); got = net.get_params().astype(np.float64)
    want = GR.adam_first_step(c["p"].astype(np.float64), g, lr=LR)
    skip, share = GC.skipped(g); ok = ~skip
    print("%s: loss %.8g (%.8g) norm %.8g (%.8g) grad err %.3g of %.3g, param err %.3g, %.2f %% not compared" % (
        tag, info[L.INFO["loss"]], loss, info[L.INFO["grad_norm"]], gn, np.abs(got_g - g).max(), np.abs(g).max(), np.abs(got[ok] - want[ok]).max(), 100 * share))
    assert abs(info[L.INFO["loss"]] - loss) <= 1e-4 * max(1.0, abs(loss))
    assert abs(info[L.INFO["grad_norm"]] - gn) <= 1e-4 * max(1.0, gn)
    assert np.abs(got_g - g).max() <= 1e-4 * np.abs(g).max()
    assert share <= 0.05
    assert np.abs(got[ok] - want[ok]).max() < 2e-5 and np.isfinite(got).all()


# ---- 1. one step of LS / hinge / W against the yardstick -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", GC.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", GC.HEAD_KINDS)
@pytest.mark.parametrize("name", list(GC.CASES))
def test_step_matches_reference(gpu_ctx, name, kind, sizes):
    c = GC.case(name); n_ex, n_pi = sizes
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, c["pi"])
    loss, g = GR.d_step(kind, c["p"], c["dims"], c["acts"], GC.x_of(c["ex"], n_ex), GC.x_of(c["pi"], n_pi))
    a, b = _net(gpu_ctx, c), _net(gpu_ctx, c)
    rc, info = _step(a, ex, n_ex, pi, n_pi, kind); gpu_ctx.check(rc)
    _check_against_yardstick(a, info, c, loss, g, "%s %s %s" % (name, kind, sizes))
    rc, info2 = _step(b, ex, n_ex, pi, n_pi, kind); gpu_ctx.check(rc)      # two identical calls: identical bits
    assert _same(info, info2) and _same(a.get_params(), b.get_params()) and _same(_grads(a), _grads(b))


# ---- 2. one step of WGP -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GC.WGP_SIZES)
@pytest.mark.parametrize("name", list(GC.CASES))
def test_wgp_step_matches_reference(gpu_ctx, name, n):
    """relu networks run the first-order sweep only, the tanh one the second-order sweep too. The yardstick interpolates with iq_reference.eps(seed, counter): a device
    draw from another (seed, counter) moves the loss by far more than 1e-4 (tests/test_gan_reference.py)."""
    c = GC.case(name)
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, c["pi"])
    loss, g = GR.d_step("WGP", c["p"], c["dims"], c["acts"], GC.x_of(c["ex"], n), GC.x_of(c["pi"], n), GC.LAM, GC.GP_SEED, GC.GP_COUNTER)
    a, b = _net(gpu_ctx, c), _net(gpu_ctx, c)
    rc, info = _step(a, ex, n, pi, n, "WGP"); gpu_ctx.check(rc)
    _check_against_yardstick(a, info, c, loss, g, "%s WGP %d" % (name, n))
    rc, info2 = _step(b, ex, n, pi, n, "WGP"); gpu_ctx.check(rc)
    assert _same(info, info2) and _same(a.get_params(), b.get_params())


def test_wgp_draw_is_iq_references_eps(gpu_ctx):
    """the interpolated columns themselves: crux_gradient_penalty(seed, counter) is documented as the same draw; here the WGP step at (seed, counter + 1) must match the
    yardstick at counter + 1 and miss the one at counter"""
    c = GC.case("cont-tanh"); n = 255
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, c["pi"])
    xe, xp = GC.x_of(c["ex"], n), GC.x_of(c["pi"], n)
    l0, _ = GR.d_step("WGP", c["p"], c["dims"], c["acts"], xe, xp, GC.LAM, GC.GP_SEED, GC.GP_COUNTER)
    l1, _ = GR.d_step("WGP", c["p"], c["dims"], c["acts"], xe, xp, GC.LAM, GC.GP_SEED, GC.GP_COUNTER + 1)
    net = _net(gpu_ctx, c)
    rc, info = _step(net, ex, n, pi, n, "WGP", counter=GC.GP_COUNTER + 1); gpu_ctx.check(rc)
    assert abs(info[0] - l1) <= 1e-4 * abs(l1) and abs(info[0] - l0) > 1e-3 * abs(l0)
    e = IQ.eps(GC.GP_SEED, GC.GP_COUNTER + 1, n)
    assert e.dtype == np.float32 and 0 <= e.min() and e.max() < 1


def test_wgp_refusals_leave_the_parameters(gpu_ctx):
    import test_gpu_sn as TS
    c = GC.case("cont-relu")
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, c["pi"])
    net = _net(gpu_ctx, c)
    rc, _ = _step(net, ex, 40, pi, 41, "WGP")
    msg = _err(gpu_ctx)
    assert rc == L.EINVAL and "40" in msg and "41" in msg, (rc, msg)
    assert _same(net.get_params(), c["p"])
    rc, _ = _step(net, ex, 40, pi, 40, "WGP", off_pi=GC.POOL - 39)
    assert rc == L.EINVAL and _same(net.get_params(), c["p"])
    info = np.zeros(L.INFO_N, np.float32)
    assert gpu_ctx.lib.crux_gail_d_step_gan(net.h, ex.h, 0, 8, pi.h, 0, 8, 5, 10.0, 0, 0, _vp(info)) == L.EINVAL and "unknown loss kind" in _err(gpu_ctx)
    s = TS.case("3-12-1", 1); sn = TS._net(gpu_ctx, s); rng = np.random.default_rng(0)
    bex, bpi = TS._buffer(gpu_ctx, TS._rows(rng, 2, 1, 40), 2, 1), TS._buffer(gpu_ctx, TS._rows(rng, 2, 1, 40), 2, 1)
    rc, _ = _step(sn, bex, 21, bpi, 21, "WGP")
    assert rc == L.EUNSUP and "crux_gail_d_step_gan" in _err(gpu_ctx), _err(gpu_ctx)
    assert _same(sn.get_params(), s["p"])



# ---- 3. kind BCE is crux_gail_d_step ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cont-tanh", "disc-relu"])
def test_bce_kind_is_gail_d_step_bit_for_bit(gpu_ctx, name):
    c = GC.case(name)
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, c["pi"])
    a, b = _net(gpu_ctx, c), _net(gpu_ctx, c)
    for (oe, ne, op, npi) in [(0, 255, 0, 257), (3, 44, 7, 128)]:      # two steps in a row: the Adam state carries on identically
        rc, info = _step(a, ex, ne, pi, npi, "BCE", off_ex=oe, off_pi=op); gpu_ctx.check(rc)
        want = np.zeros(L.INFO_N, np.float32)
        gpu_ctx.check(gpu_ctx.lib.crux_gail_d_step(b.h, ex.h, oe, ne, pi.h, op, npi, _vp(want)))
        assert _same(info, want) and _same(a.get_params(), b.get_params()) and np.isfinite(want[:2]).all() and want[1] > 0
    assert not _same(a.get_params(), c["p"])


# ---- 4. DenseSN discriminators ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Hinge", "W"])
@pytest.mark.parametrize("name,n_iter", [("3-12-1", 1), ("3-64-64-2-1", 3)])
def test_densesn_step_matches_sn_reference(gpu_ctx, name, n_iter, kind):
    """tests/test_gpu_sn.py's discriminator step (rows [1, 34) and [2, 23), one forward call over both halves, u advances once) with the new head: the seeds are the
    yardstick's autograd gradient of the loss in z, pulled back through sn_reference's analytic DenseSN gradient; that file's checks and tolerances (_check_step)"""
    import sn_reference as SR
    import test_gpu_sn as TS
    c = TS.case(name, n_iter); od = c["dims"][0] - 1
    ex, pi = TS._rows(c["rng"], od, 1, 40), TS._rows(c["rng"], od, 1, 30)
    x = np.concatenate([np.concatenate([ex["a"][:, 1:34], ex["s"][:, 1:34]], 0), np.concatenate([pi["a"][:, 2:23], pi["s"][:, 2:23]], 0)], 1)
    z, cache = SR.forward(c["p"], c["dims"], c["acts"], c["sn"], c["us"], x)
    import torch
    zt = torch.as_tensor(z.reshape(-1)); loss = GR.loss_of_z(kind, zt[:33], zt[33:]).item()
    g, _ = SR.backward(cache, GR.dz(kind, z, 33).reshape(1, -1))
    net, bex, bpi = TS._net(gpu_ctx, c), TS._buffer(gpu_ctx, ex, od, 1), TS._buffer(gpu_ctx, pi, od, 1)
    u0 = [u.copy() for u, _, _ in net.spectral_state()]
    rc, info = _step(net, bex, 33, bpi, 21, kind, off_ex=1, off_pi=2); gpu_ctx.check(rc)
    assert np.isfinite(info[:2]).all()
    TS._check_step(net, info, c, loss, g, cache)
    # u advanced as it does for BCE: the same starting u, the same weights, one forward call
    ref = TS._net(gpu_ctx, c); want = np.zeros(L.INFO_N, np.float32)
    gpu_ctx.check(gpu_ctx.lib.crux_gail_d_step(ref.h, bex.h, 1, 33, bpi.h, 2, 21, _vp(want)))
    for (u, v, s), (ur, vr, sr), ub in zip(net.spectral_state(), ref.spectral_state(), u0):
        assert np.array_equal(u, ur) and np.array_equal(v, vr) and s == sr and not np.array_equal(u, ub)


# ---- 5. the chain against the host loop --------------------------------------------------------------------------------------------------------------------------------
def _host_loop(D, ex, pi, B, epochs, counter, kind, max_batches=None):
    import nda_gail_reference as NR
    rows, total = [], 0
    for ep in range(epochs):
        crux.shuffle_device_(ex, SEED, 2 * (counter + ep)); crux.shuffle_device_(pi, SEED, 2 * (counter + ep) + 1)
        raw = None
        for (_e, oe, ne, op, np_) in NR.partition_plan(len(ex), len(pi), B, 1):
            rc, raw = _step(D, ex, ne, pi, np_, kind, off_ex=oe, off_pi=op); D.ctx.check(rc); total += 1
            if max_batches and total >= max_batches:
                break
        rows.append(raw)
        if max_batches and total >= max_batches:
            break
    return np.array(rows), total


def _chain(D, ex, pi, B, epochs, counter, kind, max_batches=0):
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((epochs, L.INFO_N), np.float32)
    rc = D.ctx.lib.crux_gail_d_batch_train_gan(D.h, ex.h, pi.h, B, epochs, max_batches, SEED, counter, KIND[kind], _vp(raw), _vp(rows))
    return rc, raw, rows


def _chain_case():
    """300 expert rows, 520 policy rows, B = 128: three pairs per epoch, the last with halves 44 / 128"""
    c = GC.case("cont-relu"); rng = np.random.default_rng(5)
    return c, c["ex"], GC.rows(rng, c["od"], c["ad"], 520, c["disc"])


@pytest.mark.parametrize("max_batches", [0, 4], ids=["all", "stop-in-epoch-2"])
@pytest.mark.parametrize("kind", ["Hinge", "LS"])
def test_chain_is_the_host_loop(gpu_ctx, kind, max_batches):
    import nda_gail_reference as NR
    c, ex_rows, pi_rows = _chain_case(); B = 128
    assert [(ne, np_) for (_e, _oe, ne, _op, np_) in NR.partition_plan(300, 520, B, 1)] == [(128, 128), (128, 128), (44, 128)]
    a, b = _net(gpu_ctx, c), _net(gpu_ctx, c)
    exa, pia, exb, pib = _buffer(gpu_ctx, c, ex_rows), _buffer(gpu_ctx, c, pi_rows), _buffer(gpu_ctx, c, ex_rows), _buffer(gpu_ctx, c, pi_rows)
    rc, raw, rows = _chain(a, exa, pia, B, 2, 11, kind, max_batches); gpu_ctx.check(rc)
    want, total = _host_loop(b, exb, pib, B, 2, 11, kind, max_batches or None)
    assert want.shape[0] == 2 and raw[L.INFO["epochs_run"]] == 2 and raw[L.INFO["batches_trained"]] == total == (max_batches or 6)
    assert _same(rows[:, :2], want[:, :2]) and np.isfinite(want[:, :2]).all() and np.all(want[:, 1] > 0) and _same(raw[:2], want[-1, :2])
    assert _same(a.get_params(), b.get_params()) and not _same(a.get_params(), c["p"])
    for x, y in zip(a.adam_state(), b.adam_state()):
        assert np.array_equal(x, y)
    for k in ("s", "a"):
        assert np.array_equal(exa[k], exb[k]) and np.array_equal(pia[k], pib[k])


def test_chain_refuses_wgp(gpu_ctx):
    c, ex_rows, pi_rows = _chain_case()
    D, ex, pi = _net(gpu_ctx, c), _buffer(gpu_ctx, c, ex_rows), _buffer(gpu_ctx, c, pi_rows)
    rc, raw, rows = _chain(D, ex, pi, 128, 1, 0, "WGP")
    msg = _err(gpu_ctx)
    assert rc == L.EUNSUP and "scratch per step" in msg, (rc, msg)
    assert _same(D.get_params(), c["p"]) and np.array_equal(ex["s"], ex_rows["s"])      # nothing ran, nothing was shuffled


# ---- 6. the round against its parts ------------------------------------------------------------------------------------------------------------------------------------
def test_round_is_its_parts_in_turn(gpu_ctx):
    """crux_nda_gail_round_gan with the hinge on a 520-row batch against the chain of D, the chain of Dnda, crux_nda_reward_cost and crux_nda_advantages, as
    tests/test_gpu_nda_gail.py checks the BCE round"""
    import test_gpu_nda_gail as NG
    c = NG.case(NG.SHAPES[0], B=128); c["batch"] = NG._rows(np.random.default_rng(8), c["od"], c["ad"], 520, c["disc"])
    a, b = NG.Setup(gpu_ctx, c), NG.Setup(gpu_ctx, c); B = 128; k = KIND["Hinge"]; lib = gpu_ctx.lib
    rD, rN, out3 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
    gpu_ctx.check(lib.crux_nda_gail_round_gan(a.D.h, a.N.h, a.demo.h, a.nda.h, a.batch.h, a.copyD.h, a.copyN.h, a.V.h, a.Vc.h, B, 2, 0, NG.SEED, 5, B, 3, 7, NG.SEED + 1, 9,
                                              0.3, 0.95, 0.99, k, _vp(rD), _vp(rN), _vp(out3)))
    wD, wN = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32)
    gpu_ctx.check(lib.crux_gail_d_batch_train_gan(b.D.h, b.demo.h, b.copyD.h, B, 2, 0, NG.SEED, 5, k, _vp(wD), None))
    gpu_ctx.check(lib.crux_gail_d_batch_train_gan(b.N.h, b.nda.h, b.copyN.h, B, 3, 7, NG.SEED + 1, 9, k, _vp(wN), None))
    w3 = crux.nda_reward_cost_(b.D, b.N, b.batch, 0.3); crux.nda_advantages_(b.batch, b.V, b.Vc, 0.95, 0.99)
    assert _same(rD, wD) and _same(rN, wN) and rN[L.INFO["batches_trained"]] == 7 and rD[L.INFO["batches_trained"]] == 8      # 393 demonstration rows: four pairs per epoch
    assert _same(out3, np.array(w3, np.float32))
    for x, y, p0 in ((a.D, b.D, c["pD"]), (a.N, b.N, c["pN"])):
        assert _same(x.get_params(), y.get_params()) and not _same(x.get_params(), p0)
        for u, w in zip(x.adam_state(), y.adam_state()):
            assert np.array_equal(u, w)
    for col in ["r", "cost"] + NG.ADV_COLS:
        assert _same(a.batch[col], b.batch[col]) and np.isfinite(a.batch[col]).all(), col
    # and the hinge is not the BCE round
    e = NG.Setup(gpu_ctx, c); eD = np.zeros(L.INFO_N, np.float32)
    gpu_ctx.check(lib.crux_gail_d_batch_train(e.D.h, e.demo.h, e.copyD.h, B, 2, 0, NG.SEED, 5, _vp(eD), None))
    assert not _same(e.D.get_params(), a.D.get_params())
    rc = lib.crux_nda_gail_round_gan(a.D.h, a.N.h, a.demo.h, a.nda.h, a.batch.h, a.copyD.h, a.copyN.h, a.V.h, a.Vc.h, B, 2, 0, NG.SEED, 5, B, 3, 7, NG.SEED + 1, 9,
                                     0.3, 0.95, 0.99, KIND["WGP"], _vp(rD), _vp(rN), _vp(out3))
    assert rc == L.EUNSUP and "scratch per step" in _err(gpu_ctx)


# ---- 7. NaN ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["BCE", "LS", "Hinge", "W", "WGP"])
def test_nan_in_the_policy_half_is_enan_and_updates_nothing(gpu_ctx, kind):
    c = GC.case("cont-relu"); pi_rows = {k: v.copy() for k, v in c["pi"].items()}; pi_rows["s"][1, 17] = np.nan
    ex, pi = _buffer(gpu_ctx, c, c["ex"]), _buffer(gpu_ctx, c, pi_rows)
    net = _net(gpu_ctx, c); m0 = [x.copy() for x in net.adam_state()]
    rc, info = _step(net, ex, 40, pi, 40, kind)
    assert rc == L.ENAN and "NaN detected" in _err(gpu_ctx), (rc, _err(gpu_ctx))
    assert _same(net.get_params(), c["p"])
    for x, y in zip(net.adam_state(), m0):
        assert np.array_equal(x, y)
    rc, info = _step(net, ex, 40, pi, 17, kind) if kind != "WGP" else _step(net, ex, 17, pi, 17, kind)      # the rows in front of the NaN: a clean step on the same handle
    gpu_ctx.check(rc); assert np.isfinite(info[:2]).all() and not _same(net.get_params(), c["p"])


# ---- 8. the solvers ----------------------------------------------------------------------------------------------------------------------------------------------------
def _pendulum(ctx, n=None):
    d = dict(np.load(os.path.join(GOLD, "pendulum_transitions.npz")))
    n = n or d["s"].shape[1]; S, A = crux.ContinuousSpace(3), crux.ContinuousSpace(1)
    obs3 = lambda x: np.vstack([np.cos(x[0]), np.sin(x[0]), x[1]]).astype(np.float32)
    rows = {"s": obs3(d["s"])[:, :n], "sp": obs3(d["sp"])[:, :n], "a": d["a"][:, :n], "r": d["r"][:, :n], "done": d["done"][:, :n], "episode_end": np.zeros((1, n), bool)}
    demo = crux.ExperienceBuffer(S, A, n, ctx=ctx); demo.push_(rows)
    nda = crux.ExperienceBuffer(S, A, n, ctx=ctx); nda.push_(dict(rows, a=-rows["a"]))
    return S, demo, nda


def _policy(ctx):
    acts = ["relu", "relu", "identity"]
    return acts, crux.ActorCritic(crux.GaussianPolicy(parity.chain([3, 64, 64, 1], acts), np.zeros(1, np.float32), seed=1, ctx=ctx), crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=2, ctx=ctx))


def _on_policy_gail(ctx, gan_loss, n_demo, B):
    S, demo, _ = _pendulum(ctx, n_demo); acts, pi = _policy(ctx)
    Dn = crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=3, ctx=ctx)
    sv = crux.OnPolicyGAIL(pi, S, gamma=0.99, D=Dn, demo=demo, N=2 * 256, dN=256, max_steps=64, normalize_demo=False, gan_loss=gan_loss,
                           a_opt={"epochs": 2, "batch_size": 128}, c_opt={"epochs": 2, "batch_size": 128}, d_opt={"epochs": 2, "batch_size": B}, target_kl=None)
    return sv, Dn


def test_onpolicy_gail_solves_with_the_hinge(gpu_ctx):
    sv, Dn = _on_policy_gail(gpu_ctx, crux.GAN_HingeLoss(), 512, 128); p0 = Dn.get_params().copy()
    assert isinstance(sv.d_opt.loss.gan_loss, crux.GAN_HingeLoss)
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    assert len(sv.history) == 2 and np.isfinite(sv.history[-1]["discriminator_loss"]) and sv.history[-1]["discriminator_batches_trained"] == 4
    assert not np.array_equal(Dn.get_params(), p0) and np.isfinite(Dn.get_params()).all() and sv.d_opt.gp_counter == 0


def test_nda_gail_solves_with_the_wasserstein_loss(gpu_ctx):
    ctx = gpu_ctx; S, demo, nda = _pendulum(ctx); acts, pi = _policy(ctx)
    Vc = crux.ContinuousNetwork(parity.chain([3, 64, 64, 1], acts), seed=5, ctx=ctx)
    Dn, Nn = crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=3, ctx=ctx), crux.ContinuousNetwork(parity.chain([4, 64, 64, 1], acts), seed=4, ctx=ctx)
    p0, n0 = Dn.get_params().copy(), Nn.get_params().copy(); opt = {"epochs": 2, "batch_size": 128}
    sv = crux.NDA_GAIL_JS(pi, S, demo, nda, Vc, 0.99, Dn, Nn, N=2 * 256, dN=256, max_steps=8, normalize_demo=False, a_opt=dict(opt), c_opt=dict(opt), cost_opt=dict(opt),
                          d_opt=dict(opt), d_opt_nda=dict(opt), target_kl=None, gan_loss=crux.GAN_WLoss())
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    h = sv.history[-1]
    assert len(sv.history) == 2 and np.isfinite(h["discriminator_loss"]) and np.isfinite(h["nda_discriminator_loss"]) and h["discriminator_batches_trained"] == 4
    assert not np.array_equal(Dn.get_params(), p0) and not np.array_equal(Nn.get_params(), n0) and np.isfinite(Dn.get_params()).all()
    assert sv.d_opt.shuffle_counter == 2 * 2 and sv.d_opt_nda.shuffle_counter == 2 * 2


def test_wgp_solves_through_the_host_loop(gpu_ctx):
    """256 demonstration rows and 256 rollout rows under batch_size 128: two equal pairs per epoch, four steps per iteration, each with its own draw counter"""
    sv, Dn = _on_policy_gail(gpu_ctx, crux.GAN_WLossGP(seed=7), 256, 128); p0 = Dn.get_params().copy()
    crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    assert len(sv.history) == 2 and np.isfinite(sv.history[-1]["discriminator_loss"]) and sv.history[-1]["discriminator_batches_trained"] == 4
    assert not np.array_equal(Dn.get_params(), p0) and np.isfinite(Dn.get_params()).all()
    assert sv.d_opt.gp_counter == 2 * 4 and sv.d_opt.shuffle_counter == 2 * 2


def test_wgp_with_unequal_pairs_raises_before_any_step(gpu_ctx):
    """200 demonstration rows against 256 rollout rows under batch_size 128: the second pair is 72 / 128"""
    sv, Dn = _on_policy_gail(gpu_ctx, crux.GAN_WLossGP(), 200, 128); p0 = Dn.get_params().copy()
    with pytest.raises(ValueError, match="72 and 128"):
        crux.solve(sv, crux.PendulumMDP(n_envs=4, seed=0))
    assert np.array_equal(Dn.get_params(), p0) and sv.d_opt.gp_counter == 0 and sv.d_opt.shuffle_counter == 0
