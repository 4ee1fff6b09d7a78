"""CPU: pins tests/gan_reference.py, the float64 yardstick of the five discriminator losses Lᴰ (src/extras/gans.jl), and asserts on it the input conditions that
tests/test_gpu_gan_losses.py relies on for every fixed seed of tests/gan_cases.py. The closed-form seeds of the table in include/cruxhip.h appear HERE, as the
other side of the comparison with autograd, and not in the yardstick."""
import numpy as np
import pytest
import torch

import gan_cases as GC
import gan_reference as GR
import iq_reference as IQ
import nda_gail_reference as NR


def _z(c, x):
    ad = c["ad"]
    return NR.d_out(c["p"], c["dims"], c["acts"], x[:ad], x[ad:])


def test_bce_is_the_nda_gail_yardsticks_loss():
    c = GC.case("disc-relu"); ex, pi = c["ex"], c["pi"]
    for ne, npi in GC.SIZES:
        xe, xp = GC.x_of(ex, ne), GC.x_of(pi, npi)
        loss, g = GR.d_step("BCE", c["p"], c["dims"], c["acts"], xe, xp)
        want, gw = NR.d_step(c["p"], c["dims"], c["acts"], ex["a"][:, :ne], ex["s"][:, :ne], pi["a"][:, :npi], pi["s"][:, :npi])
        assert loss == want and np.array_equal(g, gw)


@pytest.mark.parametrize("n_ex,n_pi", [(1, 1), (3, 7), (40, 25)])
def test_autograd_seeds_equal_the_closed_forms(n_ex, n_pi):
    rng = np.random.default_rng(n_ex); z = rng.normal(0, 2, n_ex + n_pi); e = np.arange(n_ex + n_pi) < n_ex
    sg = 1.0 / (1.0 + np.exp(-z))
    closed = {"LS": np.where(e, 2 * (sg - 1) * sg * (1 - sg) / n_ex, 2 * sg * sg * (1 - sg) / n_pi),
              "Hinge": np.where(e, -1.0 * (z < 1) / n_ex, 1.0 * (z > -1) / n_pi),
              "W": np.where(e, -1.0 / n_ex, 1.0 / n_pi)}
    for kind, want in closed.items():
        assert np.abs(GR.dz(kind, z, n_ex) - want).max() < 1e-15, kind


def test_hinge_seed_is_zero_exactly_on_the_kink():
    """relu'(0) = 0: the expert column at z = 1 and the policy column at z = -1 get no gradient"""
    assert np.array_equal(GR.dz("Hinge", np.array([1.0, 0.0, -1.0, 0.0]), 2), np.array([0.0, -0.5, 0.0, 0.5]))


def test_wgp_is_w_plus_lambda_times_the_penalty():
    for name in GC.CASES:
        c = GC.case(name); n = 37; xe, xp = GC.x_of(c["ex"], n), GC.x_of(c["pi"], n)
        layers = GR.mlp_params(c["p"], c["dims"])
        with torch.enable_grad():
            wgp, w = GR.d_loss("WGP", layers, c["acts"], xe, xp, GC.LAM, GC.GP_SEED, GC.GP_COUNTER).item(), GR.d_loss("W", layers, c["acts"], xe, xp).item()
            P = IQ.gradient_penalty(layers, c["acts"], IQ.xhat(xe, xp, IQ.eps(GC.GP_SEED, GC.GP_COUNTER, n))).item()
            other = GR.d_loss("WGP", layers, c["acts"], xe, xp, GC.LAM, GC.GP_SEED, GC.GP_COUNTER + 1).item()
        assert abs((wgp - w) - 10.0 * P) <= 1e-12 * max(1.0, abs(wgp)) and P > 0
        assert abs(other - wgp) > 1e-3 * abs(wgp)      # the draw matters: a step that used another counter's eps does not pass a 1e-4 comparison
    with pytest.raises(ValueError, match="DimensionMismatch"):
        GR.wgp_xhat(xe, xp[:, :5], 0, 0)


def test_the_references_known_answer():
    """test/extras_tests.jl:7-9: Dense(2, 1, init = ones, bias = false) on ones(2, 100): |dD/dx| = sqrt(2) in every column, penalty (sqrt(2) - 1)^2. Through the
    WGP path with both halves equal to x (xhat = x whatever eps is): the loss is W (= 0 here) + 10 times it."""
    dims, acts, p = (2, 1), ("identity",), np.array([1.0, 1.0, 0.0])
    x = np.ones((2, 100), np.float32)
    layers = GR.mlp_params(p, dims)
    assert abs(IQ.gradient_penalty(layers, acts, x).item() - (np.sqrt(2) - 1) ** 2) < 1e-15
    assert abs(GR.d_loss("WGP", layers, acts, x, x, 10.0, 5, 9).item() - 10 * (np.sqrt(2) - 1) ** 2) < 1e-14


@pytest.mark.parametrize("name", list(GC.CASES))
def test_input_conditions_of_the_gpu_tests(name):
    c = GC.case(name); xe, xp = GC.x_of(c["ex"]), GC.x_of(c["pi"]); ze, zp = _z(c, xe), _z(c, xp)
    # every step reads a prefix of the pools: no column of either pool within 1e-3 of its kink
    assert np.abs(ze - 1).min() >= 1e-3 and np.abs(zp + 1).min() >= 1e-3
    assert min(ze.min(), zp.min()) < -3 and max(ze.max(), zp.max()) > 3
    # both sides of each kink hold at least a quarter of the half, in every half wide enough to have a quarter (the halves of 1 and 3 columns cannot)
    for n in (255, 256, 257, 300):
        for frac in ((ze[:n] > 1).mean(), (zp[:n] > -1).mean()):
            assert 0.25 <= frac <= 0.75, (n, frac)
    worst = 0.0
    for kind in GC.HEAD_KINDS:
        for ne, npi in GC.SIZES:
            worst = max(worst, GC.skipped(GR.d_step(kind, c["p"], c["dims"], c["acts"], xe[:, :ne], xp[:, :npi])[1])[1])
    for n in GC.WGP_SIZES:
        worst = max(worst, GC.skipped(GR.d_step("WGP", c["p"], c["dims"], c["acts"], xe[:, :n], xp[:, :n], GC.LAM, GC.GP_SEED, GC.GP_COUNTER)[1])[1])
    print("%s: largest share under the exclusion rule %.3f" % (name, worst))
    assert worst <= 0.05
    # The GPU tests compare the entries whose float64 gradient is exactly zero. That is well-posed for a dead unit (zero in any arithmetic) and not for a cancellation
    # between columns (gan_reference.abs_seed_grad), so the inputs hold none. Exempt: the output bias under W and WGP, where the device's integer seeds cancel exactly
    # (GanHeadOp, k_advil_d_head), and the steps with one column per half, where the sum is w - w.
    for kind in GC.HEAD_KINDS + ["WGP"]:
        for ne, npi in (GC.SIZES if kind != "WGP" else [(n, n) for n in GC.WGP_SIZES]):
            if (ne, npi) == (1, 1):
                continue
            g = GR.d_step(kind, c["p"], c["dims"], c["acts"], xe[:, :ne], xp[:, :npi], GC.LAM, GC.GP_SEED, GC.GP_COUNTER)[1]
            m = (g == 0) & (GR.abs_seed_grad(kind, c["p"], c["dims"], c["acts"], xe[:, :ne], xp[:, :npi]) != 0)
            if kind in ("W", "WGP"):
                m[-1] = False
            assert not m.any(), (kind, ne, npi, np.flatnonzero(m))


def test_input_conditions_of_the_densesn_case():
    """the DenseSN steps of the GPU tests (tests/test_gpu_sn.py's 3-12-1 and 3-64-64-2-1 cases, rows [1, 34) and [2, 23)): no output on a hinge kink"""
    import sn_reference as SR
    import test_gpu_sn as TS
    for name, n_iter in TS.GAIL_STEPS:
        c = TS.case(name, n_iter); od = c["dims"][0] - 1
        ex, pi = TS._rows(c["rng"], od, 1, 40), TS._rows(c["rng"], od, 1, 30)
        x = np.concatenate([np.concatenate([ex["a"][:, 1:34], ex["s"][:, 1:34]], 0), np.concatenate([pi["a"][:, 2:23], pi["s"][:, 2:23]], 0)], 1)
        z = SR.forward(c["p"], c["dims"], c["acts"], c["sn"], c["us"], x)[0].reshape(-1)
        assert np.abs(z[:33] - 1).min() >= 1e-3 and np.abs(z[33:] + 1).min() >= 1e-3, (name, n_iter)


def test_host_api():
    import crux_jl_amd as crux
    assert list(crux.GANLosses) == ["BCE", "LS", "Hinge", "W", "WGP"]
    assert [crux.GANLosses[k].kind for k in crux.GANLosses] == [GR.KINDS[k] for k in crux.GANLosses] == [0, 1, 2, 3, 4]
    assert isinstance(crux.GANLosses["WGP"], crux.GAN_WLossGP) and crux.GANLosses["WGP"].λ == 10.0 and crux.GANLosses["WGP"].noise_range == 1.0
    w = crux.gail_d_loss(crux.GAN_WLoss())
    assert w.name == "gail_d" and isinstance(w.gan_loss, crux.GAN_WLoss) and w.gan_loss.kind == 3 and w is not crux.gail_d_loss
    p = crux.TrainingParams(loss=crux.gail_d_loss)
    assert p.loss is crux.gail_d_loss and isinstance(p.loss.gan_loss, crux.GAN_BCELoss) and p.loss.gan_loss.kind == 0 and p.gp_counter == 0
    with pytest.raises(TypeError):
        crux.gail_d_loss("Hinge")
    from crux_jl_amd import imitation as IM
    assert IM._gail_pairs(300, 520, 128) == [(0, 128, 128), (128, 128, 128), (256, 44, 128)]
