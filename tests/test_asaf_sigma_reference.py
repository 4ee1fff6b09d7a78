"""The yardstick of ASAF with a two-headed policy (tests/asaf_sigma_reference.py) on its own: known answers of the loss, the entropy's two forms, and the conditions the GPU
test's comparisons rest on (the share of parameters the Adam comparison leaves out, float32's own error in logpdf). No GPU."""
import numpy as np
import pytest
import torch

import asaf_sigma_reference as AS
import cql_reference as CR
import sigma_head_reference as SR

ALL = [(r, None) for r in AS.CASES] + [(AS.CLAMP_CASE, 0)]
IDS = ["%s-n%d-x%g-NE%d%s" % (r + ("" if k is None else "-clamp",)) for r, k in ALL]


@pytest.mark.parametrize("row,clamp", ALL, ids=IDS)
def test_skipped_share_of_every_step(row, clamp):
    """at most a quarter of the handle may sit within 1e-3 of the gradient scale of zero (left out of the Adam comparison)"""
    c = AS.case(*row, clamp); info, g, p = AS.step(c); sh = SR.skipped_share(g)
    print("skipped share %-16s n=%-4d ascale=%g N_E=%-5d: %.4f   %s" % (row + (sh, info)))
    assert sh <= 0.25, (row, sh)
    assert all(np.isfinite(v) for v in info.values()) and np.isfinite(g).all()
    keep = np.abs(g) > 1e-3 * np.abs(g).max()
    np.testing.assert_allclose((np.asarray(c["p"], np.float64) - p)[keep], AS.LR * np.sign(g[keep]), rtol=1e-3)      # Adam's first step: lr sign(g)


@pytest.mark.parametrize("row,clamp", ALL, ids=IDS)
def test_float32_error_and_tolerance(row, clamp):
    c = AS.case(*row, clamp); e = AS.logpdf32_error(c); tol = AS.logpdf_tolerance(c)
    print("float32 error %-16s n=%-4d ascale=%g N_E=%-5d: logpdf %.3e -> tolerance %.3e" % (row + (e, tol)))
    assert 0 < e < 1e-2 and tol == 4 * e
    # the torch logpdf of this yardstick is SR.logpdf (the float32 constant 0.9189385f0 against the float64 one: 1.6e-8 per action dimension)
    for s, a in ((c["s"], c["a"]), (c["sE"], c["aE"])):
        assert np.abs(AS._logpdf_np(c, c["p"], s, a) - SR.logpdf(c, s, a)).max() <= 1e-7 * c["ad"] + 1e-9


def test_policy_equal_to_its_frozen_copy_gives_two_ln2():
    for row in (AS.CASES[0], AS.CASES[3]):
        c = dict(AS.case(*row)); c["gG"] = AS._logpdf_np(c, c["p"], c["s"], c["a"]); c["gE"] = AS._logpdf_np(c, c["p"], c["sE"], c["aE"])      # (float64: exact zeros)
        with torch.no_grad():
            L, parts = AS.loss(c, CR.mlp_params(c["p"], c["dims"]))
        assert abs(float(parts["expert"]) - np.log(2.0)) < 1e-12 and abs(float(parts["policy"]) - np.log(2.0)) < 1e-12
        assert abs(float(L) - (2 * np.log(2.0) - 0.1 * float(parts["entropy"]))) < 1e-12


def test_entropy_forms_and_their_share_of_the_gradient():
    """GaussianPolicy: entropy sums logSigma(s) over the whole minibatch (one scalar, its mean is itself): d/dl = 1 per rollout column; squashed: per column, d/dl = 1 / n.
    Demonstration columns carry no entropy term. Seen through the last layer's logSigma bias rows, whose gradient is the row sum of dl."""
    for row in (AS.CASES[4], AS.CASES[3]):      # ascale 0 and 2 of 5-100-100-2x3
        c = AS.case(*row); n, ad, sc = c["B"], c["ad"], c["ascale"]
        l = SR.forward(c, c["s"])[1]; ent = SR.entropy(c, c["s"])
        info, g, _ = AS.step(c)
        assert abs(info["entropy"] - float(np.mean(ent))) <= 1e-6 and abs(info["entropy"] - (AS.AR.ENTROPY_CONST + (l.sum() / n if sc > 0 else l.sum()))) <= 1e-9
        # the same loss without the entropy term: the logSigma bias gradient differs by -0.1 ce n = -0.1 n (Gaussian) or -0.1 (squashed)
        layers = CR.mlp_params(c["p"], c["dims"]); L, parts = AS.loss(c, layers); (L + 0.1 * parts["entropy"]).backward(); g0 = CR.flat_grad(layers)
        np.testing.assert_allclose((g - g0)[-ad:], -0.1 * (1.0 if sc > 0 else n), rtol=1e-9)
        assert np.abs((g - g0)[-2 * ad:-ad]).max() <= 1e-12      # mu's bias rows: no entropy share


def test_clamp_case_covers_the_three_regions_and_masks_the_gradient():
    c = AS.case(*AS.CLAMP_CASE, 0); ad = c["ad"]
    for s in (c["s"], c["sE"]):
        l = SR.forward(c, s)[1]
        assert (l < -5).any() and ((l > -5) & (l < 2)).any() and (l > 2).any() and np.abs(l + 5).min() > 1e-3 and np.abs(l - 2).min() > 1e-3
    assert np.isfinite(AS.step(c)[1]).all()
