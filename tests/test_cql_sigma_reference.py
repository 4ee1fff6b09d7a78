"""The yardstick of CQL with a two-headed actor (tests/cql_sigma_reference.py) on its own: the streams of its policy samples, the conditions the GPU test's comparisons
rest on (the share of parameters the Adam comparison leaves out, float32's own error in the samples and their logprobs) and the clamp / beta-clamp cases. No GPU."""
import numpy as np
import pytest

import cql_reference as CR
import cql_sigma_reference as QR
import sigma_head_reference as SR

ALL = QR.CASES + [QR.CLAMP_CASE]


def _case(row):
    name, B, sc, N = row
    return QR.case(name, B, sc, 0 if row == QR.CLAMP_CASE else None), N


def test_sample_block_zero_takes_explorations_streams():
    """stream (k B + j) ad + d at k = 0 is j ad + d, the stream of exploration(pi, s) (SigmaExploreOp, SR.philox_normals): same normals, same action, same logprob"""
    for name, B, sc, N in QR.CASES:
        ad = SR.SHAPES[name][2]
        assert np.array_equal(CR.streams(N, B, ad)[:B * ad], np.arange(B * ad))
        c = QR.case(name, B, sc); e = QR.normals(c, N)
        assert len(e) == N and np.array_equal(e[0], SR.philox_normals(QR.CTR, B, ad))
        a, lp = QR.policy_samples(c, N); ra, rlp, _ = SR.explore(c, c["s"], SR.philox_normals(QR.CTR, B, ad))
        assert a.shape == (ad, N * B) and lp.shape == (N * B,) and np.array_equal(a[:, :B], ra) and np.array_equal(lp[:B], rlp)
        if N > 1:
            assert not np.array_equal(e[1], e[0])
        if sc > 0:
            assert np.abs(a).max() <= sc


@pytest.mark.parametrize("row", ALL, ids=lambda r: "%s-B%d-x%g-N%d" % r)
def test_skipped_share_of_every_critic_step(row):
    """at most a quarter of either critic may sit within 1e-3 of the gradient scale of zero (left out of the Adam comparison), at both temperatures"""
    c, N = _case(row)
    for la in QR.log_alphas(c):
        sh = QR.skipped_shares(c, N, la)
        print("skipped share %-16s B=%-4d ascale=%g N=%-2d log alpha %+.3f: q1 %.4f q2 %.4f" % (row + (la,) + tuple(sh)))
        assert max(sh) <= 0.25, (row, la, sh)


def test_skipped_share_of_the_weighted_and_beta_clamp_steps():
    name, B, sc, N = QR.WEIGHTED_CASE; c = QR.case(name, B, sc)
    sh = QR.skipped_shares(c, N, float(c["log_alpha"]), QR.weights(c)); print("weighted:", sh); assert max(sh) <= 0.25
    sh = QR.skipped_shares(c, N, QR.BETA_CLAMP); print("beta at its clamp:", sh); assert max(sh) <= 0.25


@pytest.mark.parametrize("row", ALL, ids=lambda r: "%s-B%d-x%g-N%d" % r)
def test_float32_error_and_tolerance(row):
    c, N = _case(row); ea, elp = QR.lp_error32(c, N); tol = QR.lp_tolerance(c, N); amax = np.abs(QR.policy_samples(c, N)[0]).max()
    print("float32 error %-16s B=%-4d ascale=%g N=%-2d: a %.3e (bound %.3e)  lp %.3e -> tolerance %.3e" % (row + (ea, 2e-5 * max(1.0, amax), elp, tol)))
    assert 0 < elp < 1e-2 and tol == 4 * elp
    assert ea <= 1.4e-6 and ea < 0.1 * 2e-5 * max(1.0, amax)      # the format's own share of the sampled actions' bound 2e-5 max(1, |a|max)


def test_clamp_case_covers_the_three_regions():
    c, N = _case(QR.CLAMP_CASE); l = SR.forward(c, c["s"])[1]
    assert (l < -5).any() and ((l > -5) & (l < 2)).any() and (l > 2).any() and np.abs(l + 5).min() > 1e-3 and np.abs(l - 2).min() > 1e-3
    a, lp = QR.policy_samples(c, N); mu = SR.forward(c, c["s"])[0]
    for k, e in enumerate(QR.normals(c, N)):      # sigma is the clamped one; the action stays inside the squash
        u = np.arctanh(a[:, k * c["B"]:(k + 1) * c["B"]] / c["ascale"])
        ok = np.abs(a[:, k * c["B"]:(k + 1) * c["B"]]) < c["ascale"] * (1 - 1e-9)
        np.testing.assert_allclose((u - mu)[ok], (e * np.exp(np.clip(l, -5, 2)))[ok], rtol=1e-6, atol=1e-6)
    assert np.isfinite(lp).all()


def test_alpha_gradient_inside_and_beyond_the_clamp():
    name, B, sc, N = QR.CASES[2]; c = QR.case(name, B, sc); a, lp = QR.samples(c, N)
    lse, qd, beta, _ = QR.conservative(c, a, lp, 0.0)
    info, g, x1 = QR.alpha_step(c, a, lp, 0.0)
    assert g == pytest.approx(-beta.item() * (5 * (lse - qd).item() - QR.THRESH), rel=1e-9) and abs(abs(x1) - QR.LR) <= 1e-9 and info["alpha"] == 1.0
    info, g, x1 = QR.alpha_step(c, a, lp, QR.BETA_CLAMP)
    assert g == 0.0 and x1 == QR.BETA_CLAMP and QR.conservative(c, a, lp, QR.BETA_CLAMP)[2].item() == 1e6
