"""conv_gauss_reference's hand gradients of the Gaussian head (d(loss)/d(mu), d(loss)/d(logSigma)) against central differences of its own float64 loss."""
import numpy as np
import pytest

import conv_gauss_reference as GR


@pytest.mark.parametrize("kind", ["ppo", "a2c", "reinforce"])
def test_head_gradients_match_central_differences(kind):
    rng = np.random.default_rng(5); ad, B, h = 3, 7, 1e-6
    mu, a, ls = rng.normal(0, 1, (ad, B)), rng.normal(0, 1, (ad, B)), rng.uniform(-0.7, 0.3, ad)
    adv, ret = rng.normal(0, 1, B), rng.normal(0, 1, B)
    logp = GR.gaussian(mu, a, ls, np.dtype(np.float64))[0]
    oldlp = logp - np.where(np.arange(B) % 2 == 0, 0.4, 0.05) * rng.choice([-1, 1], B)      # both sides of the clip and inside it, none near an edge
    f = lambda m, l: GR.actor_seed(kind, m, a, l, adv, ret, oldlp, 0.2, 0.7, 0.1)      # noqa: E731
    ref = f(mu, ls)
    if kind == "ppo":
        out = (ref["ratio"] > 1.2) | (ref["ratio"] < 0.8); assert out.any() and (~out).any()
    for name, x, g in (("dz", mu, ref["dz"]), ("g_ls", ls, ref["g_ls"])):
        num = np.zeros_like(x)
        for i in np.ndindex(x.shape):
            xp, xm = x.copy(), x.copy(); xp[i] += h; xm[i] -= h
            num[i] = (f(*((xp, ls) if name == "dz" else (mu, xp)))["loss"] - f(*((xm, ls) if name == "dz" else (mu, xm)))["loss"]) / (2 * h)
        assert np.abs(num - g).max() <= 1e-8 * max(1.0, np.abs(g).max()), name
