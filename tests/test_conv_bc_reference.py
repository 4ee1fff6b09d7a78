"""conv_bc_reference's gradients against torch autograd in float64, at one shape, for the three behaviour-cloning heads."""
import numpy as np
import pytest
import torch

import conv_bc_reference as BR
import conv_gauss_reference as GR
import conv_pg_reference as PG
from test_conv_pg_reference import _torch_net


@pytest.mark.parametrize("form", BR.FORMS)
def test_bc_gradients_match_autograd(form):
    sp, B, le = PG.PLAIN, 5, 0.05
    net, ls, s, a = BR.inputs(form, sp, B, seed=11)
    ref = BR.bc_reference(form, sp, net, ls, s, a, le)
    z, pt, ph = _torch_net(sp, net[0], PG.head_dims(sp, a.shape[0]), net[1], s)
    at, ce = torch.tensor(a.astype(np.float64)), np.float64(np.float32(le)); tl = None
    if form == "categorical":
        p = torch.softmax(z, 0); logp = torch.log((p * at).sum(0)); H = -(p * torch.log(p + PG.EPS)).sum(0).mean()
    elif form == "gaussian":
        tl = torch.tensor(ls.astype(np.float64), requires_grad=True)
        logp = (-(at - z) ** 2 / (2 * torch.exp(tl)[:, None] ** 2) - GR.HALF_LOG_2PI - tl[:, None]).sum(0); H = GR.ENT0 + tl.sum()
    loss = ((z - at) ** 2).mean() if form == "mse" else -logp.mean() - ce * H
    loss.backward()
    want = [(loss.item(), ref["loss"])] + ([] if form == "mse" else [(H.item(), ref["entropy"]), (-logp.mean().item(), ref["logpdf"])])
    for got, w in want:
        assert abs(got - w) <= 1e-12 * max(1.0, abs(w))
    for name, g, t in (("trunk", ref["g_trunk"], pt), ("head", ref["g_head"], ph)) + ((("logSigma", ref["g_ls"], tl),) if tl is not None else ()):
        assert np.abs(t.grad.numpy() - g).max() <= 1e-10 * np.abs(g).max(), (form, name)
    assert form != "mse" or (ref["g_ls"].size == 3 and not ref["g_ls"].any())      # action(pi, s) = mu: no gradient reaches logSigma
