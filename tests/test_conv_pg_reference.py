"""conv_pg_reference's hand-written gradients against torch autograd in float64, at one shape, for the three actor losses and the critic's mse."""
import numpy as np
import pytest
import torch

import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R


def _torch_net(sp, p_trunk, dims, p_head, s):
    """trunk + head in torch float64 with Flux's semantics (true convolution: flipped kernel; WHCN column-major features); returns (output [n x B], the two leaf tensors)"""
    pt, ph = torch.tensor(p_trunk, dtype=torch.float64, requires_grad=True), torch.tensor(p_head, dtype=torch.float64, requires_grad=True)
    B = s.shape[1]
    h = torch.tensor(s.astype(np.float64) * np.float64(np.float32(sp["scale"]))).T.reshape(B, sp["C"], sp["H"], sp["W"])      # index w + W (h + H c) per sample -> NCHW
    for (wo, bo), ly in zip(CR.layer_offsets(sp), sp["layers"]):
        w = pt[wo:bo].reshape(ly["cout"], ly["cin"], ly["k"][1], ly["k"][0]).flip(2, 3)      # (k1, k2, cin, cout) column-major == (cout, cin, k2, k1) row-major
        h = torch.relu(torch.nn.functional.conv2d(h, w, pt[bo:bo + ly["cout"]], stride=ly["stride"][::-1], padding=ly["pad"][::-1]))
    x = h.reshape(B, -1).T
    for l, ((wo, bo), act) in enumerate(zip(R.layer_offsets(dims), PG.ACTS)):
        x = ph[wo:bo].reshape(dims[l], dims[l + 1]).T @ x + ph[bo:bo + dims[l + 1]][:, None]
        x = torch.relu(x) if act == "relu" else x
    return x, pt, ph


@pytest.mark.parametrize("kind", ["ppo", "a2c", "reinforce"])
def test_hand_gradients_match_autograd(kind):
    sp, B, eps, lp, le = PG.PLAIN, 33, 0.2, 0.7, 0.1
    actor, critic, s, a, adv, ret, oldlp = PG.inputs(sp, B, seed=5)
    ref = PG.pg_reference(kind, sp, actor, critic, s, a, adv, ret, oldlp, eps, lp, le)
    z, pt, ph = _torch_net(sp, actor[0], PG.head_dims(sp, PG.N_ACTIONS), actor[1], s)
    p = torch.softmax(z, 0); logp = torch.log((p * torch.tensor(a.astype(np.float64))).sum(0)); H = -(p * torch.log(p + PG.EPS)).sum(0)
    A, Rt, old = (torch.tensor(t.astype(np.float64)) for t in (adv, ret, oldlp)); e, cp, ce = (np.float64(np.float32(v)) for v in (eps, lp, le))
    r = torch.exp(logp - old)
    loss = {"ppo": -cp * torch.minimum(r * A, torch.clamp(r, 1 - e, 1 + e) * A).mean() - ce * H.mean(), "a2c": -cp * (logp * A).mean() - ce * H.mean(), "reinforce": -(logp * Rt).mean()}[kind]
    v, ct, chd = _torch_net(sp, critic[0], PG.head_dims(sp, 1), critic[1], s)
    closs = ((v - Rt[None, :]) ** 2).mean(); (loss + closs).backward()
    for got, want in ((loss.item(), ref["loss"]), (H.mean().item(), ref["entropy"]), ((old - logp).mean().item(), ref["kl"]), (closs.item(), ref["critic_loss"])):
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    for name, g, t in (("trunk", ref["g_trunk"], pt), ("head", ref["g_head"], ph), ("critic trunk", ref["gc_trunk"], ct), ("critic head", ref["gc_head"], chd)):
        assert np.abs(t.grad.numpy() - g).max() <= 1e-10 * np.abs(g).max(), (kind, name)
    out = (r.detach().numpy() > 1 + e) | (r.detach().numpy() < 1 - e)
    assert out.any() and (~out).any() and (kind != "ppo" or ref["clip_fraction"] == out.mean())
