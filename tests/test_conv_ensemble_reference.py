"""conv_ensemble_reference.step_reference against torch autograd in float64: both kinds at the GPU test's step shape (M = 3, B = 9, weights for the Gaussian kind)."""
import numpy as np
import pytest
import torch

import conv_ensemble_reference as CER
import conv_reference as CR
import dense_reference as R
import ensemble_reference as ER


def _torch_member(sp, pt_, dims, acts, ph_, x):
    """trunk + head in torch float64, Flux's semantics (flipped kernel, WHCN column-major features): (output [n x B], the two leaves)"""
    pt, ph = torch.tensor(pt_, dtype=torch.float64, requires_grad=True), torch.tensor(ph_, dtype=torch.float64, requires_grad=True)
    B = x.shape[1]; h = torch.tensor(x.astype(np.float64)).T.reshape(B, sp["C"], sp["H"], sp["W"])
    for (wo, bo), ly in zip(CR.layer_offsets(sp), sp["layers"]):
        w = pt[wo:bo].reshape(ly["cout"], ly["cin"], ly["k"][1], ly["k"][0]).flip(2, 3)
        h = torch.tanh(torch.nn.functional.conv2d(h, w, pt[bo:bo + ly["cout"]], stride=ly["stride"][::-1], padding=ly["pad"][::-1]))
    h = h.reshape(B, -1).T
    for l, ((wo, bo), act) in enumerate(zip(R.layer_offsets(dims), acts)):
        h = ph[wo:bo].reshape(dims[l], dims[l + 1]).T @ h + ph[bo:bo + dims[l + 1]][:, None]
        h = torch.tanh(h) if act == "tanh" else h
    return h, pt, ph


@pytest.mark.parametrize("kind", [ER.GAUSS, ER.CLASS])
def test_step_reference_matches_autograd(kind):
    M, B = 3, 9
    pts, phs, x, y, w = CER.inputs(kind, M, B, seed=4); dims = CER.head_dims(4 if kind == ER.GAUSS else 3)
    ref = CER.step_reference(kind, CER.SPEC, dims, CER.ACTS, pts, phs, x, y, w)
    nets = [_torch_member(CER.SPEC, pt, dims, CER.ACTS, ph, x) for pt, ph in zip(pts, phs)]; yt = torch.tensor(y.astype(np.float64)); losses = []
    for o, _, _ in nets:
        if kind == ER.GAUSS:
            mu, var = o[:2], torch.nn.functional.softplus(o[2:]) + 1e-3
            losses.append(-(torch.tensor(w.astype(np.float64)) * (-torch.log(var) / 2 - (yt - mu) ** 2 / (2 * var))).mean())
        else:
            losses.append((-(yt * torch.log(torch.softmax(o, 0) + ER.EPS32)).sum(0)).mean())
    loss = torch.stack(losses).mean(); loss.backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
    for m, (_, pt, ph) in enumerate(nets):
        assert abs(losses[m].item() - ref["losses"][m]) <= 1e-12 * max(1.0, abs(ref["losses"][m]))
        for g, t in ((ref["g_trunk"][m], pt), (ref["g_head"][m], ph)):
            assert np.abs(t.grad.numpy() - g).max() <= 1e-10 * np.abs(g).max(), (kind, m)
    assert abs(np.sqrt(sum(float((t.grad ** 2).sum()) for _, pt, ph in nets for t in (pt, ph))) - ref["grad_norm"]) <= 1e-10 * ref["grad_norm"]
