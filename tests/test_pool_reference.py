"""Pooling layers on the host (no GPU): the mirror's extents against the reference helper and torch on the grid of test_gpu_conv_pool.py, split_chain's refusals by name,
and the tie / NaN / padding rules of pool_reference.pool2d (the rules csrc/conv_pool.hip implements) pinned on a hand example of one 3 x 3 image."""
import numpy as np
import pytest
import torch

import conv_reference as CR
import pool_reference as PR
import crux_jl_amd as crux


def host_spec(sp):
    pools = [None if q is None else (crux.MaxPool if q["kind"] == "max" else crux.MeanPool)(q["k"], stride=q["stride"], pad=q["pad"]) for q in sp["pools"]]
    return crux.ConvSpec(sp["W"], sp["H"], sp["C"], sp["scale"], [crux.Conv(ly["k"], ly["cin"], ly["cout"], ly["act"], ly["stride"], ly["pad"]) for ly in sp["layers"]], pools)


@pytest.mark.parametrize("where", [0, 1])
@pytest.mark.parametrize("window,pooled", [("2x2s2", (3, 3)), ("3x3s2", (3, 2)), ("3x2s2x1p1x0", (4, 5)), ("2x2s3", (2, 2))])
def test_mirror_extents_follow_the_pools(window, pooled, where):
    sp = PR.grid_spec(window, "max", where, "relu"); hs = host_spec(sp)
    assert hs.extents == PR.extents(sp) and hs.extents[where + 1][:2] == pooled and hs.extents[2 - where][:2] == ((7, 6) if where else pooled)
    assert hs.out_features == PR.n_features(sp) and hs.n_params == CR.n_params(sp)      # the parameter layout does not change
    r = PR.reference(np.zeros(CR.n_params(sp), np.float32), sp, np.zeros((84, 2), np.float32), np.zeros((PR.n_features(sp), 2), np.float32))
    assert r["y"].shape == (hs.out_features, 2) and tuple(r["P"][where].shape[2:]) == pooled[::-1]


def test_defaults_and_a_chain_with_pools():
    q = crux.MaxPool((2, 3))
    assert q.stride == (2, 3) and q.pad == (0, 0) and crux.MeanPool(2, stride=1, pad=1).k == (2, 2)
    ch = crux.Chain(crux.Conv((3, 3), 1, 8, "relu", pad=1), crux.MaxPool((2, 2)), crux.Conv((3, 3), 8, 16, "relu", pad=1), crux.MeanPool((2, 2)), crux.flatten,
                    crux.Dense(2 * 2 * 16, 10), input=(8, 8, 1))
    assert ch.conv.extents == [(8, 8, 1), (4, 4, 8), (2, 2, 16)] and [type(q).__name__ for q in ch.conv.pools] == ["MaxPool", "MeanPool"]


@pytest.mark.parametrize("layers,err,word", [
    (lambda: [crux.MaxPool(2), crux.Conv(3, 1, 4), crux.flatten, crux.Dense(4, 2)], NotImplementedError, "before the first Conv"),
    (lambda: [crux.Scale(0.5), crux.MeanPool(2), crux.Conv(3, 1, 4), crux.flatten, crux.Dense(4, 2)], NotImplementedError, "before the first Conv"),
    (lambda: [crux.Conv(3, 1, 4), crux.MaxPool(2), crux.MeanPool(2), crux.flatten, crux.Dense(4, 2)], NotImplementedError, "two pooling layers in a row"),
    (lambda: [crux.Conv(3, 1, 4), crux.flatten, crux.MaxPool(2), crux.Dense(4, 2)], NotImplementedError, "after flatten"),
    (lambda: [crux.Conv(3, 1, 4), crux.MaxPool(7), crux.flatten, crux.Dense(4, 2)], ValueError, "does not fit"),
    (lambda: [crux.Conv(3, 1, 4), crux.MaxPool(5), crux.Conv(3, 4, 4), crux.flatten, crux.Dense(4, 2)], ValueError, "does not fit"),      # the next Conv on a 1 x 1 input
    (lambda: [crux.Conv(3, 1, 4), crux.MaxPool(2, pad=2)], ValueError, "pad < window"),
    (lambda: [crux.Conv(3, 1, 4), crux.MaxPool((17, 16))], NotImplementedError, "256"),
], ids=["first", "after_scale", "two", "after_flatten", "too_large", "next_conv", "pad", "window256"])
def test_refusals_name_themselves(layers, err, word):
    with pytest.raises(err) as e:
        crux.Chain(*layers(), input=(8, 8, 1))
    assert word in str(e.value)


def test_the_dense_only_refusal_no_longer_names_pooling():
    class BatchNorm:
        conv_kind = "batchnorm"
    with pytest.raises(ValueError) as e:
        crux.Chain(crux.Conv(3, 1, 4), crux.flatten, BatchNorm(), crux.Dense(4, 2), input=(8, 8, 1))
    assert "batch norm" in str(e.value) and "pooling" not in str(e.value)


def test_tie_nan_and_padding_rules_on_one_3x3_image():
    """image[h][w] (torch's order: W is the last axis):  1 1 2 / 1 0 2 / -3 -inf nan.  Window (2, 2), stride 1, pad 1: 4 x 4 windows."""
    inf, nan = np.inf, np.nan
    img = torch.tensor([[1.0, 1.0, 2.0], [1.0, 0.0, 2.0], [-3.0, -inf, nan]], dtype=torch.float64).reshape(1, 1, 3, 3).requires_grad_(True)
    q = PR.pool("max", 2, 1, 1)
    p = PR.pool2d(img, q); p.backward(torch.ones_like(p))
    want = np.array([[1, 1, 2, 2], [1, 1, 2, 2], [1, 1, nan, nan], [-3, -3, nan, nan]])
    assert np.array_equal(p.detach().numpy()[0, 0], want, equal_nan=True)      # padding taps never win (the corner windows hold one real tap, -3 beats the padding beside
    # it); a NaN in a window gives NaN. Ties go to the FIRST element in window order, W fastest: image (0, 0) collects windows (0, 0), (0, 1), (1, 0), (1, 1), whose ones
    # tie; the two 2s tie in windows (1, 2), (1, 3): the upper one, (0, 2), wins and collects four windows; the 1 at (1, 0) wins windows (2, 0), (2, 1); -3 wins (3, 0), (3, 1)
    # (-inf loses to it); the NaN takes all four windows that hold it
    g = img.grad.numpy()[0, 0]
    assert np.array_equal(g, [[4, 0, 4], [2, 0, 0], [2, 0, 4]])
    m = PR.pool2d(torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]], dtype=torch.float64).reshape(1, 1, 3, 3), PR.pool("mean", 2, 1, 1))
    assert np.array_equal(m.numpy()[0, 0, 0], [0.25, 0.75, 1.25, 0.75]) and m[0, 0, 1, 1] == 3.0      # padding taps count as 0, the divisor is k1 k2 always
