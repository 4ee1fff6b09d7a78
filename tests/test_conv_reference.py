"""The yardstick of the convolutional trunk (tests/conv_reference.py) pinned on the CPU: Flux's flip on the hand example, torch.nn.functional.conv2d in float64 with the kernel
flipped on both axes and W / H transposed, torch autograd for dW, db, dX; the emulated kernel order against the float32 restatement over the whole GPU grid (the margin M); the
bound of the post-Adam parameter comparison against a float32 restatement of the update."""
import numpy as np
import pytest
import torch

import conv_reference as CR


def test_hand_example_true_convolution():
    """Conv((2,1), 1=>1) with weight [a, b] on [x1, x2, x3] gives [a x2 + b x1, a x3 + b x2] (NNlib flips the kernel; CrossCor would give a x1 + b x2)"""
    sp = CR.spec(3, 1, 1, [CR.layer((2, 1), 1, 1)])
    a, b, x = 2.0, -3.0, np.array([[5.0], [7.0], [11.0]])
    r = CR.trunk_reference(np.array([a, b, 0.5]), sp, x, np.ones((2, 1)))
    assert np.array_equal(r["y"][:, 0], [a * 7 + b * 5 + 0.5, a * 11 + b * 7 + 0.5])
    assert np.array_equal(r["dW"][0].reshape(-1), [7 + 11, 5 + 7]) and np.array_equal(r["db"][0], [2.0])
    assert np.array_equal(r["dx"][:, 0], [b, a + b, a])


def _torch_trunk(p, sp, x, dy):
    """the same trunk through torch (NCHW, cross-correlation): weights flipped on both axes, W and H transposed"""
    B = x.shape[1]; Ws, bs = CR.weights(p, sp, np.float64)
    xt = torch.tensor(np.asarray(x, np.float64).reshape((sp["W"], sp["H"], sp["C"], B), order="F").transpose(3, 2, 1, 0).copy(), requires_grad=True)
    wt = [torch.tensor(w[::-1, ::-1].transpose(3, 2, 1, 0).copy(), requires_grad=True) for w in Ws]
    bt = [torch.tensor(b, requires_grad=True) for b in bs]
    h = xt * float(np.float32(sp["scale"]))
    for ly, w, b in zip(sp["layers"], wt, bt):
        h = torch.nn.functional.conv2d(h, w, b, stride=(ly["stride"][1], ly["stride"][0]), padding=(ly["pad"][1], ly["pad"][0]))
        h = torch.relu(h) if ly["act"] == "relu" else torch.tanh(h) if ly["act"] == "tanh" else h
    OW, OH, co = CR.extents(sp)[-1]
    yf = h.permute(3, 2, 1, 0).detach().numpy().reshape((OW * OH * co, B), order="F")
    dyt = torch.tensor(np.asarray(dy, np.float64).reshape((OW, OH, co, B), order="F").transpose(3, 2, 1, 0).copy())
    (h * dyt).sum().backward()
    dW = [w.grad.numpy().transpose(3, 2, 1, 0)[::-1, ::-1] for w in wt]
    dx = xt.grad.numpy().transpose(3, 2, 1, 0).reshape((-1, B), order="F")
    return yf, dx, dW, [b.grad.numpy() for b in bt]


SCALED = (CR.spec(8, 8, 2, [CR.layer((4, 4), 2, 3, "tanh", 2), CR.layer((2, 2), 3, 2, "relu", 1)], scale=1.0 / 255.0), 3)      # the input-scale path (forward, and dx times scale) on pixel values


@pytest.mark.parametrize("case", CR.grid_cases()[:-1] + [SCALED, (CR.ATARI, 1)], ids=CR.case_id)
def test_float64_reference_matches_torch_conv2d_and_autograd(case):
    sp, B = case
    p, x, dy = CR.case_inputs(case)
    r = CR.trunk_reference(p, sp, x, dy)
    y, dx, dW, db = _torch_trunk(p, sp, x, dy)
    assert np.abs(r["y"] - y).max() <= 1e-12 * max(1, np.abs(y).max())
    assert np.abs(r["dx"] - dx).max() <= 1e-12 * max(1, np.abs(dx).max())
    for l in range(len(dW)):
        assert np.abs(r["dW"][l] - dW[l]).max() <= 1e-12 * max(1, np.abs(dW[l]).max()) and np.abs(r["db"][l] - db[l]).max() <= 1e-12 * max(1, np.abs(db[l]).max())


def test_uncovered_inputs_have_exactly_zero_gradient():
    case = [c for c in CR.grid_cases() if c[0]["layers"][0]["stride"] == (3, 3)][0]
    sp, B = case; p, x, dy = CR.case_inputs(case)
    for r in (CR.trunk_reference(p, sp, x, dy), CR.emulated_reference(p, sp, x, dy)):
        dx = r["dx"].reshape((11, 11, B), order="F")
        assert np.all(dx[2::3] == 0) and np.all(dx[:, 2::3] == 0) and np.count_nonzero(dx) == 8 * 8 * B


def tensors(r, sp):
    out = [("y", r["y"]), ("dx", r["dx"])]
    for l in range(len(sp["layers"])):
        out += [("dW%d" % l, r["dW"][l]), ("db%d" % l, r["db"][l])]
    return out


def test_emulated_kernel_order_sets_the_margin():
    """M_MARGIN = 2 x the worst ratio of the emulated kernel order's error to max(e32, u) over the grid: measured here, recorded in conv_reference.py"""
    worst, where = 0.0, None
    for case in CR.grid_cases():
        sp, B = case; p, x, dy = CR.case_inputs(case)
        r64, r32, rem = CR.trunk_reference(p, sp, x, dy), CR.trunk_reference(p, sp, x, dy, np.float32), CR.emulated_reference(p, sp, x, dy)
        for (name, t64), (_, t32), (_, tem) in zip(tensors(r64, sp), tensors(r32, sp), tensors(rem, sp)):
            e32, eem = CR.rel_err(t32, t64), CR.rel_err(tem, t64); ratio = eem / max(e32, CR.U32)
            print("EMUL %s %s e32_u %.3f emul_u %.3f ratio %.3f" % (CR.case_id(case), name, e32 / CR.U32, eem / CR.U32, ratio))
            if ratio > worst:
                worst, where = ratio, (CR.case_id(case), name)
    print("EMUL worst ratio %.3f at %s" % (worst, where))
    assert worst <= CR.M_EMULATED_WORST + 0.005 and where == CR.M_EMULATED_WORST_CASE, (worst, where)
    assert CR.M_MARGIN == 2 * CR.M_EMULATED_WORST


def test_scale_prelude_is_one_float32_multiply():
    sp = CR.spec(4, 4, 1, [CR.layer((2, 2), 1, 2)], scale=1.0 / 255.0); rng = np.random.default_rng(0)
    p = CR.glorot_params(sp, rng); x = rng.integers(0, 256, (16, 3)).astype(np.float32); dy = np.ones((18, 3), np.float32)
    sp1 = dict(sp, scale=1.0)
    a = CR.trunk_reference(p, sp, x, dy, np.float32)["y"]; b = CR.trunk_reference(p, sp1, (x * np.float32(1.0 / 255.0)).astype(np.float32), dy, np.float32)["y"]
    assert np.array_equal(a, b)


def test_adam_bound_holds_for_the_float32_restatement():
    """|(p' - p) - Delta64(g)| <= adam_small(p, eta) eta for the kernel's arithmetic (Float64 update from Float32 m, v, rounded once, subtracted in Float32), tiny and zero
    gradients included; and sign(p' - p) = -sign(g) wherever the update does not vanish against p's spacing"""
    rng = np.random.default_rng(1); eta = 1e-3
    p = rng.normal(0, 0.3, 4000).astype(np.float32)
    g = (rng.normal(0, 1, 4000) * 10.0 ** rng.uniform(-12, 0, 4000)).astype(np.float32); g[:50] = 0
    pn = CR.adam_first_step_f32(p, g, eta)
    d64 = CR.adam_first_step_delta(g, eta)
    assert np.all(np.abs((pn.astype(np.float64) - p) - d64) <= CR.adam_small(p, eta) * eta)
    assert np.all(np.abs(pn.astype(np.float64) - p) <= eta * (1 + CR.adam_small(p, eta)))
    assert CR.adam_sign_ok(p, pn, g, eta)
    assert not CR.adam_sign_ok(p, p + (p - pn), g, eta)      # an update of the wrong sign is seen
