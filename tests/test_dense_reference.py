"""CPU tests of tests/dense_reference.py: the float64 chain against torch autograd, the kink-free draw on every relu member of the engine grid, and the margin of the
grid test (tests/test_gpu_dense_grid.py) from the float32 emulation of the engine's defined summation order. No GPU, no library."""
import numpy as np
import pytest

import dense_reference as R


def _torch_chain(params, dims, acts, x, dy):
    import torch
    torch.set_num_threads(1)
    Ws, bs = [], []
    for l, (wo, bo) in enumerate(R.layer_offsets(dims)):
        i, o = dims[l], dims[l + 1]
        Ws.append(torch.tensor(np.asarray(params[wo:bo], np.float64).reshape((o, i), order="F").copy(), requires_grad=True))
        bs.append(torch.tensor(np.asarray(params[bo:bo + o], np.float64), requires_grad=True))
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True); h = xt
    for l, a in enumerate(acts):
        z = Ws[l] @ h + bs[l][:, None]
        h = torch.relu(z) if a == "relu" else torch.tanh(z) if a == "tanh" else z
    h.backward(torch.tensor(np.asarray(dy, np.float64)))
    return h.detach().numpy(), xt.grad.numpy(), [w.grad.numpy() for w in Ws], [b.grad.numpy() for b in bs]


@pytest.mark.parametrize("dims,acts,B", [([3, 32, 1], ["tanh", "identity"], 37), ([4, 64, 64, 2], ["relu", "relu", "identity"], 130), ([8, 48, 40, 4], ["relu", "relu", "tanh"], 19),
                                         ([8, 32, 24, 16, 4], ["relu", "tanh", "relu", "identity"], 65), ([5, 3], ["identity"], 7), ([17, 64, 32, 6], ["tanh", "tanh", "identity"], 200)])
def test_chain_reference_float64_is_torch_autograd(dims, acts, B):
    rng = np.random.default_rng(5)
    p = R.perturbed_params(R.glorot_params(dims, rng), rng)
    x = R.kink_free_inputs(p, dims, acts, B, rng); dy = rng.normal(0, 1, (dims[-1], B)).astype(np.float32)
    ref = R.chain_reference(p, dims, acts, x, dy, np.float64)
    y, dx, dW, db = _torch_chain(p, dims, acts, x, dy)
    assert np.abs(ref["y"] - y).max() <= 1e-13 * max(1, np.abs(y).max()) and np.abs(ref["dx"] - dx).max() <= 1e-12 * max(1, np.abs(dx).max())
    for l in range(len(acts)):
        assert np.abs(ref["dW"][l] - dW[l]).max() <= 1e-12 * max(1, np.abs(dW[l]).max()), l
        assert np.abs(ref["db"][l] - db[l]).max() <= 1e-12 * max(1, np.abs(db[l]).max()), l
    # the pair test_gpu_sac.py has always used is the same function
    hs = R._np_mlp(p, dims, acts, x); g, d = R._np_backward(p, dims, acts, hs, dy)
    assert np.abs(g - R.flat_gradient(ref, dims)).max() <= 1e-12 * max(1, np.abs(g).max()) and np.abs(d - ref["dx"]).max() <= 1e-12 * max(1, np.abs(d).max())


def test_chain_reference_keeps_the_requested_precision():
    rng = np.random.default_rng(6); dims, acts = [4, 64, 64, 2], ["relu", "tanh", "identity"]
    p = R.perturbed_params(R.glorot_params(dims, rng), rng); x = rng.normal(0, 1, (4, 33)).astype(np.float32); dy = rng.normal(0, 1, (2, 33)).astype(np.float32)
    r32 = R.chain_reference(p, dims, acts, x, dy, np.float32)
    assert all(t.dtype == np.float32 for t in [r32["y"], r32["dx"]] + r32["dW"] + r32["db"])
    r64 = R.chain_reference(p, dims, acts, x, dy, np.float64)
    assert 0 < R.rel_err(r32["dW"][1], r64["dW"][1]) < 64 * R.U32      # float32 really was used, and is float32-close


def test_grid_names_every_edge():
    cs = R.grid_cases(); ids = [R.case_id(c) for c in cs]
    assert len(set(ids)) == len(ids) and 120 <= len(cs) <= 200, len(cs)
    for w in R.FUSED_WIDTHS:                                              # every fused width pair at every B of the pullback's window
        for B in R.FUSED_B:
            assert any(tuple(d[1:3]) == w and b == B and len(d) == 4 for d, _, b in cs), (w, B)
    have = lambda f: sum(1 for c in cs if f(*c))
    assert have(lambda d, a, B: len(d) == 4 and d[1] == 192 and d[2] == 192) >= 7
    for in0 in (1, 3, 16, 17, 32, 33):
        assert have(lambda d, a, B: d[0] == in0 and len(d) == 4 and d[1] in (128, 192, 256)) >= 2, in0
    for out_ in (1, 4, 2, 6, 17):
        assert have(lambda d, a, B: d[-1] == out_ and R.is_fused_backward(d, B)) >= 2, out_
    assert have(lambda d, a, B: a[-1] == "tanh" and R.is_fused_backward(d, B)) >= 2
    for B in (1, 15, 16, 17, 127, 128, 129, 200, 255, 256, 257, 512, 1000, 4000, 4097, 5003):
        assert have(lambda d, a, b: b == B) >= 2, B
    assert have(lambda d, a, B: B == 4112 and d[1] == 256) >= 2 and have(lambda d, a, B: B == 4096 and d[1] == 256) >= 2 and have(lambda d, a, B: B == 65536) == 1
    assert have(lambda d, a, B: len(d) == 2) >= 2 and have(lambda d, a, B: len(d) == 5) >= 2
    for h in ((256, 64), (64, 256), (64, 64), (48, 48), (160, 96), (320, 320), (130, 50)):
        assert have(lambda d, a, B: len(d) == 4 and tuple(d[1:3]) == h) >= 2, h


@pytest.mark.parametrize("case", [c for c in R.grid_cases() if "relu" in c[1]], ids=R.case_id)
def test_kink_free_inputs_terminates_on_the_grid(case):
    dims, acts, B = case
    rng = np.random.default_rng(3)
    p = R.perturbed_params(R.glorot_params(dims, rng), rng); st = {}
    x = R.kink_free_inputs(p, dims, acts, B, rng, 1e-4, stats=st)
    assert x.shape == (dims[0], B) and x.dtype == np.float32 and x.flags.f_contiguous
    assert not R._near_kink(p, dims, acts, x, 1e-4).any() and st["rounds"] <= 32


def test_kink_free_inputs_gives_up():
    dims, acts = [2, 4, 1], ["relu", "identity"]
    p = np.zeros(R.n_layer_params(dims), np.float32)          # every pre-activation is exactly 0
    with pytest.raises(RuntimeError):
        R.kink_free_inputs(p, dims, acts, 8, np.random.default_rng(0), 1e-4, max_rounds=3)


def test_gemm16_order_is_the_defined_order():
    rng = np.random.default_rng(1)
    A = rng.normal(0, 1, (5, 130)).astype(np.float32); B = rng.normal(0, 1, (130, 3)).astype(np.float32)
    assert R._quarters(130, None) == [(0, 48), (48, 96), (96, 130), (130, 130)] and R._quarters(127, None) == [(0, 127)] and R._quarters(256, None) == [(0, 64), (64, 128), (128, 192), (192, 256)]
    want = np.zeros((5, 3), np.float32)
    for i in range(5):
        for j in range(3):
            qs = []
            for kb, ke in R._quarters(130, None):
                s = np.float32(0)
                for k in range(kb, ke):
                    s = np.float32(s + np.float32(A[i, k] * B[k, j]))
                qs.append(s)
            want[i, j] = np.float32(np.float32(np.float32(qs[0] + qs[1]) + qs[2]) + qs[3])
    assert np.array_equal(R.gemm16_order_f32(A, B), want)
    one = R.gemm16_order_f32(A, B, split=False)
    assert not np.array_equal(one, want) and np.abs(one - A.astype(np.float64) @ B.astype(np.float64)).max() < 1e-4
    assert np.abs(R.rowsum16_order_f32(A) - A.astype(np.float64).sum(axis=1)).max() < 1e-4


_RATIOS = {}


@pytest.mark.parametrize("case", [c for c in R.grid_cases() if c[2] <= 1000], ids=R.case_id)
def test_emulated_engine_order_stays_inside_the_margin(case):
    """The margin M of the grid test is chosen here, from the CPU alone: M is twice the worst ratio the float32 emulation of the engine's defined order reaches against
    max(e32, u) over every tensor of every grid member with B <= 1000 (dense_reference.M_EMULATED_WORST, measured by this test; the other half is left for the fma contraction
    of the MFMA chain and another BLAS). The emulation must stay inside the grid's bound M x max(e32, u). Never fitted to what the GPU produced."""
    dims, acts, B = case
    rng = np.random.default_rng(3)
    p = R.perturbed_params(R.glorot_params(dims, rng), rng)
    x = R.kink_free_inputs(p, dims, acts, B, rng) if "relu" in acts else np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    dy = rng.normal(0, 1, (dims[-1], B)).astype(np.float32)
    r64 = R.chain_reference(p, dims, acts, x, dy, np.float64); r32 = R.chain_reference(p, dims, acts, x, dy, np.float32)
    rem = R.chain_reference(p, dims, acts, x, dy, np.float32, mm=R.gemm16_order_f32, rowsum=R.rowsum16_order_f32)
    worst = 0.0
    for name, get in [("y", lambda r: r["y"]), ("dx", lambda r: r["dx"])] + [("dW%d" % l, lambda r, l=l: r["dW"][l]) for l in range(len(acts))] + [("db%d" % l, lambda r, l=l: r["db"][l]) for l in range(len(acts))]:
        e32, eem = R.rel_err(get(r32), get(r64)), R.rel_err(get(rem), get(r64))
        ratio = eem / max(e32, R.U32); worst = max(worst, ratio)
        _RATIOS[(R.case_id(case), name)] = (e32 / R.U32, eem / R.U32, ratio)
        print("%-34s %-4s e32 %7.2f u  emulated %7.2f u  ratio %.2f" % (R.case_id(case), name, e32 / R.U32, eem / R.U32, ratio))
        assert ratio <= R.M_MARGIN, (name, e32 / R.U32, eem / R.U32)
