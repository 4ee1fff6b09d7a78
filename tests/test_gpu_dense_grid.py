"""The dense tile-GEMM engine (csrc/dense.hip, csrc/dense_fused.h) against float64 at every tile edge.

One parametrised test walks an explicit shape grid (tests/dense_reference.py: grid_cases) through crux_mlp_forward_cached / crux_mlp_backward and compares y, dx and every
layer's dW, db with chain_reference(float64). A tensor T passes iff
    max |T_gpu - T_f64| / max |T_f64|  <=  M x max(e32(T), u),        u = 2^-24,
where e32(T) is the same quantity for the float32 NumPy restatement of the chain on the same inputs: the bound is the reference's own float32 error, not a number taken from the
kernel. M comes from the CPU alone (dense_reference.M_MARGIN; tests/test_dense_reference.py). relu members draw kink-free observations, so no entry is left out of any comparison.
The 1e-4 / 2e-5 assertions of tests/test_gpu_sac.py stay beside the new bound as an outer guard.

What the C ABI reaches: with parameter gradients wanted, crux_mlp_backward runs the per-layer launches whatever the shape (the fused pair leaves layer 0's gradient as quarter
partials that only the learners' Sumsq2Op completes); with want_param_grads = 0 it runs the fused pullback (Dgrad2W1Op, and the output layer folded in for widths 1 and 4) on the
shapes of df_bwd_ok. Every case therefore takes the input gradient BOTH ways and compares both with float64. Wgrad2Op and the quarter partials are compared with the oracle through
the learner (tests/test_gpu_dense_learner.py: 8-256-256-4 and 4-192-192-1 at a minibatch of 256).

Three further tests: the switch forms CRUX_DENSE_FUSED = 0 / 1 / 2 give identical bits; one handle called at B = 37, 4097, 129, 37 (the workspace grows once and is then re-used
at smaller B with the offsets of the larger one) equals a fresh handle bit for bit; the want_param_grads / d_dx flags select outputs without changing them.
Measured figures: profiles/dense_grid_parity.txt.
"""
import numpy as np
import pytest

import dense_reference as R
import parity
from parity import crux

pytestmark = pytest.mark.gpu
GSCALE = 0.5      # != 1 and a power of two: the scaled gradient is compared without a rounding of the test's own


class _Run:
    """forward + pullback of one handle through the C ABI"""

    def __init__(self, ctx, dims, acts, params=None, seed=7):
        self.ctx, self.dims = ctx, dims
        self.net = crux.ContinuousNetwork(parity.chain(dims, acts), seed=seed, stream=2, ctx=ctx)
        if params is not None:
            self.net.set_params(params)

    def __call__(self, x, dy, want_g=1, want_dx=True):
        ctx, net, B = self.ctx, self.net, x.shape[1]
        d_x, d_dy, d_y, d_dx = ctx.alloc(x.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
            ctx.check(ctx.lib.crux_mlp_forward_cached(net.h, d_x, B, d_y))
            ctx.check(ctx.lib.crux_mlp_backward(net.h, d_x, B, d_dy, GSCALE, want_g, d_dx if want_dx else None))
            y, dx, g = np.empty_like(dy), np.empty_like(x), np.empty(net.n_params, np.float32)
            ctx.d2h(d_y, y); ctx.d2h(ctx.lib.crux_mlp_grads_ptr(net.h), g)
            if want_dx:
                ctx.d2h(d_dx, dx)
            return y, (dx if want_dx else None), g
        finally:
            for d in (d_x, d_dy, d_y, d_dx):
                ctx.free(d)


def _inputs(p, dims, acts, B, rng):
    x = R.kink_free_inputs(p, dims, acts, B, rng) if "relu" in acts else np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    return x, np.asfortranarray(rng.normal(0, 1, (dims[-1], B)).astype(np.float32))


@pytest.mark.parametrize("case", R.grid_cases(), ids=R.case_id)
def test_dense_engine_matches_float64_on_the_grid(gpu_ctx, case):
    dims, acts, B = case
    run = _Run(gpu_ctx, dims, acts); rng = np.random.default_rng(3)
    p = R.perturbed_params(run.net.get_params(), rng); run.net.set_params(p)      # non-zero biases
    x, dy = _inputs(p, dims, acts, B, rng)
    y, dx, g = run(x, dy, 1, True)
    _, dx_only, _ = run(x, dy, 0, True)                                             # the fused pullback where the shape has one
    r64, r32 = R.chain_reference(p, dims, acts, x, dy, np.float64), R.chain_reference(p, dims, acts, x, dy, np.float32)
    offs = R.layer_offsets(dims)
    tensors = [("y", y, r64["y"], r32["y"]), ("dx", dx, r64["dx"], r32["dx"]), ("dx_only", dx_only, r64["dx"], r32["dx"])]
    for l, (wo, bo) in enumerate(offs):
        i, o = dims[l], dims[l + 1]
        tensors.append(("dW%d" % l, (g[wo:bo] / GSCALE).reshape((o, i), order="F"), r64["dW"][l], r32["dW"][l]))
        tensors.append(("db%d" % l, g[bo:bo + o] / GSCALE, r64["db"][l], r32["db"][l]))
    bad = []
    for name, t, t64, t32 in tensors:
        e32, eg = R.rel_err(t32, t64), R.rel_err(t, t64); ratio = eg / max(e32, R.U32)
        print("GRID %s %s e32_u %.3f gpu_u %.3f ratio %.3f" % (R.case_id(case), name, e32 / R.U32, eg / R.U32, ratio))
        if not eg <= R.M_MARGIN * max(e32, R.U32):
            bad.append((name, "e32 %.2f u" % (e32 / R.U32), "gpu %.2f u" % (eg / R.U32), "ratio %.2f > M = %.2f" % (ratio, R.M_MARGIN)))
    assert not bad, bad
    # the outer guard: the assertions of test_gpu_sac.py::test_dense_forward_backward_match_float64
    gref = R.flat_gradient(r64, dims)
    assert np.abs(y - r64["y"]).max() < 2e-5 * max(1, np.abs(r64["y"]).max())
    assert np.abs(dx - r64["dx"]).max() < 1e-4 * max(1, np.abs(r64["dx"]).max()) and np.abs(dx_only - r64["dx"]).max() < 1e-4 * max(1, np.abs(r64["dx"]).max())
    assert np.abs(g[:gref.size] - GSCALE * gref).max() < 1e-4 * max(1, np.abs(gref).max())


_FUSED = [c for c in R.grid_cases() if R.is_fused_forward(c[0]) or R.is_fused_backward(c[0], c[2])]


@pytest.mark.parametrize("case", _FUSED, ids=R.case_id)
def test_switch_forms_give_identical_bits(gpu_ctx, monkeypatch, case):
    """CRUX_DENSE_FUSED = 0 (every layer its own Gemm16 launch), 1 (Fwd12Op, the fused pullback with the narrow output layer folded in) and 2 (the pair without the folded
    output layer): dense_fused.h claims the same bits. y and the flat gradient from the full call, dx from the full call and from the input-gradient-only call."""
    dims, acts, B = case
    run = _Run(gpu_ctx, dims, acts); rng = np.random.default_rng(4)
    p = R.perturbed_params(run.net.get_params(), rng); run.net.set_params(p)
    x, dy = _inputs(p, dims, acts, B, rng)
    res = {}
    for form in ("0", "1", "2"):
        monkeypatch.setenv("CRUX_DENSE_FUSED", form)
        y, dx, g = run(x, dy, 1, True); _, dx_only, _ = run(x, dy, 0, True)
        res[form] = (y, dx, g, dx_only)
    for form in ("1", "2"):
        for name, a, b in zip(("y", "dx", "gradient", "dx_only"), res["0"], res[form]):
            assert np.array_equal(a, b), (form, name, float(np.abs(a - b).max()))
    assert np.array_equal(res["0"][1], res["0"][3])      # and the two ways to the input gradient agree


@pytest.mark.parametrize("dims,acts", [([8, 256, 256, 4], R.RELU3), ([17, 64, 64, 6], R.TANH3), ([4, 192, 192, 1], R.TANH3)], ids=["8-256-256-4", "17-64-64-6", "4-192-192-1"])
def test_one_handle_across_growing_and_shrinking_batches(gpu_ctx, dims, acts):
    """ensure_ws sizes the workspace to the next power of two >= B and never shrinks it; crux_dense_act / ws_delta / ws_part derive their offsets from that capacity. One handle
    at B = 37, 4097, 129, 37 must give what a fresh handle gives at each B."""
    rng = np.random.default_rng(5)
    one = _Run(gpu_ctx, dims, acts); p = R.perturbed_params(one.net.get_params(), rng); one.net.set_params(p)
    for B in (37, 4097, 129, 37):
        x, dy = _inputs(p, dims, acts, B, np.random.default_rng(100 + B))
        fresh = _Run(gpu_ctx, dims, acts, params=p)
        for want_g in (1, 0):
            for name, a, b in zip(("y", "dx", "gradient"), one(x, dy, want_g, True), fresh(x, dy, want_g, True)):
                if want_g or name != "gradient":
                    assert np.array_equal(a, b), (B, want_g, name, float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", [([8, 256, 256, 4], R.RELU3, 200), ([16, 192, 128, 1], R.TANH3, 129), ([17, 64, 64, 6], R.TANH3, 1000), ([33, 130, 50, 6], R.TANH3, 257), ([5, 3], ["identity"], 130)], ids=R.case_id)
def test_flags_select_outputs_without_changing_them(gpu_ctx, case):
    """want_param_grads = 0 with d_dx given, and d_dx = NULL with gradients wanted, against the full call (on the first two shapes the former is the fused pullback)."""
    dims, acts, B = case
    run = _Run(gpu_ctx, dims, acts); rng = np.random.default_rng(6)
    p = R.perturbed_params(run.net.get_params(), rng); run.net.set_params(p)
    x, dy = _inputs(p, dims, acts, B, rng)
    y, dx, g = run(x, dy, 1, True)
    _, dx_only, _ = run(x, dy, 0, True)
    assert np.array_equal(dx_only, dx), float(np.abs(dx_only - dx).max())
    _, _, g_other = run(x, (2 * dy).astype(np.float32), 1, True)      # the gradient buffer now holds something else ...
    assert not np.array_equal(g_other, g)
    y2, none, g_only = run(x, dy, 1, False)                            # ... and the call without d_dx writes the full call's bits over it
    assert none is None and np.array_equal(y2, y) and np.array_equal(g_only, g), float(np.abs(g_only - g).max())
