"""The branches of the conv trunk (csrc/conv.hip, conv_pair.hip, conv_group.hip) that conv_reference.grid_cases() never reaches, on conv_reference.edge_cases(): three and
four layers (the rotation of the two delta buffers, with and without the first swap), cin > 16 (two row tiles in the data gradient, at layer 0 and behind an activation), the
vector-load forward with padding along H, with K no multiple of 64 and at an inner layer, the host's alignment decision, padding combined with stride, H = 1, pad = k - 1, k1 = 1.

1. Every edge case against trunk_reference(float64) under test_gpu_conv.py's rule err <= M max(e32, u), M = conv_reference.M_MARGIN from the CPU alone, grad_scale = 0.5.
2. The vector-load and the dword form of the forward kernel give the same bits: the same bytes read from a 16-byte-aligned d_x and from d_x + 4 inside an allocation the test owns.
3. crux_conv_forward_pair / crux_conv_backward_pair equal two single passes bit for bit on the deep, wide and inner-VEC trunks, both d_dx asked for.
4. crux_conv_ensemble_passes equals the single-member entries bit for bit at M = 3 (the three-member body alone) and M = 7 (a group of 4 and one of 3).
5. One handle at B = 3, 40, 3 on the four-layer trunk: the workspace grows under it and the bits stay those of a fresh handle."""
import ctypes as C

import numpy as np
import pytest

import conv_pg_reference as PG
import conv_reference as CR
import dense_reference as R
from test_gpu_conv import GSCALE, _Run, _bound_check, _grad_tensors
from test_gpu_conv_ensemble import _Members

pytestmark = pytest.mark.gpu
EXACT_ZEROS = (CR.FULL, CR.PADSTR)      # padding: the inputs whose gradient is exactly 0 are the reference's


@pytest.mark.parametrize("case", CR.edge_cases(), ids=CR.case_id)
def test_trunk_matches_float64_on_the_edge_cases(gpu_ctx, case):
    sp, B = case
    p, x, dy = CR.case_inputs(case)
    y, dx, g = _Run(gpu_ctx, sp, p)(x, dy)
    r64, r32 = CR.trunk_reference(p, sp, x, dy, np.float64), CR.trunk_reference(p, sp, x, dy, np.float32)
    tensors = [("y", y, r64["y"], r32["y"]), ("dx", dx, r64["dx"], r32["dx"])]
    for name, t, l, kind in _grad_tensors(g / GSCALE, sp):
        tensors.append((name, t, r64[kind][l], r32[kind][l]))
    assert len(tensors) == 2 + 2 * len(sp["layers"])
    _bound_check(CR.case_id(case), tensors)
    if any(sp is s for s in EXACT_ZEROS):
        assert np.count_nonzero(dx) == np.count_nonzero(r64["dx"])


def _passes_from(run, x, dy, shift):
    """forward + pullback with the observations at d_x + shift bytes of an allocation of x.nbytes + 16"""
    ctx, t, B = run.ctx, run.t, x.shape[1]
    base, d_dy, d_y, d_dx = ctx.alloc(x.nbytes + 16), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(x.nbytes)
    try:
        assert base.value % 16 == 0 and shift % 4 == 0 and 0 <= shift <= 16
        d_x = C.c_void_p(base.value + shift)
        ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
        ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, d_y))
        ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_dy, GSCALE, 1, d_dx))
        return ctx.d2h(d_y, np.empty_like(dy)), ctx.d2h(d_dx, np.empty_like(x)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(t.p.h), np.empty(t.p.n_params, np.float32))
    finally:
        for d in (base, d_dy, d_y, d_dx):
            ctx.free(d)


def _pixel_inputs(sp, B, seed):
    rng = np.random.default_rng(seed); p = CR.perturbed(CR.glorot_params(sp, rng), rng)
    x = np.asfortranarray(rng.integers(0, 256, (sp["W"] * sp["H"] * sp["C"], B)).astype(np.float32))
    return p, x, np.asfortranarray(rng.normal(0, 1, (CR.n_features(sp), B)).astype(np.float32))


SCALE16 = CR.spec(16, 16, 2, [CR.layer((4, 4), 2, 5, "tanh", 4)], scale=1.0 / 255.0)      # the 16x16 case of test_input_scale_is_one_multiply_to_the_bit
FORM_CASES = {"vecpad": (CR.VECPAD, lambda: CR.case_inputs((CR.VECPAD, 5))), "pg_vec": (PG.VEC, lambda: _pixel_inputs(PG.VEC, 33, 8)), "scale16": (SCALE16, lambda: _pixel_inputs(SCALE16, 6, 5))}


@pytest.mark.parametrize("name", list(FORM_CASES))
def test_vector_and_dword_forms_agree_bit_for_bit(gpu_ctx, name):
    """conv_fwd_vec takes the vector-load form from an aligned d_x and the dword form from d_x + 4; which k meets which does not change, so neither may a bit"""
    sp, inputs = FORM_CASES[name]; p, x, dy = inputs()
    assert CR.fwd_vec_expected(sp, 0)
    vec, dword = _passes_from(_Run(gpu_ctx, sp, p), x, dy, 0), _passes_from(_Run(gpu_ctx, sp, p), x, dy, 4)
    for what, a, b in zip(("y", "dx", "gradient"), vec, dword):
        assert np.any(a) and np.array_equal(a, b), what


PAIR_CASES = [c for c in CR.edge_cases() if any(c[0] is s for s in (CR.L3, CR.L4, CR.CIN, CR.VECIN, CR.VECOFF))]


@pytest.mark.parametrize("case", PAIR_CASES, ids=CR.case_id)
def test_pair_equals_two_single_passes_bit_for_bit(gpu_ctx, case):
    ctx, (sp, B) = gpu_ctx, case; rng = np.random.default_rng(17)
    ins = [CR.case_inputs(case, seed=3 + m) for m in range(2)]; ps = [i[0] for i in ins]; x = ins[0][1]
    dys = [np.asfortranarray(rng.normal(0, 1, (CR.n_features(sp), B)).astype(np.float32)) for _ in range(2)]
    assert not np.array_equal(ps[0], ps[1])
    single = [_Run(ctx, sp, p)(x, dy) for p, dy in zip(ps, dys)]
    t = [_Run(ctx, sp, p).t for p in ps]
    d = [ctx.alloc(a.nbytes) for a in (x, dys[0], dys[1], dys[0], dys[1], x, x)]      # x, dy0, dy1, y0, y1, dx0, dx1
    try:
        for dst, a in zip(d[:3], (x, dys[0], dys[1])):
            ctx.h2d(dst, a)
        ctx.check(ctx.lib.crux_conv_forward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[3], d[4]))
        ctx.check(ctx.lib.crux_conv_backward_pair(t[0].h, t[0].p.h, t[1].h, t[1].p.h, d[0], B, d[1], d[2], GSCALE, 1, d[5], d[6]))
        for m in range(2):
            got = (ctx.d2h(d[3 + m], np.empty_like(dys[m])), ctx.d2h(d[5 + m], np.empty_like(x)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(t[m].p.h), np.empty(ps[m].size, np.float32)))
            for name, a, b in zip(("y", "dx", "gradient"), got, single[m]):
                assert np.any(b) and np.array_equal(a, b), (m, name)
    finally:
        for q in d:
            ctx.free(q)


GROUP_CASES = [(c, M) for c in CR.edge_cases() if any(c[0] is s for s in (CR.L4, CR.VECPAD, CR.VECIN)) for M in (3, 7)]


@pytest.mark.parametrize("case,M", GROUP_CASES, ids=["%s_M%d" % (CR.case_id(c), M) for c, M in GROUP_CASES])
def test_grouped_passes_equal_single_passes_bit_for_bit(gpu_ctx, case, M):
    sp, B = case; F = CR.n_features(sp); dims, acts = [F, 24, 3], ["tanh", "identity"]; rng = np.random.default_rng(M)
    ins = [CR.case_inputs(case, seed=3 + m) for m in range(M)]; x = ins[0][1]
    phs = [R.perturbed_params(R.glorot_params(dims, rng), rng) for _ in range(M)]; dys = [np.asfortranarray(rng.normal(0, 1, (3, B)).astype(np.float32)) for _ in range(M)]
    ref = _Members(gpu_ctx, sp, dims, acts, [i[0] for i in ins], phs)      # the single passes run on handles of their own (test_gpu_conv_ensemble.py)
    want = [ref.single(m, x, dys[m], F) for m in range(M)]
    got = _Members(gpu_ctx, sp, dims, acts, [i[0] for i in ins], phs).passes(x, dys, F)
    for m in range(M):
        for name, a, b in zip(("output", "d_dx of the head", "trunk gradient", "head gradient"), got[m], want[m]):
            assert np.any(b) and np.array_equal(a, b), (m, name)


def test_one_handle_across_batches_on_the_four_layer_trunk(gpu_ctx):
    """B = 3, then 40 (the workspace grows from 32 to 64 columns: every cached output and both delta buffers move), then 3 again"""
    sp = CR.L4; p, x3, dy3 = CR.case_inputs((sp, 3)); rng = np.random.default_rng(9)
    x40 = np.asfortranarray(rng.normal(0, 1, (x3.shape[0], 40)).astype(np.float32)); dy40 = np.asfortranarray(rng.normal(0, 1, (dy3.shape[0], 40)).astype(np.float32))
    one = _Run(gpu_ctx, sp, p)
    first, big, last = one(x3, dy3), one(x40, dy40), one(x3, dy3)
    for B, got, args in ((3, last, (x3, dy3)), (40, big, (x40, dy40))):
        fresh = _Run(gpu_ctx, sp, p)(*args)
        for name, a, b in zip(("y", "dx", "gradient"), got, fresh):
            assert np.any(b) and np.array_equal(a, b), (B, name)
    for a, b in zip(first, last):
        assert np.array_equal(a, b)
