"""Ensembles whose members are conv chains (csrc/conv_group.hip, the conv entries of csrc/ensemble.hip): the grouped passes bit for bit against the single-member entries on
handles of their own; one step of both kinds against float64 under test_gpu_conv.py's rule err <= M_MARGIN max(e32, u); the NaN gate; the host mirror and its refusals."""
import ctypes as C

import numpy as np
import pytest

import conv_ensemble_reference as CER
import conv_reference as CR
import dense_reference as R
import ensemble_reference as ER
from parity import crux
from crux_jl_amd import _lib as L
from test_gpu_conv import _Run, _bound_check, _flat_slices
from test_gpu_wide import Handle

pytestmark = pytest.mark.gpu
MM, U, ETA = CR.M_MARGIN, CR.U32, float(np.float32(1e-3))
_CASES = {CR.case_id(c): c for c in CR.grid_cases()}
SMALL = [_CASES["9x7x3_5@3x2s2x1p0x0r_B37"], _CASES["10x10x2_16@3x3s1x1p1x1r_B5"]]
BIG = [(CR.TWO_LAYER, 7), (CR.ATARI, 4)]
PASS_CASES = [(c, M) for c in SMALL for M in (1, 2, 5, 16)] + [(c, M) for c in BIG for M in (1, 2, 5)]


def _ptrs(hs):
    return (C.c_void_p * len(hs))(*[getattr(h, "value", h) for h in hs])


class _Members:
    """M trunks (test_gpu_conv._Run) and M dense heads of one shape, and the three handle arrays of the C ABI"""

    def __init__(self, ctx, sp, dims, acts, pts, phs):
        self.ctx, self.t = ctx, [_Run(ctx, sp, p).t for p in pts]
        self.heads = [Handle(ctx, dims, acts) for _ in phs]      # crux_mlp_create_wide: the padded and the Atari case flatten to 1600 and 2048 features
        for h, p in zip(self.heads, phs):
            h.set(p)
        self.arrs = (_ptrs([t.h for t in self.t]), _ptrs([t.p.h for t in self.t]), _ptrs([h.h for h in self.heads]))

    def grads(self, m):
        ctx = self.ctx; return (ctx.d2h(ctx.lib.crux_mlp_grads_ptr(self.t[m].p.h), np.empty(self.t[m].p.n_params, np.float32)), ctx.d2h(ctx.lib.crux_mlp_grads_ptr(self.heads[m].h), np.empty(self.heads[m].n, np.float32)))

    def passes(self, x, dys, F):
        """crux_conv_ensemble_passes: per member (head output, head d_dx, trunk gradient, head gradient)"""
        ctx, M, B = self.ctx, len(self.t), x.shape[1]
        d_x = ctx.alloc(x.nbytes); d = [[ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(4 * F * B)] for dy in dys]; ctx.h2d(d_x, x)
        for q, dy in zip(d, dys):
            ctx.h2d(q[0], dy)
        try:
            ctx.check(ctx.lib.crux_conv_ensemble_passes(*self.arrs, M, d_x, B, _ptrs([q[0] for q in d]), _ptrs([q[1] for q in d]), _ptrs([q[2] for q in d])))
            return [(ctx.d2h(q[1], np.empty_like(dy)), ctx.d2h(q[2], np.empty((F, B), np.float32, order="F"))) + self.grads(m) for m, (q, dy) in enumerate(zip(d, dys))]
        finally:
            [ctx.free(p) for p in [d_x] + [p for q in d for p in q]]

    def single(self, m, x, dy, F):
        """the same four arrays of member m from the single-member entries"""
        ctx, B, t, h = self.ctx, x.shape[1], self.t[m], self.heads[m].h
        d_x, d_f, d_dy, d_o, d_df = ctx.alloc(x.nbytes), ctx.alloc(4 * F * B), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(4 * F * B)
        try:
            ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
            ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, d_f)); ctx.check(ctx.lib.crux_mlp_forward_cached(h, d_f, B, d_o))
            ctx.check(ctx.lib.crux_mlp_backward(h, d_f, B, d_dy, 1.0, 1, d_df)); ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_df, 1.0, 1, None))
            return (ctx.d2h(d_o, np.empty_like(dy)), ctx.d2h(d_df, np.empty((F, B), np.float32, order="F"))) + self.grads(m)
        finally:
            [ctx.free(p) for p in (d_x, d_f, d_dy, d_o, d_df)]


@pytest.mark.parametrize("case,M", PASS_CASES, ids=["%s_M%d" % (CR.case_id(c), M) for c, M in PASS_CASES])
def test_grouped_passes_equal_single_passes_bit_for_bit(gpu_ctx, case, M):
    sp, B = case; F = CR.n_features(sp); dims, acts = [F, 24, 3], ["tanh", "identity"]; rng = np.random.default_rng(M)
    ins = [CR.case_inputs(case, seed=3 + m) for m in range(M)]; x = ins[0][1]
    phs = [R.perturbed_params(R.glorot_params(dims, rng), rng) for _ in range(M)]; dys = [np.asfortranarray(rng.normal(0, 1, (3, B)).astype(np.float32)) for _ in range(M)]
    ref = _Members(gpu_ctx, sp, dims, acts, [i[0] for i in ins], phs)      # the single passes run on handles of their own: the grouped pass finds workspaces and
    want = [ref.single(m, x, dys[m], F) for m in range(M)]                # gradient vectors that nothing has written
    got = _Members(gpu_ctx, sp, dims, acts, [i[0] for i in ins], phs).passes(x, dys, F)
    for m in range(M):
        for name, a, b in zip(("output", "d_dx of the head", "trunk gradient", "head gradient"), got[m], want[m]):
            assert np.array_equal(a, b), (m, name)
        assert np.any(want[m][2]) and np.any(want[m][1])


@pytest.mark.parametrize("kind", [ER.GAUSS, ER.CLASS])
def test_one_step_matches_float64(gpu_ctx, kind):
    ctx, M, B, sp, acts = gpu_ctx, 3, 9, CER.SPEC, CER.ACTS; F = CR.n_features(sp)
    pts, phs, x, y, w = CER.inputs(kind, M, B, seed=21); dims = CER.head_dims(4 if kind == ER.GAUSS else 3)
    r64, r32 = (CER.step_reference(kind, sp, dims, acts, pts, phs, x, y, w, t) for t in (np.float64, np.float32))
    # the gradients through _passes with the reference's seeds; the step below runs on fresh handles
    got = _Members(ctx, sp, dims, acts, pts, phs).passes(x, [np.asfortranarray(s.astype(np.float32)) for s in r64["seeds"]], F)
    tensors = []
    for m in range(M):
        o, df, gt, gh = got[m]
        tensors += [("m%d o" % m, o, r64["o"][m], r32["o"][m]), ("m%d dfeat" % m, df, r64["dfeat"][m], r32["dfeat"][m])]
        tensors += [("m%d %s" % (m, n), t, r64["g_trunk"][m][a:b], r32["g_trunk"][m][a:b]) for n, t, (a, b) in _flat_slices("trunk", gt, CR.layer_offsets(sp), [ly["cout"] for ly in sp["layers"]])]
        tensors += [("m%d %s" % (m, n), t, r64["g_head"][m][a:b], r32["g_head"][m][a:b]) for n, t, (a, b) in _flat_slices("head", gh, R.layer_offsets(dims), dims[1:])]
    _bound_check("ens %s" % kind, tensors)
    bound = lambda t64, t32: MM * max(R.rel_err(t32, t64), U) * np.abs(t64).max()      # noqa: E731
    # the step itself: info row, then the parameters after Adam's first update from the device's own gradients
    mem = _Members(ctx, sp, dims, acts, pts, phs); opt = crux.Adam(np.float32(ETA))
    for q, h in zip(mem.t, mem.heads):
        for hh in (q.p.h, h.h):
            ctx.check(ctx.lib.crux_adam_init(hh, opt.eta, opt.beta[0], opt.beta[1], opt.epsilon))
    raw = np.zeros(L.INFO_N + 2 * M, np.float32); d = [ctx.alloc(a.nbytes) for a in (x, y)] + ([ctx.alloc(w.nbytes)] if w is not None else [None])
    try:
        [ctx.h2d(p, a) for p, a in zip(d, (x, y, w)) if a is not None]
        ctx.check(ctx.lib.crux_conv_ensemble_step(*mem.arrs, M, L.ENS[kind], d[0], d[1], d[2], B, raw.ctypes.data_as(C.c_void_p)))
    finally:
        [ctx.free(p) for p in d if p is not None]
    # a member's loss moves by at most sum |dL_m/do| |do| (+ |do|^2), dL_m/do = M x its seed; the norms by the norm of the tensors' bounds; each + 4 u / 2 u of its value for
    # its own Float32 roundings, as test_gpu_conv.py allows the TD step's loss and norm
    bl, bn = [], []
    for m in range(M):
        bo = bound(r64["o"][m], r32["o"][m]); bl.append(float(np.abs(r64["seeds"][m]).sum()) * M * bo + bo * bo)
        bn.append(np.sqrt(sum(t.size * bound(t64, t32) ** 2 for n, t, t64, t32 in tensors if n.startswith("m%d " % m) and (" dW" in n or " db" in n))))
        assert abs(raw[L.INFO_N + m] - r64["losses"][m]) <= bl[m] + 4 * U * abs(r64["losses"][m])
        assert abs(raw[L.INFO_N + M + m] - r64["norms"][m]) <= bn[m] + 2 * U * r64["norms"][m]
    assert abs(raw[0] - r64["loss"]) <= float(np.mean(bl)) + 4 * U * abs(r64["loss"])
    assert abs(raw[1] - r64["grad_norm"]) <= float(np.sqrt(sum(b * b for b in bn))) + 2 * U * r64["grad_norm"]
    for m in range(M):
        gt, gh = mem.grads(m)      # the step's own gradients (its seeds are the device's Float32 ones): the update they define
        for name, p0, p1, g in (("trunk", pts[m], mem.t[m].p.get_params(), gt), ("head", phs[m], mem.heads[m].get(), gh)):
            small = CR.adam_small(p0, ETA); dlt = p1.astype(np.float64) - p0
            assert np.all(np.abs(dlt - CR.adam_first_step_delta(g, ETA)) <= small * ETA), (m, name)
            assert np.all(np.abs(dlt) <= ETA * (1 + small)) and CR.adam_sign_ok(p0, p1, g, ETA), (m, name)
            assert np.array_equal(p1, CR.adam_first_step_f32(p0, g, ETA)), (m, name)


def _blobs(n, seed):
    rng = np.random.default_rng(seed); X = rng.normal(0, 0.3, (12, 12, 1, n)).astype(np.float32); c = rng.integers(0, 3, n)
    for j, k in enumerate(c):
        X[6 * (k % 2) + 1:6 * (k % 2) + 5, 6 * (k // 2) + 1:6 * (k // 2) + 5, 0, j] += 1.0
    return X, np.asfortranarray(np.eye(3, dtype=np.float32)[:, c])


def _image_ensemble(ctx):
    ens = crux.DeepClassificationEnsemble(lambda: crux.Chain(crux.Conv((3, 3), 1, 4, "relu"), crux.flatten, crux.Dense(400, 3), input=(12, 12, 1)), 3, ctx=ctx)
    ens.attach_optimizer(crux.Adam(np.float32(1e-2))); return ens


def test_nan_pixel_closes_the_gate_for_every_handle(gpu_ctx):
    ens = _image_ensemble(gpu_ctx); X, Y = _blobs(16, 1); X[3, 4, 0, 5] = np.nan; before = [m.get_params() for m in ens.models]
    with pytest.raises(crux.CruxError) as e:
        ens.train_step(X, Y)
    assert e.value.code == L.ENAN
    for m, p in zip(ens.models, before):
        assert np.array_equal(m.get_params(), p) and m.n_params == 4 * 9 + 4 + 400 * 3 + 3      # trunk and head of every member, bit for bit


def test_public_interface_fit_call_and_refusals(gpu_ctx):
    ctx = gpu_ctx; ens, twin = _image_ensemble(ctx), _image_ensemble(ctx); X, Y = _blobs(64, 2); l0 = crux.training_loss(ens, X, Y)
    for a, b in zip(ens.models, twin.models):
        b.set_params(a.get_params())
    out = ens.fit(X, Y, batch_size=24, epochs=2, seed=5)      # 24 + 24 + 16: a short last minibatch
    assert out["epochs_run"] == 2 and out["batches_trained"] == 6 and crux.training_loss(ens, X, Y) < l0
    p = ens(X)
    assert p.shape == (3, 64) and np.abs(p.sum(0) - 1).max() <= 4 * U and np.array_equal(p, ens(X.reshape((144, 64), order="F")))
    assert len(crux.individual_forward(ens, X)) == 3 and crux.logpdf(ens, X, Y).shape == (1, 64)
    rng = np.random.default_rng(5); same = np.stack([rng.permutation(64) for _ in range(2)])
    twin.fit_with_permutations(X, Y, None, 24, same)
    for a, b in zip(ens.models, twin.models):
        assert np.array_equal(a.get_params(), b.get_params())
    conv = lambda cout=4, act="relu": crux.Chain(crux.Conv((3, 3), 1, cout, act), crux.flatten, crux.Dense(100 * cout, 3), input=(12, 12, 1))      # noqa: E731
    gens = {"wide head": lambda: conv(12), "conv table differs": iter([conv(), conv(act="tanh")]).__next__,
            "conv and MLP members mixed": iter([conv(), crux.Chain(crux.Dense(400, 3))]).__next__}
    for word, gen in gens.items():
        with pytest.raises(NotImplementedError) as e:
            crux.DeepClassificationEnsemble(gen, 2, ctx=ctx)
        assert word in str(e.value), (word, str(e.value))
