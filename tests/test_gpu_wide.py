"""Wide handles (crux_mlp_create_wide: a dimension above 1024, up to 4096) through the dense engine's C ABI against float64.

crux_mlp_forward_cached / crux_mlp_backward of every member of tests/wide_cases.py under the bound of tests/test_gpu_dense_grid.py, unchanged:
    max |T_gpu - T_f64| / max |T_f64|  <=  M_MARGIN x max(e32(T), u)
per tensor (y, dx, every layer's dW and db; grad_scale = 0.5). tests/test_wide_reference.py shows on the CPU that the engine's summation order stays inside the figure M_MARGIN
was derived from at these reduction lengths. relu members draw kink-free observations. Further: identical bits across two calls and across a regrowth of the workspace;
crux_mlp_create keeps its refusal of 1025 and crux_mlp_create_wide refuses 4097; crux_mlp_create_wide with narrow dimensions is crux_mlp_create; the accepting entries
(parameters, copy, polyak, the Adam state) work; and a sample of the other entries refuses a wide handle by name and leaves it unchanged."""
import ctypes as C

import numpy as np
import pytest

import dense_reference as R
from crux_jl_amd import _lib as L
from wide_cases import WIDE_CASES

pytestmark = pytest.mark.gpu
GSCALE = 0.5


class Handle:
    """a raw crux_mlp from crux_mlp_create_wide (the host mirror builds wide handles behind a conv trunk only)"""

    def __init__(self, ctx, dims, acts, seed=7, create="crux_mlp_create_wide"):
        self.ctx, self.dims = ctx, list(dims)
        d = (C.c_int32 * len(dims))(*dims); a = (C.c_int32 * len(acts))(*[L.ACT[x] for x in acts]); h = C.c_void_p()
        ctx.check(getattr(ctx.lib, create)(ctx.h, len(acts), d, a, 0, C.byref(h)))
        self.h = h; self.n = int(ctx.lib.crux_mlp_n_params(h))
        ctx.check(ctx.lib.crux_mlp_init_glorot(h, seed, 2, 0.0))

    def get(self):
        out = np.empty(self.n, np.float32); self.ctx.check(self.ctx.lib.crux_mlp_get_params(self.h, out.ctypes.data_as(C.c_void_p), self.n)); return out

    def set(self, p):
        p = np.ascontiguousarray(p, np.float32); self.ctx.check(self.ctx.lib.crux_mlp_set_params(self.h, p.ctypes.data_as(C.c_void_p), p.size))

    def grads(self):
        return self.ctx.d2h(self.ctx.lib.crux_mlp_grads_ptr(self.h), np.empty(self.n, np.float32))

    def adam(self):
        m, v, bp = np.empty(self.n, np.float32), np.empty(self.n, np.float32), np.empty(2, np.float64)
        self.ctx.check(self.ctx.lib.crux_adam_get_state(self.h, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p)))
        return m, v, bp

    def passes(self, x, dy, want_g=1):
        ctx, B = self.ctx, x.shape[1]
        d_x, d_dy, d_y, d_dx = ctx.alloc(x.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(dy.nbytes), ctx.alloc(x.nbytes)
        try:
            ctx.h2d(d_x, x); ctx.h2d(d_dy, dy)
            ctx.check(ctx.lib.crux_mlp_forward_cached(self.h, d_x, B, d_y))
            ctx.check(ctx.lib.crux_mlp_backward(self.h, d_x, B, d_dy, GSCALE, want_g, d_dx))
            return ctx.d2h(d_y, np.empty_like(dy)), ctx.d2h(d_dx, np.empty_like(x)), self.grads()
        finally:
            for d in (d_x, d_dy, d_y, d_dx):
                ctx.free(d)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self.ctx.lib.crux_mlp_destroy(self.h)
        except Exception:       # noqa: BLE001
            pass


def _inputs(p, dims, acts, B, rng):
    x = R.kink_free_inputs(p, dims, acts, B, rng) if "relu" in acts else np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    return x, np.asfortranarray(rng.normal(0, 1, (dims[-1], B)).astype(np.float32))


@pytest.mark.parametrize("case", WIDE_CASES, ids=R.case_id)
def test_wide_handle_matches_float64(gpu_ctx, case):
    dims, acts, B = case
    net = Handle(gpu_ctx, dims, acts); rng = np.random.default_rng(3)
    p = R.perturbed_params(net.get(), rng); net.set(p)
    x, dy = _inputs(p, dims, acts, B, rng)
    y, dx, g = net.passes(x, dy)
    y2, dx2, g2 = net.passes(x, dy)                                            # two calls: identical bits
    assert np.array_equal(y, y2) and np.array_equal(dx, dx2) and np.array_equal(g, g2)
    r64, r32 = R.chain_reference(p, dims, acts, x, dy, np.float64), R.chain_reference(p, dims, acts, x, dy, np.float32)
    tensors = [("y", y, r64["y"], r32["y"]), ("dx", dx, r64["dx"], r32["dx"])]
    for l, (wo, bo) in enumerate(R.layer_offsets(dims)):
        i, o = dims[l], dims[l + 1]
        tensors.append(("dW%d" % l, (g[wo:bo] / GSCALE).reshape((o, i), order="F"), r64["dW"][l], r32["dW"][l]))
        tensors.append(("db%d" % l, g[bo:bo + o] / GSCALE, r64["db"][l], r32["db"][l]))
    bad = []
    for name, t, t64, t32 in tensors:
        e32, eg = R.rel_err(t32, t64), R.rel_err(t, t64); ratio = eg / max(e32, R.U32)
        print("WIDE %s %s e32_u %.3f gpu_u %.3f ratio %.3f" % (R.case_id(case), name, e32 / R.U32, eg / R.U32, ratio))
        if not eg <= R.M_MARGIN * max(e32, R.U32):
            bad.append((name, "e32 %.2f u" % (e32 / R.U32), "gpu %.2f u" % (eg / R.U32), "ratio %.2f > M = %.2f" % (ratio, R.M_MARGIN)))
    assert not bad, bad


@pytest.mark.parametrize("case", [WIDE_CASES[1], WIDE_CASES[2]], ids=R.case_id)
def test_bits_survive_a_workspace_regrowth(gpu_ctx, case):
    """the workspace starts at 256 columns; B = 300 regrows it to 512 and every offset moves. The small batch afterwards, and a fresh handle, give the first call's bits"""
    dims, acts, B = case
    one = Handle(gpu_ctx, dims, acts); rng = np.random.default_rng(5)
    p = R.perturbed_params(one.get(), rng); one.set(p)
    x, dy = _inputs(p, dims, acts, B, rng); xb, dyb = _inputs(p, dims, acts, 300, np.random.default_rng(6))
    first = one.passes(x, dy); big = one.passes(xb, dyb); again = one.passes(x, dy)
    fresh = Handle(gpu_ctx, dims, acts); fresh.set(p); big_fresh = fresh.passes(xb, dyb)
    for name, a, b, c, d in zip(("y", "dx", "gradient"), first, again, big, big_fresh):
        assert np.array_equal(a, b) and np.array_equal(c, d), name


def test_create_limits_and_narrow_equivalence(gpu_ctx):
    ctx = gpu_ctx
    for create, dims, word in (("crux_mlp_create", [1025, 4], "dim 0 = 1025"), ("crux_mlp_create", [4, 1025], "dim 1 = 1025"), ("crux_mlp_create_wide", [4097, 4], "dim 0 = 4097"),
                               ("crux_mlp_create_wide", [4, 4097, 2], "dim 1 = 4097"), ("crux_mlp_create_wide", [0, 4], "dim 0 = 0")):
        d = (C.c_int32 * len(dims))(*dims); a = (C.c_int32 * (len(dims) - 1))(); h = C.c_void_p()
        rc = getattr(ctx.lib, create)(ctx.h, len(dims) - 1, d, a, 0, C.byref(h))
        assert rc == L.EINVAL and h.value is None and word in ctx.lib.crux_last_error(ctx.h).decode(), (create, dims)
    # every dimension <= 1024: crux_mlp_create exactly -- the same draws, and crux_mlp_forward (which refuses a wide handle) takes it
    a_, b_ = Handle(ctx, [8, 64, 3], ["tanh", "identity"]), Handle(ctx, [8, 64, 3], ["tanh", "identity"], create="crux_mlp_create")
    assert np.array_equal(a_.get(), b_.get())
    edge = Handle(ctx, [8, 1024, 4], ["tanh", "identity"])      # 1024 itself is not wide: an entry that refuses wide handles takes it
    ctx.check(ctx.lib.crux_mlp_set_sigma_head(edge.h, 1)); assert ctx.lib.crux_mlp_get_sigma_head(edge.h) == 1
    x = np.asfortranarray(np.random.default_rng(1).normal(0, 1, (8, 5)).astype(np.float32)); ys = []
    for net in (a_, b_):
        d_x, d_y = ctx.alloc(x.nbytes), ctx.alloc(4 * 3 * 5)
        try:
            ctx.h2d(d_x, x); ctx.check(ctx.lib.crux_mlp_forward(net.h, d_x, 5, d_y)); ys.append(ctx.d2h(d_y, np.empty((3, 5), np.float32, order="F")))
        finally:
            ctx.free(d_x); ctx.free(d_y)
    assert np.array_equal(ys[0], ys[1])


def test_accepting_entries_copy_polyak_adam_state(gpu_ctx):
    ctx = gpu_ctx; dims, acts = [1300, 40, 3], ["relu", "identity"]; rng = np.random.default_rng(9)
    a, b = Handle(ctx, dims, acts, seed=1), Handle(ctx, dims, acts, seed=2)
    pa, pb = a.get(), b.get()
    assert a.n == R.n_layer_params(dims) and np.any(pa != pb) and np.abs(pa[:1300 * 40]).max() <= np.sqrt(6.0 / 1340) and not pa[1300 * 40:1300 * 40 + 40].any()
    ctx.check(ctx.lib.crux_polyak(a.h, b.h, 0.25))
    want = (np.float32(0.25) * pb + (np.float32(1) - np.float32(0.25)) * pa).astype(np.float32)
    assert np.array_equal(a.get(), want) and np.array_equal(b.get(), pb)      # PolyakOp: two products and a sum, no contraction
    ctx.check(ctx.lib.crux_mlp_copy(a.h, b.h)); assert np.array_equal(a.get(), pb)
    ctx.check(ctx.lib.crux_adam_init(a.h, 1e-3, 0.9, 0.999, 1e-8)); m, v, bp = a.adam()
    assert not m.any() and not v.any() and np.array_equal(bp, [0.9, 0.999])
    m1 = rng.normal(0, 1, a.n).astype(np.float32); v1 = rng.random(a.n).astype(np.float32); bp1 = np.array([0.5, 0.25])
    ctx.check(ctx.lib.crux_adam_set_state(a.h, m1.ctypes.data_as(C.c_void_p), v1.ctypes.data_as(C.c_void_p), bp1.ctypes.data_as(C.c_void_p)))
    m, v, bp = a.adam(); assert np.array_equal(m, m1) and np.array_equal(v, v1) and np.array_equal(bp, bp1)
    dm, dv = C.c_void_p(), C.c_void_p(); ctx.check(ctx.lib.crux_adam_state_ptrs(a.h, C.byref(dm), C.byref(dv))); assert dm.value and dv.value
    ctx.check(ctx.lib.crux_adam_set_clip_value(a.h, 0.5)); assert ctx.lib.crux_adam_get_clip_value(a.h) == 0.5
    ctx.check(ctx.lib.crux_mlp_copy(b.h, a.h)); assert ctx.lib.crux_adam_get_clip_value(b.h) == 0.0      # copy moves parameters, not the optimiser's fields


def test_other_entries_refuse_a_wide_handle_by_name_and_leave_it_unchanged(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib
    net, twin = Handle(ctx, [2048, 256, 6], ["relu", "identity"], seed=3), Handle(ctx, [2048, 256, 6], ["relu", "identity"], seed=4)
    ctx.check(lib.crux_adam_init(net.h, 1e-3, 0.9, 0.999, 1e-8))
    x = np.asfortranarray(np.random.default_rng(2).normal(0, 1, (2048, 4)).astype(np.float32)); dy = np.ones((6, 4), np.float32, order="F")
    net.passes(x, dy)                                       # something in the gradient buffer
    before = (net.get(), net.grads()) + net.adam()
    d_x, d_y = ctx.alloc(x.nbytes), ctx.alloc(4 * 6 * 4); ctx.h2d(d_x, x)
    pair = (C.c_void_p * 2)(net.h, twin.h); it = (C.c_int32 * 2)(1, 0)
    calls = [("crux_rollout", lambda: lib.crux_rollout(None, net.h, None, None, 0, None, None)),
             ("crux_td_step", lambda: lib.crux_td_step(net.h, None, None, 0, None)),
             ("crux_td_step_with_error", lambda: lib.crux_td_step_with_error(net.h, None, None, 0, None, None)),
             ("crux_mlp_forward", lambda: lib.crux_mlp_forward(net.h, d_x, 4, d_y)),
             ("crux_ensemble_forward", lambda: lib.crux_ensemble_forward(pair, 2, L.ENS["class"], d_x, 4, None, None, d_y, None)),
             ("crux_dqn_target", lambda: lib.crux_dqn_target(net.h, None, 0.99, None)),
             ("crux_dqn_epochs", lambda: lib.crux_dqn_epochs(net.h, twin.h, None, None, 0.99, 0, 0.0, 0, 1, None)),
             ("crux_fill_gae", lambda: lib.crux_fill_gae(None, net.h, 0.95, 0.99)),
             ("crux_adam_apply", lambda: lib.crux_adam_apply(net.h, 1.0)),
             ("crux_mlp_set_sigma_head", lambda: lib.crux_mlp_set_sigma_head(net.h, 1)),
             ("crux_mlp_set_spectral", lambda: lib.crux_mlp_set_spectral(net.h, it, None, 0, 0))]
    try:
        for name, call in calls:
            rc = call(); msg = lib.crux_last_error(ctx.h).decode()
            assert rc == L.EUNSUP and name in msg and "wide handle" in msg, (name, rc, msg)
    finally:
        ctx.free(d_x); ctx.free(d_y)
    ctx.sync()
    for a, b in zip(before, (net.get(), net.grads()) + net.adam()):
        assert np.array_equal(a, b)
    assert lib.crux_mlp_get_sigma_head(net.h) == 0 and lib.crux_mlp_spectral_layers(net.h, None) == 0
