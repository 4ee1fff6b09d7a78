"""GPU: DeepEnsemble / DeepClassificationEnsemble (csrc/ensemble.hip on the member-grouped passes of csrc/dense.hip) against the float64 yardstick of
tests/ensemble_reference.py.

Parameters and data of every case come from numpy (`ER.case`), so each case also runs through the yardstick alone (tests/test_ensemble_reference.py).
Shapes: 3-12-2 relu (sub-tile), 5-100-100-4 tanh and 4-100-100-3 tanh (no multiple of 16: a member's last partial tile must not reach into its neighbour),
4-256-256-2 relu and 6-300-6 relu (K >= 128: the split-K tiles); nd = 1, 2, 3 and three classes; M 1, 3, 5 (16 once); B 1, 37, 256.
Tolerances (those of tests/test_gpu_sn.py, test_gpu_advil.py, test_gpu_cql.py): 1e-4 relative on the members' mu, var, p, the mixture mean, losses and norms, 1e-4
of the gradient scale on gradients, 2e-5 absolute on parameters after one Adam step at lr 1e-3. Parameters whose float64 gradient lies within 1e-3 of the gradient
scale of zero are not compared (the first Adam step is lr sign(g) there); at most a quarter may be left out per member. Largest share left out over the step cases,
measured with the yardstick alone (test_ensemble_reference.py::test_adam_comparison_leaves_out_at_most_a_quarter): 19.7 % (4-256-256-2, M = 3, B = 256, weights).
var* = mean(var + mu^2) - mu*^2 cancels in Float32, so var* and the ensemble logpdf have a tolerance of their own: four times the largest absolute error of a
float32 numpy restatement in the reference's operand order against float64 on the same inputs (`ER.mixture_tolerance`, per shape over its M x B grid; the margin
covers the tile GEMMs' other summation order). Measured float32 error var* / logpdf -> tolerance:
    3-12-2       8.9e-07 / 1.29e-06 -> 3.56e-06 / 5.15e-06        5-100-100-4  6.36e-07 / 5.33e-06 -> 2.54e-06 / 2.13e-05
    4-256-256-2  8.74e-07 / 4.82e-06 -> 3.49e-06 / 1.93e-05       6-300-6      7.33e-07 / 5.93e-06 -> 2.93e-06 / 2.37e-05
    4-100-100-3  (no var*) / 3.63e-07 -> 1.45e-06
The inputs keep |mu*| of order one and var* >= 0.05 (asserted there).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ensemble_reference as ER

pytestmark = pytest.mark.gpu

LR = 1e-3
STEP_SKIPPED_MAX = 0.25
GRID = [(n, M, B) for n in ER.SHAPES for M in ER.MS for B in ER.BS]
# (shape, M, B, weighted): both kinds, with and without weights, every shape, M = 1 and 16 once
STEP_CASES = [("3-12-2", 3, 37, True), ("3-12-2", 5, 256, False), ("3-12-2", 16, 37, True), ("5-100-100-4", 3, 37, True), ("5-100-100-4", 5, 256, False),
              ("4-256-256-2", 3, 256, True), ("4-256-256-2", 1, 37, False), ("6-300-6", 3, 37, True), ("6-300-6", 5, 256, False),
              ("4-100-100-3", 3, 37, False), ("4-100-100-3", 5, 256, True)]


def _crux():
    from parity import crux
    return crux


def _L():
    from parity import L
    return L


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rel(a, b, tol=1e-4):
    return np.abs(np.asarray(a, np.float64) - b).max() <= tol * max(1.0, np.abs(b).max())


@functools.lru_cache(maxsize=None)
def _mixture_tol(name):
    return ER.mixture_tolerance(name)


class Ens:
    """M ContinuousNetwork handles with the case's parameters, and the pointer array the entries take"""

    def __init__(self, ctx, c, ps=None, lr=LR, adam=True):
        crux = _crux(); self.ctx, self.c = ctx, c
        ch = lambda: crux.Chain(*[crux.Dense(c["dims"][l], c["dims"][l + 1], a) for l, a in enumerate(c["acts"])])      # noqa: E731
        self.nets = [crux.ContinuousNetwork(ch(), ctx=ctx) for _ in (ps or c["ps"])]
        for n, p in zip(self.nets, ps or c["ps"]):
            n.set_params(p)
            if adam:
                n.attach_optimizer(crux.Adam(np.float32(lr)))
        self.M = len(self.nets); self.arr = (C.c_void_p * self.M)(*[n.h.value for n in self.nets]); self.kind = _L().ENS[c["kind"]]

    def grads(self):
        return [self.ctx.d2h(self.ctx.lib.crux_mlp_grads_ptr(n.h), np.empty(n.n_params, np.float32)) for n in self.nets]

    def state(self):
        return [a for n in self.nets for a in (n.get_params(),) + tuple(n.adam_state())]


class Dev:
    """device buffers freed at the end of a test"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        a = np.asfortranarray(a); p = self.ctx.alloc(max(a.nbytes, 4)); self.ptrs.append(p); self.ctx.h2d(p, a); return p

    def empty(self, nfloats):
        p = self.ctx.alloc(4 * max(int(nfloats), 1)); self.ptrs.append(p); return p

    def down(self, p, shape):
        return self.ctx.d2h(p, np.empty(shape, np.float32, order="F"))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.ctx.free(p)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- 1. the grouped passes are the per-handle passes, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,B", GRID + [("3-12-2", 16, 37)])
def test_grouped_passes_equal_the_per_handle_passes(gpu_ctx, name, M, B):
    ctx, lib, c = gpu_ctx, gpu_ctx.lib, ER.case(name, M, B); nout = c["dims"][-1]
    one, grp = Ens(ctx, c, adam=False), Ens(ctx, c, adam=False)
    with Dev(ctx) as d:
        dx = d.up(c["x"]); ddy = [d.up(dy) for dy in c["dys"]]; dout = [d.empty(nout * B) for _ in range(M)]; dy1 = d.empty(nout * B)
        outs = []
        for n, dd in zip(one.nets, ddy):
            ctx.check(lib.crux_mlp_forward_cached(n.h, dx, B, dy1)); outs.append(d.down(dy1, (nout, B)))
            ctx.check(lib.crux_mlp_backward(n.h, dx, B, dd, 1.0, 1, None))
        ctx.check(lib.crux_ensemble_passes(grp.arr, M, dx, B, (C.c_void_p * M)(*[p.value for p in ddy]), (C.c_void_p * M)(*[p.value for p in dout])))
        gouts = [d.down(p, (nout, B)) for p in dout]
    for m in range(M):
        assert np.array_equal(_bits(outs[m]), _bits(gouts[m])), (name, M, B, m)
        assert np.isfinite(outs[m]).all() and _rel(outs[m], ER.forward(c["ps"][m], c["dims"], c["acts"], c["x"])[0])
    for m, (a, b) in enumerate(zip(one.grads(), grp.grads())):
        assert np.array_equal(_bits(a), _bits(b)) and np.isfinite(a).all() and np.abs(a).max() > 0, (name, M, B, m)
    _same([n.get_params() for n in grp.nets], c["ps"])      # the passes train nothing


# ---- 2. forward and logpdf against the yardstick -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,B", GRID)
def test_forward_and_logpdf_match_reference(gpu_ctx, name, M, B):
    ctx, lib, c = gpu_ctx, gpu_ctx.lib, ER.case(name, M, B); kind = c["kind"]; ny = c["y"].shape[0]; n = ny * B
    e = Ens(ctx, c, adam=False); tv, tl = _mixture_tol(name)
    os = [ER.forward(p, c["dims"], c["acts"], c["x"])[0] for p in c["ps"]]
    a_ref, b_ref = ER.members(kind, os); mean_ref, evar_ref = ER.mixture(kind, os); lp_ref = ER.logpdf(kind, os, c["y"])
    with Dev(ctx) as d:
        dx, dy = d.up(c["x"]), d.up(c["y"]); dmu, dvar, dmean, devar, dlp = d.empty(M * n), d.empty(M * n), d.empty(n), d.empty(n), d.empty(lp_ref.size)
        ctx.check(lib.crux_ensemble_forward(e.arr, M, e.kind, dx, B, dmu, dvar, dmean, devar))
        mu, mean = d.down(dmu, (n, M)), d.down(dmean, (ny, B))
        ctx.check(lib.crux_ensemble_logpdf(e.arr, M, e.kind, dx, dy, B, dlp)); lp = d.down(dlp, lp_ref.shape)
        for m in range(M):
            assert _rel(mu[:, m].reshape((ny, B), order="F"), a_ref[m]), (name, M, B, m)
        assert _rel(mean, mean_ref)
        if kind == ER.GAUSS:
            var, evar = d.down(dvar, (n, M)), d.down(devar, (ny, B))
            for m in range(M):
                assert _rel(var[:, m].reshape((ny, B), order="F"), b_ref[m])
            print("var* error %.3g (tolerance %.3g)" % (np.abs(evar - evar_ref).max(), tv))
            assert np.abs(evar - evar_ref).max() <= tv
        else:
            assert np.abs(mean.sum(0) - 1).max() < 1e-6
        print("logpdf error %.3g (tolerance %.3g)" % (np.abs(lp - lp_ref).max(), tl))
        assert np.abs(lp - lp_ref).max() <= tl


# ---- 3. one step against the yardstick -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,B,weighted", STEP_CASES)
def test_step_matches_reference(gpu_ctx, name, M, B, weighted):
    L = _L(); ctx, lib, c = gpu_ctx, gpu_ctx.lib, ER.case(name, M, B); w = c["w"] if weighted else None
    info_r, gs, new = ER.step(c["ps"], [ER.Adam64(len(p), lr=LR) for p in c["ps"]], c["dims"], c["acts"], c["kind"], c["x"], c["y"], w)
    e = Ens(ctx, c); raw = np.zeros(L.INFO_N + 2 * M, np.float32)
    with Dev(ctx) as d:
        ctx.check(lib.crux_ensemble_step(e.arr, M, e.kind, d.up(c["x"]), d.up(c["y"]), d.up(c["w"]) if weighted else None, B, _vp(raw)))
    print("loss %.7g (ref %.7g) norm %.7g (ref %.7g)" % (raw[0], info_r["loss"], raw[1], info_r["grad_norm"]))
    close = lambda a, b: abs(a - b) <= 1e-4 * max(1.0, abs(b))      # noqa: E731
    assert close(raw[L.INFO["loss"]], info_r["loss"]) and close(raw[L.INFO["grad_norm"]], info_r["grad_norm"])
    for m in range(M):
        assert close(raw[L.INFO_N + m], info_r["losses"][m]) and close(raw[L.INFO_N + M + m], info_r["norms"][m]), m
    worst_share, worst_err = 0.0, 0.0
    for m, (g, gr, n, want) in enumerate(zip(e.grads(), gs, e.nets, new)):
        assert np.abs(g - gr).max() <= 1e-4 * np.abs(gr).max(), (m, np.abs(g - gr).max(), np.abs(gr).max())
        ok = np.abs(gr) > 1e-3 * np.abs(gr).max(); got = n.get_params()
        worst_share = max(worst_share, 1.0 - ok.mean()); worst_err = max(worst_err, np.abs(got[ok] - want[ok]).max())
        assert np.isfinite(got).all()
    print("  entries not compared: %.2f %%; worst parameter error %.3g" % (100 * worst_share, worst_err))
    assert worst_share <= STEP_SKIPPED_MAX and worst_err < 2e-5


def test_classification_step_ignores_the_weights(gpu_ctx):
    L = _L(); c = ER.case("4-100-100-3", 3, 37); out = []
    for w in (None, 5.0 * c["w"]):
        e = Ens(gpu_ctx, c); raw = np.zeros(L.INFO_N + 6, np.float32)
        with Dev(gpu_ctx) as d:
            gpu_ctx.check(gpu_ctx.lib.crux_ensemble_step(e.arr, 3, e.kind, d.up(c["x"]), d.up(c["y"]), d.up(w) if w is not None else None, 37, _vp(raw)))
        out.append(e.state() + [raw])
    _same(out[0], out[1])


# ---- 4. the chain is its steps -------------------------------------------------------------------------------------------------------------------------------------------
def _train(e, c, perms, batch, max_batches, W):
    L = _L(); M = e.M; epochs, N = perms.shape; stride = L.INFO_N + 2 * M
    raw, rows = np.zeros(stride, np.float32), np.zeros((epochs, stride), np.float32)
    with Dev(e.ctx) as d:
        rc = e.ctx.lib.crux_ensemble_train(e.arr, M, e.kind, d.up(c["x"]), d.up(c["y"]), d.up(W) if W is not None else None, N, batch, epochs, max_batches, _vp(perms), _vp(raw), _vp(rows))
    return rc, raw, rows


@pytest.mark.parametrize("name,weighted", [("3-12-2", True), ("5-100-100-4", False), ("4-100-100-3", False)])
def test_train_equals_the_steps_one_by_one(gpu_ctx, name, weighted):
    L = _L(); ctx, M, N, batch, epochs = gpu_ctx, 3, 300, 128, 2
    c = ER.case(name, M, N); W = c["w"] if weighted else None
    perms = np.ascontiguousarray(np.stack([np.random.default_rng(40 + k).permutation(N) for k in range(epochs)]), np.int64)
    for max_batches in (0, 3):
        mbs = ER.minibatches(N, batch, epochs, perms, max_batches or None)
        assert [len(i) for _, i in mbs] == ([128, 128, 44] * 2 if not max_batches else [128, 128, 44])
        chain, chain2, steps = Ens(ctx, c), Ens(ctx, c), Ens(ctx, c)
        rc, raw, rows = _train(chain, c, perms, batch, max_batches, W); ctx.check(rc)
        rc2, raw2, rows2 = _train(chain2, c, perms, batch, max_batches, W); ctx.check(rc2)
        want_rows = {}
        for ep, idx in mbs:
            r = np.zeros(L.INFO_N + 2 * M, np.float32)
            with Dev(ctx) as d:
                ctx.check(ctx.lib.crux_ensemble_step(steps.arr, M, steps.kind, d.up(c["x"][:, idx]), d.up(c["y"][:, idx]), d.up(W[:, idx]) if weighted else None, len(idx), _vp(r)))
            want_rows[ep] = r
        n_run = len(want_rows)
        _same(chain.state(), steps.state()); _same(chain.state() + [raw, rows], chain2.state() + [raw2, rows2])
        assert raw[L.INFO["batches_trained"]] == len(mbs) and raw[L.INFO["epochs_run"]] == n_run and n_run == (2 if not max_batches else 1)
        for ep in range(n_run):
            assert rows[ep].tobytes() == want_rows[ep].tobytes()
        keep = [k for k in range(L.INFO_N + 2 * M) if k not in (L.INFO["batches_trained"], L.INFO["epochs_run"])]
        assert raw[keep].tobytes() == want_rows[n_run - 1][keep].tobytes()
        assert np.isfinite(chain.nets[0].get_params()).all() and not np.array_equal(chain.nets[0].get_params(), c["ps"][0])
        if not max_batches:      # and the yardstick's fit over the same permutations
            ps, _ = ER.fit(c["ps"], c["dims"], c["acts"], c["kind"], c["x"], c["y"], W, batch, epochs, perms, lr=LR)
            assert all(np.abs(n.get_params() - p).max() < 6 * 2e-5 for n, p in zip(chain.nets, ps))      # six steps of at most lr each: 2e-5 per step


# ---- 5. the NaN gate -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3-12-2", "4-100-100-3"])
def test_a_nan_in_y_updates_no_member(gpu_ctx, name):
    L = _L(); ctx, lib, M, B = gpu_ctx, gpu_ctx.lib, 3, 37
    c = ER.case(name, M, B); y = c["y"].copy(); y[0, 5] = np.nan
    e = Ens(ctx, c); before = e.state(); raw = np.zeros(L.INFO_N + 2 * M, np.float32)
    with Dev(ctx) as d:
        rc = lib.crux_ensemble_step(e.arr, M, e.kind, d.up(c["x"]), d.up(y), None, B, _vp(raw))
    assert rc == L.ENAN and "NaN detected!" in (lib.crux_last_error(ctx.h) or b"").decode()
    assert np.isnan(raw[L.INFO["grad_norm"]])
    _same(e.state(), before)
    perms = np.arange(B, dtype=np.int64).reshape(1, B)      # the chain: the same verdict, nothing updated
    rc, raw2, _ = _train(e, dict(c, y=y), perms, 16, 0, None)
    assert rc == L.ENAN; _same(e.state(), before)
    fresh = Ens(ctx, c); clean = Ens(ctx, c); r1, r2 = np.zeros_like(raw), np.zeros_like(raw)      # a following clean step is unaffected
    with Dev(ctx) as d:
        ctx.check(lib.crux_ensemble_step(fresh.arr, M, fresh.kind, d.up(c["x"]), d.up(c["y"]), None, B, _vp(r1)))
        ctx.check(lib.crux_ensemble_step(e.arr, M, e.kind, d.up(c["x"]), d.up(c["y"]), None, B, _vp(r2)))
    _same(fresh.state() + [r1], e.state() + [r2])
    assert np.isfinite(r1[:2]).all() and not np.array_equal(fresh.nets[0].get_params(), clean.nets[0].get_params())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_parameters_untouched(gpu_ctx):
    L = _L(); crux = _crux(); ctx, lib, B = gpu_ctx, gpu_ctx.lib, 8
    c = ER.case("3-12-2", 3, B); e = Ens(ctx, c); raw = np.zeros(L.INFO_N + 40, np.float32)
    err = lambda: (lib.crux_last_error(ctx.h) or b"").decode()      # noqa: E731
    with Dev(ctx) as d:
        dx, dy, dm, dv = d.up(c["x"]), d.up(c["y"]), d.empty(B), d.empty(B)
        step = lambda arr, M, kind=e.kind: lib.crux_ensemble_step(arr, M, kind, dx, dy, None, B, _vp(raw))      # noqa: E731
        many = Ens(ctx, ER.case("3-12-2", 16, B)); arr17 = (C.c_void_p * 17)(*([n.h.value for n in many.nets] + [e.nets[0].h.value]))
        assert step(arr17, 17) == L.EINVAL and "17 members" in err()
        wide = Ens(ctx, ER.case("5-100-100-4", 1, B)); other = ER.case("3-12-2", 1, B)
        other["dims"], other["ps"] = (3, 13, 2), [np.zeros(3 * 13 + 13 + 13 * 2 + 2, np.float32)]
        o13 = Ens(ctx, other)
        for bad in (wide, o13):
            assert step((C.c_void_p * 2)(e.nets[0].h.value, bad.nets[0].h.value), 2) == L.EINVAL and "differs from member 0" in err()
        assert step((C.c_void_p * 2)(e.nets[0].h.value, e.nets[0].h.value), 2) == L.EINVAL and "one handle" in err()
        odd = Ens(ctx, dict(ER.case("4-100-100-3", 2, B), kind=ER.GAUSS))
        assert lib.crux_ensemble_forward(odd.arr, 2, L.ENS["gauss"], dx, B, None, None, dm, dv) == L.EINVAL and "even output width" in err()
        sn = crux.ContinuousNetwork(crux.Chain(crux.DenseSN(3, 12, "relu"), crux.Dense(12, 2)), ctx=ctx); sn.attach_optimizer(crux.Adam(np.float32(LR)))
        assert step((C.c_void_p * 2)(e.nets[0].h.value, sn.h.value), 2) == L.EUNSUP and "spectrally normalised" in err()
        noadam = Ens(ctx, c, adam=False)
        assert step(noadam.arr, 3) == L.EINVAL and "crux_adam_init" in err()
        assert lib.crux_ensemble_step(e.arr, 3, e.kind, dx, dy, None, 0, _vp(raw)) == L.EINVAL and lib.crux_ensemble_step(e.arr, 3, e.kind, dx, dy, None, (1 << 20) + 1, _vp(raw)) == L.EINVAL
        assert lib.crux_ensemble_forward_recording(e.arr, 3, e.kind, dx, B, dm, dv) == L.EUNSUP and "not recordable" in err()
        assert lib.crux_ensemble_forward(e.arr, 3, e.kind, dx, B, None, None, dm, dv) == 0      # and the context records nothing afterwards
        bad_perm = np.full((1, B), B, np.int64)
        assert _train(e, c, bad_perm, 4, 0, None)[0] == L.EINVAL and "permutation entry" in err()
    for ens in (e, many, wide, o13, odd, noadam):
        _same([n.get_params() for n in ens.nets], ens.c["ps"])
    with pytest.raises(NotImplementedError):
        crux.DeepEnsemble(lambda: crux.Chain(crux.Dense(3, 12, "relu"), crux.Dense(12, 2)), 17, ctx=ctx)
    with pytest.raises(NotImplementedError):
        crux.DeepEnsemble(lambda: crux.Chain(crux.DenseSN(3, 12, "relu"), crux.Dense(12, 2)), 2, ctx=ctx)
    widths = iter([12, 13])
    with pytest.raises(NotImplementedError):
        crux.DeepEnsemble(lambda: (lambda h: crux.Chain(crux.Dense(3, h, "relu"), crux.Dense(h, 2)))(next(widths)), 2, ctx=ctx)


# ---- 7. the host mirror ----------------------------------------------------------------------------------------------------------------------------------------------------
def _mirror(ctx, c, cls):
    crux = _crux()
    ens = cls(lambda: crux.Chain(*[crux.Dense(c["dims"][l], c["dims"][l + 1], a) for l, a in enumerate(c["acts"])]), c["M"], ctx=ctx)
    assert len({m.get_params().tobytes() for m in ens.models}) == c["M"]      # independent Glorot streams
    for m, p in zip(ens.models, c["ps"]):
        m.set_params(p)
    return ens


@pytest.mark.parametrize("name", ["3-12-2", "4-100-100-3"])
def test_host_mirror_matches_reference(gpu_ctx, name):
    crux = _crux(); M, N = 3, 300; c = ER.case(name, M, N); kind = c["kind"]; dims, acts = c["dims"], c["acts"]
    cls = crux.DeepEnsemble if kind == ER.GAUSS else crux.DeepClassificationEnsemble
    ens = _mirror(gpu_ctx, c, cls); x, y, w = c["x"][:, :37], c["y"][:, :37], c["w"][:, :37]
    os = [ER.forward(p, dims, acts, x)[0] for p in c["ps"]]; a_ref, b_ref = ER.members(kind, os); mean_ref, evar_ref = ER.mixture(kind, os); tv, tl = _mixture_tol(name)
    if kind == ER.GAUSS:
        mean, evar = ens(x); mus, vars_ = crux.individual_forward(ens, x)
        assert _rel(mean, mean_ref) and np.abs(evar - evar_ref).max() <= tv and all(_rel(a, b) for a, b in zip(mus, a_ref)) and all(_rel(a, b) for a, b in zip(vars_, b_ref))
    else:
        assert _rel(ens(x), mean_ref) and all(_rel(a, b) for a, b in zip(crux.individual_forward(ens, x), a_ref))
    assert np.abs(crux.logpdf(ens, x, y) - ER.logpdf(kind, os, y)).max() <= tl
    for wt in (None, w):
        lr_ = ER.training_loss(kind, os, y, wt); assert abs(crux.training_loss(ens, x, y, wt) - lr_) <= 1e-4 * max(1.0, abs(lr_))
    _same([m.get_params() for m in ens.models], c["ps"])      # training_loss updates nothing
    with pytest.raises(ValueError):
        ens.train_step(x, y)
    ens.attach_optimizer(crux.Adam(np.float32(LR)))
    info_r, gs, new = ER.step(c["ps"], [ER.Adam64(len(p), lr=LR) for p in c["ps"]], dims, acts, kind, x, y, w)
    info = ens.train_step(x, y, w)
    assert abs(info["loss"] - info_r["loss"]) <= 1e-4 * max(1.0, abs(info_r["loss"])) and _rel(info["member_losses"], np.array(info_r["losses"])) and _rel(info["member_grad_norms"], np.array(info_r["norms"]))
    for m, gr, want in zip(ens.models, gs, new):
        ok = np.abs(gr) > 1e-3 * np.abs(gr).max(); assert np.abs(m.get_params()[ok] - want[ok]).max() < 2e-5
    outs = []
    for _ in range(2):      # fit: reproducible bit for bit, and the yardstick over the same permutations
        e2 = _mirror(gpu_ctx, c, cls); e2.attach_optimizer(crux.Adam(np.float32(LR)))
        h = e2.fit(c["x"], c["y"], batch_size=128, epochs=2, weights=c["w"], seed=7)
        outs.append([m.get_params() for m in e2.models] + [np.array([r["loss"] for r in h["epochs"]], np.float32)])
        assert h["batches_trained"] == 6 and h["epochs_run"] == 2 and len(h["epochs"]) == 2
    _same(outs[0], outs[1])
    rng = np.random.default_rng(7); perms = [rng.permutation(N) for _ in range(2)]
    ps, rows = ER.fit(c["ps"], dims, acts, kind, c["x"], c["y"], c["w"], 128, 2, perms, lr=LR)
    assert all(np.abs(a - b).max() < 6 * 2e-5 for a, b in zip(outs[0][:M], ps)) and _rel(outs[0][M], np.array([r["loss"] for r in rows]))
    h3 = e2.fit(c["x"], c["y"], batch_size=128, epochs=2, seed=7, max_batches=3)
    assert h3["batches_trained"] == 3 and h3["epochs_run"] == 1
