"""GPU: MixtureNetwork (csrc/mixture.hip on the member-grouped passes of csrc/dense.hip) against the float64 yardstick of tests/mixture_reference.py.

Parameters and data of every case come from numpy (`MR.case`), so each case also runs through the yardstick alone (tests/test_mixture_reference.py).
Shapes: 2-32-1 relu with a 2-32-K weight network (the reference's DeepGMM, nd = 1), 5-100-100-3 tanh with constant weights (no multiple of 16, nd = 3), 4-256-256-2 relu
with a 4-64-K weight network (K >= 128: the split-K tiles, nd = 2); K 1, 3, 5 (16 once); B 1, 37, 257 (a lone column, an odd tail, one past a 256-thread block and past
four head blocks of 64), and one step at B = 4200, past the head's 64 blocks of 64 columns.
Tolerances (those of tests/test_gpu_ensemble.py, test_gpu_sn.py, test_gpu_advil.py): 1e-4 relative on alpha, the components' mu, the loss and the norms, 1e-4 of the
gradient scale on gradients, 2e-5 absolute on parameters after one Adam step at lr 1e-3. Parameters whose float64 gradient lies within 1e-3 of the gradient scale of zero
are not compared (the first Adam step is lr sign(g) there); at most a quarter may be left out per handle. Largest share left out over the step cases, measured with the
yardstick alone (test_mixture_reference.py::test_adam_comparison_leaves_out_at_most_a_quarter): 14.7 % (4-256-256-2, K = 5, B = 37, component 1).
lp has a tolerance of its own per shape: four times the largest absolute error of a float32 numpy restatement against float64 over the shape's K x B grid
(`MR.mixture_tolerance`, the rule of `ER.mixture_tolerance`; the margin covers the tile GEMMs' other summation order). Float32 error -> tolerance; largest error measured
on the device:
    2-32-1       5.56e-07 -> 2.22e-06;  device 7.69e-07
    5-100-100-3  2.69e-06 -> 1.08e-05;  device 1.74e-06
    4-256-256-2  3.07e-06 -> 1.23e-05;  device 9.55e-07
Learning (test_fit_learns_the_bimodal_target): 60 epochs of 32 minibatches at lr 3e-3 take the held-out NLL from 1.6617 to 1.1933 with K = 2 and from
1.6618 to 1.6174 with K = 1; the held-out sample's single-Gaussian optimum is 1.6169 (fitted: 0.49 N(0.99, 0.20) + 0.51 N(-1.03, 0.97)).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ensemble_reference as ER
import mixture_reference as MR

pytestmark = pytest.mark.gpu

LR = 1e-3
STEP_SKIPPED_MAX = 0.25
GRID = [(n, K, B) for n in MR.SHAPES for K in MR.KS for B in MR.BS]


def _crux():
    from parity import crux
    return crux


def _L():
    from parity import L
    return L


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _rel(a, b, tol=1e-4):
    return np.abs(np.asarray(a, np.float64) - b).max() <= tol * max(1.0, np.abs(b).max())


def _chain(dims, acts):
    crux = _crux()
    return crux.Chain(*[crux.Dense(dims[l], dims[l + 1], a) for l, a in enumerate(acts)])


@functools.lru_cache(maxsize=None)
def _lp_tol(name):
    return MR.mixture_tolerance(name)


@functools.lru_cache(maxsize=None)
def _case(name, K, B):
    """a case is computed once and shared; nobody writes into it"""
    return MR.case(name, K, B)


class Mix:
    """K GaussianPolicy handles and the weight handle (a ContinuousNetwork, or a ParamVector for constant weights) with the case's parameters, and what the entries take"""

    def __init__(self, ctx, c, lr=LR, adam=True, squashed=False):
        crux = _crux(); self.ctx, self.c, nd = ctx, c, c["nd"]
        mk = (lambda: crux.SquashedGaussianPolicy(_chain(c["dims"], c["acts"]), np.zeros(nd, np.float32), 1.0, ctx=ctx)) if squashed else \
             (lambda: crux.GaussianPolicy(_chain(c["dims"], c["acts"]), np.zeros(nd, np.float32), ctx=ctx))
        self.nets = [mk() for _ in c["ps"]]
        self.w = crux.ParamVector(c["wp"], ctx=ctx) if c["wdims"] is None else crux.ContinuousNetwork(_chain(c["wdims"], c["wacts"]), ctx=ctx)
        for n, p in zip(self.handles, self.vectors):
            n.set_params(p)
            if adam:
                n.attach_optimizer(crux.Adam(np.float32(lr)))
        self.K = len(self.nets); self.arr = (C.c_void_p * self.K)(*[n.h.value for n in self.nets])

    @property
    def handles(self):
        return self.nets + [self.w]

    @property
    def vectors(self):
        return list(self.c["ps"]) + [self.c["wp"]]

    def grads(self):
        return [self.ctx.d2h(self.ctx.lib.crux_mlp_grads_ptr(n.h), np.empty(n.n_params, np.float32)) for n in self.handles]

    def params(self):
        return [n.get_params() for n in self.handles]

    def state(self):
        return [a for n in self.handles for a in (n.get_params(),) + tuple(n.adam_state())]


class Dev:
    """device buffers freed at the end of a test"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        a = np.asfortranarray(a); p = self.ctx.alloc(max(a.nbytes, 4)); self.ptrs.append(p); self.ctx.h2d(p, a); return p

    def empty(self, nfloats):
        p = self.ctx.alloc(4 * max(int(nfloats), 1)); self.ptrs.append(p); return p

    def down(self, p, shape, dtype=np.float32):
        return self.ctx.d2h(p, np.empty(shape, dtype, order="F"))

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


def _step(m, s, a, w, B, raw):
    with Dev(m.ctx) as d:
        return m.ctx.lib.crux_mixture_step(m.arr, m.K, m.w.h, d.up(s), d.up(a), d.up(w) if w is not None else None, B, _vp(raw))


# ---- 1. forward: alpha, the components' mu and lp against the yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,B", GRID + [("2-32-1", 16, 37)])
def test_weights_means_and_logpdf_match_reference(gpu_ctx, name, K, B):
    ctx, lib, c = gpu_ctx, gpu_ctx.lib, _case(name, K, B); nd = c["nd"]; m = Mix(ctx, c, adam=False); tol = _lp_tol(name)
    al_ref = MR.alphas(c, c["s"]); mu_ref = [ER.forward(p[:-nd], c["dims"], c["acts"], c["s"])[0] for p in c["ps"]]; lp_ref = MR.logpdf(c)
    with Dev(ctx) as d:
        ds, da, dal, dmu, dlp = d.up(c["s"]), d.up(c["a"]), d.empty(K * B), d.empty(K * nd * B), d.empty(B)
        ctx.check(lib.crux_mixture_weights(m.arr, K, m.w.h, ds, B, dal, dmu)); al = d.down(dal, (K, B)); mu = d.down(dmu, (nd * B, K))
        ctx.check(lib.crux_mixture_logpdf(m.arr, K, m.w.h, ds, da, B, dlp)); lp = d.down(dlp, (B,))
        ctx.check(lib.crux_mixture_weights(m.arr, K, m.w.h, ds, B, dal, None)); _same([al], [d.down(dal, (K, B))])      # without the components' pass: the same bits
    assert _rel(al, al_ref)
    if c["wdims"] is not None:
        assert np.abs(al.sum(0) - 1).max() < 1e-6
    else:
        _same([al], [np.repeat(c["wp"][:, None], B, 1)])      # raw, not renormalised
    for k in range(K):
        assert _rel(mu[:, k].reshape((nd, B), order="F"), mu_ref[k]), (name, K, B, k)
    print("lp error %.3g (tolerance %.3g)" % (np.abs(lp - lp_ref).max(), tol))
    assert np.isfinite(lp).all() and np.abs(lp - lp_ref).max() <= tol
    _same(m.params(), m.vectors)      # the forward entries train nothing


# ---- 2. where the naive formula underflows --------------------------------------------------------------------------------------------------------------------------------
def test_logpdf_and_step_survive_thirty_sigma(gpu_ctx):
    L = _L(); ctx, K, B = gpu_ctx, 2, 37; c = _case("2-32-1", K, B); far = MR.far_actions(c)
    l, _ = MR.component_logpdfs(c, c["s"], far); assert (l < -200).all()
    m = Mix(ctx, c); lp_ref = MR.logpdf(c, a=far)
    with Dev(ctx) as d:
        dlp = d.empty(B); ctx.check(ctx.lib.crux_mixture_logpdf(m.arr, K, m.w.h, d.up(c["s"]), d.up(far), B, dlp)); lp = d.down(dlp, (B,))
    print("lp relative error %.3g" % (np.abs(lp - lp_ref) / np.abs(lp_ref)).max())
    assert np.isfinite(lp).all() and (np.abs(lp - lp_ref) <= 1e-5 * np.abs(lp_ref)).all()
    raw = np.zeros(L.INFO_N + K, np.float32); ctx.check(_step(m, c["s"], far, None, B, raw))
    info_r, _, new = MR.step(dict(c, a=far), MR.optimisers(c, LR))
    assert np.isfinite(raw[:2]).all() and abs(raw[0] - info_r["loss"]) <= 1e-4 * abs(info_r["loss"])
    after = m.params()      # the component that is not responsible has an exactly zero gradient and stays; the responsible one and the weight network move
    assert all(np.isfinite(got).all() for got in after) and sum(not np.array_equal(got, before) for got, before in zip(after, m.vectors)) >= 2


# ---- 3. one step against the yardstick ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,B,weighted", MR.STEP_CASES)
def test_step_matches_reference(gpu_ctx, name, K, B, weighted):
    L = _L(); ctx, c = gpu_ctx, _case(name, K, B); w = c["w"] if weighted else None
    info_r, gs, new = MR.step(c, MR.optimisers(c, LR), w=w)
    m = Mix(ctx, c); raw = np.zeros(L.INFO_N + K, np.float32)
    ctx.check(_step(m, c["s"], c["a"], w, B, raw))
    print("loss %.7g (ref %.7g) norm %.7g (ref %.7g)" % (raw[0], info_r["loss"], raw[1], info_r["grad_norm"]))
    close = lambda a, b: abs(a - b) <= 1e-4 * max(1.0, abs(b))      # noqa: E731
    assert close(raw[L.INFO["loss"]], info_r["loss"]) and close(raw[L.INFO["grad_norm"]], info_r["grad_norm"])
    assert _rel(raw[L.INFO_N:L.INFO_N + K], info_r["resp"])
    worst_share, worst_err, worst_g = 0.0, 0.0, 0.0
    for h, (g, gr, got, want) in enumerate(zip(m.grads(), gs, m.params(), new)):
        scale = np.abs(gr).max(); worst_g = max(worst_g, np.abs(g - gr).max() / scale)
        assert np.abs(g - gr).max() <= 1e-4 * scale, (h, np.abs(g - gr).max(), scale)
        ok = np.abs(gr) > 1e-3 * scale
        worst_share = max(worst_share, 1.0 - ok.mean()); worst_err = max(worst_err, np.abs(got[ok] - want[ok]).max())
        assert np.isfinite(got).all()
    print("  worst gradient error %.3g of the scale; entries not compared: %.2f %%; worst parameter error %.3g" % (worst_g, 100 * worst_share, worst_err))
    assert worst_share <= STEP_SKIPPED_MAX and worst_err < 2e-5


# ---- 4. the chain is its steps --------------------------------------------------------------------------------------------------------------------------------------------
def _train(m, c, perms, batch, max_batches, W):
    L = _L(); epochs, N = perms.shape; stride = L.INFO_N + m.K
    raw, rows = np.zeros(stride, np.float32), np.zeros((epochs, stride), np.float32)
    with Dev(m.ctx) as d:
        rc = m.ctx.lib.crux_mixture_train(m.arr, m.K, m.w.h, d.up(c["s"]), d.up(c["a"]), d.up(W) if W is not None else None, N, batch, epochs, max_batches, _vp(perms), _vp(raw), _vp(rows))
    return rc, raw, rows


@pytest.mark.parametrize("name,weighted", [("2-32-1", True), ("5-100-100-3", False)])
def test_train_equals_the_steps_one_by_one(gpu_ctx, name, weighted):
    L = _L(); ctx, K, N, batch, epochs = gpu_ctx, 3, 300, 128, 2
    c = _case(name, K, N); W = c["w"] if weighted else None
    perms = np.ascontiguousarray(np.stack([np.random.default_rng(40 + k).permutation(N) for k in range(epochs)]), np.int64)
    for max_batches in (0, 3):
        mbs = ER.minibatches(N, batch, epochs, perms, max_batches or None)
        assert [len(i) for _, i in mbs] == ([128, 128, 44] * 2 if not max_batches else [128, 128, 44])
        chain, chain2, steps = Mix(ctx, c), Mix(ctx, c), Mix(ctx, c)
        rc, raw, rows = _train(chain, c, perms, batch, max_batches, W); ctx.check(rc)
        rc2, raw2, rows2 = _train(chain2, c, perms, batch, max_batches, W); ctx.check(rc2)
        want_rows = {}
        for ep, idx in mbs:
            r = np.zeros(L.INFO_N + K, np.float32)
            ctx.check(_step(steps, c["s"][:, idx], c["a"][:, idx], W[:, idx] if weighted else None, len(idx), r)); want_rows[ep] = r
        n_run = len(want_rows)
        _same(chain.state(), steps.state()); _same(chain.state() + [raw, rows], chain2.state() + [raw2, rows2])
        assert raw[L.INFO["batches_trained"]] == len(mbs) and raw[L.INFO["epochs_run"]] == n_run and n_run == (2 if not max_batches else 1)
        for ep in range(n_run):
            assert rows[ep].tobytes() == want_rows[ep].tobytes()
        keep = [k for k in range(L.INFO_N + K) if k not in (L.INFO["batches_trained"], L.INFO["epochs_run"])]
        assert raw[keep].tobytes() == want_rows[n_run - 1][keep].tobytes()
        assert all(np.isfinite(p).all() and not np.array_equal(p, q) for p, q in zip(chain.params(), chain.vectors))
        ps, _ = MR.fit(c, c["s"], c["a"], W, batch, epochs, perms, max_batches or None, lr=LR)      # and the yardstick's fit over the same permutations
        err = max(np.abs(p - q).max() for p, q in zip(chain.params(), ps)); print("after %d steps: worst parameter error %.3g" % (len(mbs), err))
        assert err < len(mbs) * 2e-5      # 2e-5 per step taken


# ---- 5. exploration -------------------------------------------------------------------------------------------------------------------------------------------------------
def _explore(m, s, B, seed, counter, stream=0):
    nd = m.c["nd"]
    with Dev(m.ctx) as d:
        da, dl, dk = d.empty(nd * B), d.empty(B), d.empty(B)
        m.ctx.check(m.ctx.lib.crux_mixture_explore(m.arr, m.K, m.w.h, d.up(s), B, seed, counter, stream, da, dl, dk))
        return d.down(da, (nd, B)), d.down(dl, (B,)), d.down(dk, (B,), np.int32)


@pytest.mark.parametrize("name,K,B", [("2-32-1", 3, 257), ("5-100-100-3", 5, 37), ("4-256-256-2", 3, 37)])
def test_exploration_is_reproducible_and_consistent(gpu_ctx, name, K, B):
    ctx, c = gpu_ctx, _case(name, K, B); nd = c["nd"]; m = Mix(ctx, c, adam=False)
    a, lp, k = _explore(m, c["s"], B, 7, 100); a2, lp2, k2 = _explore(m, c["s"], B, 7, 100); a3, lp3, k3 = _explore(m, c["s"], B, 7, 100 + B)
    _same([a, lp, k], [a2, lp2, k2])
    assert not np.array_equal(a, a3) and (K == 1 or not np.array_equal(k, k3))
    assert ((k >= 0) & (k < K)).all() and len(set(k.tolist())) == K      # every component is drawn at these sizes
    with Dev(ctx) as d:
        dlp = d.empty(B); ctx.check(ctx.lib.crux_mixture_logpdf(m.arr, K, m.w.h, d.up(c["s"]), d.up(a), B, dlp)); lp_dev = d.down(dlp, (B,))
    assert (np.abs(lp - lp_dev) <= 1e-5 * np.maximum(1.0, np.abs(lp_dev))).all()
    assert np.abs(lp - MR.logpdf(c, a=a)).max() <= _lp_tol(name)
    mus = np.stack([ER.forward(p[:-nd], c["dims"], c["acts"], c["s"])[0] for p in c["ps"]]); sg = np.stack([np.exp(np.asarray(p[-nd:], np.float64)) for p in c["ps"]])
    eps = (a - mus[k, :, np.arange(B)].T) / sg[k].T      # a = mu_k + sigma_k eps for the reported k
    assert np.abs(eps).max() < 6
    n = eps.size; assert abs(eps.mean()) < 5 / np.sqrt(n) and abs((eps ** 2).mean() - 1) < 5 * np.sqrt(2.0 / n)      # standard normals: five standard deviations of either statistic


def test_exploration_draws_components_with_the_constant_weights(gpu_ctx):
    ctx, K, B = gpu_ctx, 2, 4096; c = dict(_case("5-100-100-3", K, B), wp=np.array([0.1, 0.9], np.float32)); m = Mix(ctx, c, adam=False)
    a, lp, k = _explore(m, c["s"], B, 11, 0)
    first = int((k == 0).sum()); print("component 1 drawn %d times of %d" % (first, B))
    assert 314 <= first <= 506      # 409.6 +- 5 binomial standard deviations of 19.2
    assert np.abs(lp - MR.logpdf(c, a=a)).max() <= _lp_tol("5-100-100-3")


# ---- 6. the NaN gate ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2-32-1", "5-100-100-3"])
def test_a_nan_in_a_updates_no_handle(gpu_ctx, name):
    L = _L(); ctx, lib, K, B = gpu_ctx, gpu_ctx.lib, 3, 37
    c = _case(name, K, B); a = c["a"].copy(); a[0, 5] = np.nan
    m = Mix(ctx, c); before = m.state(); raw = np.zeros(L.INFO_N + K, np.float32)
    rc = _step(m, c["s"], a, None, B, raw)
    assert rc == L.ENAN and "NaN detected!" in (lib.crux_last_error(ctx.h) or b"").decode()
    assert np.isnan(raw[L.INFO["grad_norm"]])
    _same(m.state(), before)
    with Dev(ctx) as d:      # the forward form gives NaN for that column alone
        dlp = d.empty(B); ctx.check(lib.crux_mixture_logpdf(m.arr, K, m.w.h, d.up(c["s"]), d.up(a), B, dlp)); lp = d.down(dlp, (B,))
    assert np.isnan(lp[5]) and np.isfinite(np.delete(lp, 5)).all()
    perms = np.arange(B, dtype=np.int64).reshape(1, B)      # the chain: the same verdict, nothing updated
    rc, _, _ = _train(m, dict(c, a=a), perms, 16, 0, None)
    assert rc == L.ENAN; _same(m.state(), before)
    fresh = Mix(ctx, c); r1, r2 = np.zeros_like(raw), np.zeros_like(raw)      # a following clean step is unaffected
    ctx.check(_step(fresh, c["s"], c["a"], None, B, r1)); ctx.check(_step(m, c["s"], c["a"], None, B, r2))
    _same(fresh.state() + [r1], m.state() + [r2])
    assert np.isfinite(r1[:2]).all() and not np.array_equal(fresh.nets[0].get_params(), c["ps"][0])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_parameters_untouched(gpu_ctx):
    L = _L(); crux = _crux(); ctx, lib, B = gpu_ctx, gpu_ctx.lib, 8
    c = MR.case("2-32-1", 3, 37); c = dict(c, s=c["s"][:, :B], a=c["a"][:, :B]); m = Mix(ctx, c); raw = np.zeros(L.INFO_N + 40, np.float32)
    err = lambda: (lib.crux_last_error(ctx.h) or b"").decode()      # noqa: E731
    with Dev(ctx) as d:
        ds, da = d.up(c["s"]), d.up(c["a"])
        step = lambda arr, K, w=m.w: lib.crux_mixture_step(arr, K, w.h, ds, da, None, B, _vp(raw))      # noqa: E731
        many = Mix(ctx, MR.case("2-32-1", 16, 37)); arr17 = (C.c_void_p * 17)(*([n.h.value for n in many.nets] + [m.nets[0].h.value]))
        assert step(arr17, 17) == L.EINVAL and "17 components" in err()
        other = dict(c, dims=(2, 33, 1), ps=[np.zeros(2 * 33 + 33 + 33 + 1 + 1, np.float32)]); o33 = Mix(ctx, other)
        assert step((C.c_void_p * 3)(m.nets[0].h.value, m.nets[1].h.value, o33.nets[0].h.value), 3) == L.EINVAL and "differs from member 0" in err()
        assert step((C.c_void_p * 3)(m.nets[0].h.value, m.nets[1].h.value, m.nets[0].h.value), 3) == L.EINVAL and "one handle" in err()
        sq = Mix(ctx, c, squashed=True)
        assert step(sq.arr, 3, sq.w) == L.EUNSUP and "SquashedGaussianPolicy" in err()
        plain = crux.ContinuousNetwork(_chain(c["dims"], c["acts"]), ctx=ctx); plain.attach_optimizer(crux.Adam(np.float32(LR)))
        assert step((C.c_void_p * 3)(m.nets[0].h.value, m.nets[1].h.value, plain.h.value), 3) == L.EINVAL      # no logSigma extras: another shape
        assert step(m.arr, 2) == L.EINVAL and "weight network must map" in err()      # three weights for two components
        two = crux.ParamVector(np.array([0.5, 0.5], np.float32), ctx=ctx); two.attach_optimizer(crux.Adam(np.float32(LR)))
        assert step(m.arr, 3, two) == L.EINVAL and "constant weights" in err()
        sn = crux.ContinuousNetwork(crux.Chain(crux.DenseSN(2, 32, "relu"), crux.Dense(32, 3)), ctx=ctx); sn.attach_optimizer(crux.Adam(np.float32(LR)))
        assert step(m.arr, 3, sn) == L.EUNSUP and "spectrally normalised" in err()
        wide = dict(c, dims=(2, 8, 9), nd=9, ps=[np.zeros(2 * 8 + 8 + 8 * 9 + 9 + 9, np.float32)] * 15, wdims=None, wp=np.full(15, 1 / 15, np.float32)); w15 = Mix(ctx, wide)
        assert lib.crux_mixture_step(w15.arr, 15, w15.w.h, ds, da, None, B, _vp(raw)) == L.EUNSUP and "at most 128 values per column" in err()      # 15 x 9 > the head's tile
        noadam = Mix(ctx, c, adam=False)
        assert step(noadam.arr, 3, noadam.w) == L.EINVAL and "crux_adam_init" in err()
        assert lib.crux_mixture_step(m.arr, 3, m.w.h, ds, da, None, 0, _vp(raw)) == L.EINVAL and lib.crux_mixture_step(m.arr, 3, m.w.h, ds, da, None, (1 << 20) + 1, _vp(raw)) == L.EINVAL
        bad_perm = np.full((1, B), B, np.int64)
        assert _train(m, c, bad_perm, 4, 0, None)[0] == L.EINVAL and "permutation entry" in err()
    for mix in (m, many, o33, sq, w15, noadam):
        _same(mix.params(), mix.vectors)
    # the host class
    gp = lambda h=32, cls=crux.Dense: crux.GaussianPolicy(crux.Chain(cls(2, h, "relu"), crux.Dense(h, 1)), np.zeros(1, np.float32), ctx=ctx)      # noqa: E731
    with pytest.raises(NotImplementedError, match="17 components"):
        crux.MixtureNetwork([gp() for _ in range(17)], np.full(17, 1 / 17), ctx=ctx)
    with pytest.raises(NotImplementedError, match="different shapes"):
        crux.MixtureNetwork([gp(), gp(33)], [0.5, 0.5], ctx=ctx)
    with pytest.raises(NotImplementedError, match="DenseSN"):
        crux.MixtureNetwork([gp(), gp(cls=crux.DenseSN)], [0.5, 0.5], ctx=ctx)
    with pytest.raises(NotImplementedError, match="SquashedGaussianPolicy"):
        crux.MixtureNetwork([gp(), crux.SquashedGaussianPolicy(crux.Chain(crux.Dense(2, 32, "relu"), crux.Dense(32, 1)), np.zeros(1, np.float32), 1.0, ctx=ctx)], [0.5, 0.5], ctx=ctx)
    with pytest.raises(NotImplementedError, match="categorical"):
        crux.MixtureNetwork([crux.DiscreteNetwork(crux.Chain(crux.Dense(2, 32, "relu"), crux.Dense(32, 2)), [1, 2], ctx=ctx) for _ in range(2)], [0.5, 0.5], ctx=ctx)
    keep = [gp(), gp()]; before = [n.get_params() for n in keep]
    for bad in ([0.5, 0.0], [1.5, -0.5]):
        with pytest.raises(ValueError, match="positive"):
            crux.MixtureNetwork(keep, bad, ctx=ctx)
    _same([n.get_params() for n in keep], before)


# ---- 8. the host mirror ---------------------------------------------------------------------------------------------------------------------------------------------------
def _mirror(ctx, c, opt=True):
    crux = _crux(); nd = c["nd"]
    nets = [crux.GaussianPolicy(_chain(c["dims"], c["acts"]), np.zeros(nd, np.float32), ctx=ctx, seed=3, stream=k) for k in range(c["K"])]
    pi = crux.MixtureNetwork(nets, c["wp"] if c["wdims"] is None else _chain(c["wdims"], c["wacts"]), ctx=ctx, seed=3)
    for n, p in zip(pi.networks + [pi.weight_network], list(c["ps"]) + [c["wp"]]):
        n.set_params(p)
    if opt:
        pi.attach_optimizer(crux.Adam(np.float32(LR)))
    return pi


@pytest.mark.parametrize("name", ["2-32-1", "5-100-100-3"])
def test_host_mirror_matches_reference(gpu_ctx, name):
    crux = _crux(); K, N = 3, 300; c = _case(name, K, N); nd = c["nd"]; tol = _lp_tol(name)
    pi = _mirror(gpu_ctx, c, opt=False); s, a, w = c["s"][:, :37], c["a"][:, :37], c["w"][:, :37]
    assert pi.K == K and pi.constant_weights == (c["wdims"] is None) and crux.dim(pi.action_space()) == (nd,)
    assert len(pi.params()) == K * (2 * len(c["acts"]) + 1) + (1 if c["wdims"] is None else 2 * len(c["wacts"]))      # the components' arrays, then the weights'
    assert _rel(pi.weights(s), MR.alphas(c, s)) and all(_rel(x, ER.forward(p[:-nd], c["dims"], c["acts"], s)[0]) for x, p in zip(pi.means(s), c["ps"]))
    lp = pi.logpdf(s, a); assert lp.shape == (1, 37) and np.abs(lp[0] - MR.logpdf(c, s, a)).max() <= tol
    assert np.abs(crux.logpdf(pi, s, a) - lp).max() == 0
    act, lpe, k = pi.exploration(s, seed=5, counter=9); act2 = pi.action(s, seed=5, counter=9)
    assert act.shape == (nd, 37) and lpe.shape == (1, 37) and k.shape == (37,) and np.array_equal(act, act2) and np.abs(lpe - pi.logpdf(s, act)).max() <= 1e-5 * max(1.0, np.abs(lpe).max())
    with pytest.raises(NotImplementedError):
        pi.entropy(s)
    with pytest.raises(ValueError):
        pi.train_step(s, a)
    for hand_over in (lambda: crux.PolicyParams(pi), lambda: crux.Sampler(crux.PendulumMDP(), pi), lambda: crux.clone_policy(pi)):
        with pytest.raises(NotImplementedError, match="Sampler and the solvers"):
            hand_over()
    _same([n.get_params() for n in pi.networks + [pi.weight_network]], list(c["ps"]) + [c["wp"]])
    pi.attach_optimizer(crux.Adam(np.float32(LR)))
    info_r, gs, new = MR.step(dict(c, s=s, a=a), MR.optimisers(c, LR), w=w)
    info = pi.train_step(s, a, w)
    assert abs(info["loss"] - info_r["loss"]) <= 1e-4 * max(1.0, abs(info_r["loss"])) and _rel(info["responsibilities"], info_r["resp"]) and abs(info["grad_norm"] - info_r["grad_norm"]) <= 1e-4 * max(1.0, info_r["grad_norm"])
    for n, gr, want in zip(pi.networks + [pi.weight_network], gs, new):
        ok = np.abs(gr) > 1e-3 * np.abs(gr).max(); assert np.abs(n.get_params()[ok] - want[ok]).max() < 2e-5
    outs = []
    for _ in range(2):      # fit: reproducible bit for bit, and the yardstick over the same permutations
        p2 = _mirror(gpu_ctx, c); h = p2.fit(c["s"], c["a"], batch_size=128, epochs=2, weights=c["w"], seed=7)
        outs.append([n.get_params() for n in p2.networks + [p2.weight_network]] + [np.array([r["loss"] for r in h["epochs"]], np.float32)])
        assert h["batches_trained"] == 6 and h["epochs_run"] == 2 and len(h["epochs"]) == 2 and h["responsibilities"].shape == (K,)
    _same(outs[0], outs[1])
    rng = np.random.default_rng(7); perms = [rng.permutation(N) for _ in range(2)]
    ps, rows = MR.fit(c, c["s"], c["a"], c["w"], 128, 2, perms, lr=LR)
    assert all(np.abs(x - y).max() < 6 * 2e-5 for x, y in zip(outs[0][:K + 1], ps)) and _rel(outs[0][K + 1], np.array([r["loss"] for r in rows]))
    h3 = p2.fit(c["s"], c["a"], batch_size=128, epochs=2, seed=7, max_batches=3)
    assert h3["batches_trained"] == 3 and h3["epochs_run"] == 1


# ---- 9. learning ----------------------------------------------------------------------------------------------------------------------------------------------------------
LEARN_EPOCHS, LEARN_BATCH, LEARN_LR = 60, 256, 3e-3


def _fit_bimodal(ctx, K):
    crux = _crux(); N = 8192; S, Y = MR.bimodal(N, 1); Sh, Yh = MR.bimodal(N, 2)
    nets = [crux.GaussianPolicy(_chain((2, 32, 1), ("relu", "identity")), np.zeros(1, np.float32), ctx=ctx, seed=5, stream=k) for k in range(K)]
    pi = crux.MixtureNetwork(nets, _chain((2, 32, K), ("relu", "identity")), ctx=ctx, seed=5); pi.attach_optimizer(crux.Adam(np.float32(LEARN_LR)))
    before = float(-pi.logpdf(Sh, Yh).mean(dtype=np.float64))
    h = pi.fit(S, Y, batch_size=LEARN_BATCH, epochs=LEARN_EPOCHS, seed=1)
    assert h["epochs_run"] == LEARN_EPOCHS and h["batches_trained"] == LEARN_EPOCHS * (N // LEARN_BATCH)
    return before, float(-pi.logpdf(Sh, Yh).mean(dtype=np.float64)), float(0.5 * np.log(2 * np.pi * np.e * Yh.var(dtype=np.float64))), pi, Sh


def test_fit_learns_the_bimodal_target(gpu_ctx):
    """The reference's DeepGMM experiment (mixture_network_tests.jl): 0.5 N(1, 0.2) + 0.5 N(-1, 1), constant input 0.1, N = 8192 and a held-out 8192."""
    b2, nll2, single, pi, Sh = _fit_bimodal(gpu_ctx, 2); b1, nll1, _, _, _ = _fit_bimodal(gpu_ctx, 1)
    al = pi.weights(Sh[:, :1])[:, 0]; mu = [float(m[0, 0]) for m in pi.means(Sh[:, :1])]; sg = [float(np.exp(n.get_params()[-1])) for n in pi.networks]
    print("held-out NLL: K = 2 %.4f -> %.4f, K = 1 %.4f -> %.4f, single-Gaussian optimum %.4f; fitted alpha %s mu %s sigma %s" % (b2, nll2, b1, nll1, single, al, mu, sg))
    assert 1.55 < single < 1.70
    assert nll2 < single and nll2 < b2
    assert nll1 >= single - 0.02
