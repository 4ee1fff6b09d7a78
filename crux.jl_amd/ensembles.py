"""ensembles.py -- DeepEnsemble and DeepClassificationEnsemble (src/extras/deep_ensembles.jl) over the member-grouped dense passes (csrc/ensemble.hip).

Arrays are (features, batch) as everywhere in core.py. Everything numerical runs on the device; what the device path does not cover raises NotImplementedError
naming the reason (DenseSN layers, members of different shapes, more than 16 members) -- there is no host fallback."""
import ctypes as C

import numpy as np

from . import _lib as L
from .core import Chain, ContinuousNetwork, DenseSN, _vp, default_context, refuse_optimiser_chain

MAX_MEMBERS = 16


class _DeviceArrays:
    """device copies of host arrays for the length of one call"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, a):
        a = np.asfortranarray(a, np.float32); p = self.ctx.alloc(max(a.nbytes, 4)); self.ptrs.append(p); self.ctx.h2d(p, a); return p

    def empty(self, n):
        p = self.ctx.alloc(4 * max(int(n), 1)); self.ptrs.append(p); return p

    def down(self, p, shape):
        return self.ctx.d2h(p, np.empty(shape, np.float32, order="F"))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.ctx.free(p)


class _Ensemble:
    kind = None

    def __init__(self, generator, N, ctx=None, seed=0):
        N = int(N)
        if N < 1:
            raise ValueError("%s: N = %d members" % (type(self).__name__, N))
        if N > MAX_MEMBERS:
            raise NotImplementedError("%s: %d members; the grouped device passes take at most %d" % (type(self).__name__, N, MAX_MEMBERS))
        self.ctx = ctx or default_context()
        chains = [generator() for _ in range(N)]                                                 # [generator() for _=1:N] (:3, :41)
        for ch in chains:
            if not isinstance(ch, Chain):
                raise TypeError("%s: generator() must return a Chain" % type(self).__name__)
            if any(isinstance(l, DenseSN) for l in ch.layers):
                raise NotImplementedError("%s: DenseSN layers (the grouped device passes read the raw weights)" % type(self).__name__)
            if ch.dims != chains[0].dims or ch.acts != chains[0].acts:
                raise NotImplementedError("%s: members of different shapes (the grouped device passes need one shape)" % type(self).__name__)
        if self.kind == "gauss" and chains[0].dims[-1] % 2:
            raise ValueError("DeepEnsemble: the output width %d is odd (mean and variance halves)" % chains[0].dims[-1])
        if any(getattr(ch, "conv", None) is not None for ch in chains):
            raise NotImplementedError("%s: members with a convolutional trunk (Conv layers in their Chain) are not implemented" % type(self).__name__)
        self.models = [ContinuousNetwork(ch, ctx=self.ctx, seed=seed, stream=m) for m, ch in enumerate(chains)]      # independent Glorot streams
        self.dims = chains[0].dims
        self.optimizer = None
        self._nets = (C.c_void_p * N)(*[m.h.value for m in self.models])

    # ---- shapes -------------------------------------------------------------------------------------------------------------------------------------------------
    @property
    def M(self):
        return len(self.models)

    @property
    def ny(self):
        """rows of y: nd for the regression ensemble, the number of classes otherwise"""
        return self.dims[-1] // 2 if self.kind == "gauss" else self.dims[-1]

    def _x(self, x):
        x = np.asarray(x, np.float32)
        x = x.reshape(self.dims[0], 1) if x.ndim == 1 else x
        if x.shape[0] != self.dims[0]:
            raise ValueError("input has %d rows, the members expect %d" % (x.shape[0], self.dims[0]))
        return x

    def _y(self, y, B, what="y"):
        y = np.asarray(y, np.float32)
        y = y.reshape(self.ny, B) if y.ndim == 1 else y
        if y.shape != (self.ny, B):
            raise ValueError("%s has shape %s, expected %s" % (what, y.shape, (self.ny, B)))
        return y

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------------------------
    def _forward(self, x, members=True):
        x = self._x(x); B, n, M = x.shape[1], self.ny * x.shape[1], self.M; lib, k = self.ctx.lib, L.ENS[self.kind]
        with _DeviceArrays(self.ctx) as d:
            dx, dmean, devar = d.up(x), d.empty(n), d.empty(n)
            dmu, dvar = (d.empty(M * n), d.empty(M * n)) if members else (None, None)
            self.ctx.check(lib.crux_ensemble_forward(self._nets, M, k, dx, B, dmu, dvar, dmean, devar))
            mean = d.down(dmean, (self.ny, B)); evar = d.down(devar, (self.ny, B)) if self.kind == "gauss" else None
            mus = vars_ = None
            if members:
                mu = d.down(dmu, (n, M)); mus = [mu[:, m].reshape((self.ny, B), order="F") for m in range(M)]
                if self.kind == "gauss":
                    va = d.down(dvar, (n, M)); vars_ = [va[:, m].reshape((self.ny, B), order="F") for m in range(M)]
        return mus, vars_, mean, evar

    def logpdf(self, x, y):
        x = self._x(x); B = x.shape[1]; y = self._y(y, B); rows = self.ny if self.kind == "gauss" else 1
        with _DeviceArrays(self.ctx) as d:
            dx, dy, do = d.up(x), d.up(y), d.empty(rows * B)
            self.ctx.check(self.ctx.lib.crux_ensemble_logpdf(self._nets, self.M, L.ENS[self.kind], dx, dy, B, do))
            return d.down(do, (rows, B))

    # ---- training -----------------------------------------------------------------------------------------------------------------------------------------------
    def attach_optimizer(self, opt):
        """one Adam for the ensemble: element-wise, so one Adam per member with the same hyper-parameters"""
        refuse_optimiser_chain(opt, type(self).__name__ + ".attach_optimizer (the grouped Adam of the ensemble step)")
        self.optimizer = opt
        for m in self.models:
            m.attach_optimizer(opt)

    def _info(self, raw):
        M = self.M; raw = np.asarray(raw, np.float32)
        return {"loss": float(raw[L.INFO["loss"]]), "grad_norm": float(raw[L.INFO["grad_norm"]]), "member_losses": raw[L.INFO_N:L.INFO_N + M].copy(),
                "member_grad_norms": raw[L.INFO_N + M:L.INFO_N + 2 * M].copy()}

    def train_step(self, x, y, weights=None):
        """one gradient step of training_loss on (x, y) (train!, src/training.jl:13-25); raises CruxError(ENAN) and updates nothing on a NaN gradient norm"""
        if self.optimizer is None:
            raise ValueError("train_step: attach_optimizer was not called")
        x = self._x(x); B = x.shape[1]; y = self._y(y, B); w = None if weights is None else self._y(weights, B, "weights")
        raw = np.zeros(L.INFO_N + 2 * self.M, np.float32)
        with _DeviceArrays(self.ctx) as d:
            dx, dy, dw = d.up(x), d.up(y), (d.up(w) if w is not None else None)
            self.ctx.check(self.ctx.lib.crux_ensemble_step(self._nets, self.M, L.ENS[self.kind], dx, dy, dw, B, _vp(raw)))
        return self._info(raw)

    def fit(self, X, Y, batch_size=128, epochs=1, weights=None, seed=0, max_batches=None):
        """batch_train! (src/training.jl:28-55) over (X, Y): per epoch a permutation drawn from numpy's default_rng(seed), partitions of batch_size columns (a short last
        one runs). Returns the last epoch's info with "epochs" (one info per epoch run), "batches_trained" and "epochs_run"."""
        if self.optimizer is None:
            raise ValueError("fit: attach_optimizer was not called")
        X = self._x(X); N = X.shape[1]; Y = self._y(Y, N); W = None if weights is None else self._y(weights, N, "weights")
        rng = np.random.default_rng(seed); epochs = int(epochs)
        perms = np.ascontiguousarray(np.stack([rng.permutation(N) for _ in range(epochs)]), np.int64)
        return self.fit_with_permutations(X, Y, W, batch_size, perms, max_batches)

    def fit_with_permutations(self, X, Y, W, batch_size, perms, max_batches=None):
        perms = np.ascontiguousarray(perms, np.int64); epochs, N = perms.shape; stride = L.INFO_N + 2 * self.M
        raw, rows = np.zeros(stride, np.float32), np.zeros((epochs, stride), np.float32)
        with _DeviceArrays(self.ctx) as d:
            dX, dY, dW = d.up(X), d.up(Y), (d.up(W) if W is not None else None)
            self.ctx.check(self.ctx.lib.crux_ensemble_train(self._nets, self.M, L.ENS[self.kind], dX, dY, dW, N, int(batch_size), epochs, int(max_batches or 0), _vp(perms), _vp(raw), _vp(rows)))
        out = self._info(raw); n_run = int(raw[L.INFO["epochs_run"]])
        out.update(batches_trained=int(raw[L.INFO["batches_trained"]]), epochs_run=n_run, epochs=[self._info(r) for r in rows[:n_run]])
        return out


class DeepEnsemble(_Ensemble):
    """DeepEnsemble(generator, N) (deep_ensembles.jl:1-36): N regression members whose output halves are a mean and a softplus variance."""
    kind = "gauss"

    def __call__(self, x):
        """(mu*, var*) of the mixture (:20-24)"""
        _, _, mean, evar = self._forward(x, members=False)
        return mean, evar


class DeepClassificationEnsemble(_Ensemble):
    """DeepClassificationEnsemble(generator, N) (deep_ensembles.jl:39-68): N softmax classifiers; y is one-hot (classes, batch)."""
    kind = "class"

    def __call__(self, x):
        """mean_m softmax(model_m(x)) (:54-57)"""
        return self._forward(x, members=False)[2]


def individual_forward(ens, x):
    """([mu_m], [var_m]) of a DeepEnsemble (:11-17), [p_m] of a DeepClassificationEnsemble (:49-51)"""
    mus, vars_, _, _ = ens._forward(x)
    return (mus, vars_) if ens.kind == "gauss" else mus


def logpdf(ens, x, y):
    """Distributions.logpdf(ens, x, y) (:30, :60-62)"""
    return ens.logpdf(x, y)


def training_loss(ens, x, y, weights=None):
    """training_loss(ens, x, y, weights) (:33-36, :65-68): the value only, from the members' heads of one device forward pass (Float32 like the reference; the means in
    Float64). Updates nothing. The classification loss accepts and ignores the weights, as the reference does."""
    x = ens._x(x); B = x.shape[1]; y = ens._y(y, B)
    mus, vars_, _, _ = ens._forward(x)
    if ens.kind == "class":
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.mean([np.mean(-np.where(y == 0, np.float32(0), y * np.log(p + np.float32(2.0 ** -23))).sum(0), dtype=np.float64) for p in mus]))
    w = np.ones_like(y) if weights is None else ens._y(weights, B, "weights")
    return float(np.mean([np.mean(-(w * (-np.log(v) / np.float32(2) - (y - mu) ** 2 / (np.float32(2) * v))), dtype=np.float64) for mu, v in zip(mus, vars_)]))


__all__ = ["DeepEnsemble", "DeepClassificationEnsemble", "individual_forward", "logpdf", "training_loss"]
