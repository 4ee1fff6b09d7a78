"""mixture.py -- MixtureNetwork (src/policies.jl:189-242): a mixture-density policy over the member-grouped dense passes (csrc/mixture.hip).

Arrays are (features, batch) and Float32 as everywhere in core.py. K <= 16 GaussianPolicy components of one shape give mu_k(s) [nd x B]; their trailing extras are the
constant trainable logSigma_k [nd], unclamped. The weights are a Chain with K output rows (the head applies a max-subtracted softmax over the rows: the reference's
Chain(..., softmax)) or a constant positive vector alpha [K], used raw and trainable (its ConstantLayer form; not renormalised).

    l_kj = sum_d [ -(a_dj - mu_kdj)^2 / (2 sigma_kd^2) - 0.9189385332046727f0 - logSigma_kd ],   t_kj = log alpha_kj + l_kj,   lp_j = m_j + log sum_k exp(t_kj - m_j)

Two deliberate differences from policies.jl:229-233:
  1. the reference evaluates log(sum(alpha[i] .* exp.(logpdf_i))) directly, which is -Inf once every l_k < -103; the stable form above is its commented-out intent
     (weighted_logsumexp, utils.jl:147). The two agree wherever the naive form is finite;
  2. alpha[i] there is linear indexing: with a weight network and B > 1 it reads column 1's weights for every column. Here alpha_kj is per column. The two agree for
     constant weights and for B = 1.

Everything numerical runs on the device; what the device path does not cover raises NotImplementedError naming the reason (components of different shapes, DenseSN
layers, more than 16 components, SquashedGaussianPolicy or DiscreteNetwork components) -- there is no host fallback. A MixtureNetwork is a policy class with a likelihood
step and a fit loop; handing it to a Sampler or a solver raises NotImplementedError."""
import ctypes as C

import numpy as np

from . import _lib as L
from .core import refuse_conv, refuse_optimiser_chain
from .core import Chain, ContinuousNetwork, ContinuousSpace, DenseSN, DiscreteNetwork, GaussianPolicy, ParamVector, SquashedGaussianPolicy, _vp, default_context
from .ensembles import _DeviceArrays

MAX_COMPONENTS = 16
NOT_A_SOLVER_POLICY = "a MixtureNetwork is a policy class with logpdf, exploration, train_step and fit; the Sampler and the solvers do not take it yet"


class MixtureNetwork:
    """MixtureNetwork(networks, weights) (policies.jl:189-194). networks: K GaussianPolicy of one shape; weights: a Chain in -> K (or a ContinuousNetwork over one), or K
    positive numbers. params(): the components' arrays followed by the weights', as Flux.trainable orders them."""
    not_a_solver_policy = NOT_A_SOLVER_POLICY

    def __init__(self, networks, weights, ctx=None, seed=0):
        name = type(self).__name__; networks = list(networks); K = len(networks)
        if K < 1:
            raise ValueError("%s: no components" % name)
        for q in networks + [weights]:      # (a Chain carries its trunk in .conv, a network in .trunk)
            if getattr(q, "conv", None) is not None:
                raise NotImplementedError("%s: a weight network with a convolutional trunk (Conv layers in its Chain) is not implemented" % name)
            refuse_conv(q, name)
        if K > MAX_COMPONENTS:
            raise NotImplementedError("%s: %d components; the grouped device passes take at most %d" % (name, K, MAX_COMPONENTS))
        for n in networks:
            if isinstance(n, DiscreteNetwork):
                raise NotImplementedError("%s: DiscreteNetwork components (a mixture of categoricals is itself a categorical, and the reference's own test marks its action "
                                          "as broken); the device head is the Gaussian one" % name)
            if getattr(n, "two_headed", False):
                raise NotImplementedError("%s: components whose logSigma is a network (two-headed actors); the mixture head reads constant logSigma extras" % name)
            if isinstance(n, SquashedGaussianPolicy):
                raise NotImplementedError("%s: SquashedGaussianPolicy components (the mixture head has no tanh correction)" % name)
            if not isinstance(n, GaussianPolicy):
                raise TypeError("%s: the components must be GaussianPolicy, not %s" % (name, type(n).__name__))
            if n.is_spectral:
                raise NotImplementedError("%s: DenseSN layers (the grouped device passes read the raw weights)" % name)
            if n.network.dims != networks[0].network.dims or n.network.acts != networks[0].network.acts or n.n_extra != networks[0].n_extra:
                raise NotImplementedError("%s: components of different shapes (the grouped device passes need one shape)" % name)
        self.ctx = ctx or networks[0].ctx
        if any(n.ctx is not self.ctx for n in networks):
            raise ValueError("%s: the components belong to different contexts" % name)
        self.networks, self.dims = networks, networks[0].network.dims
        if networks[0].n_extra != self.dims[-1]:
            raise ValueError("%s: %d logSigma entries for %d action rows" % (name, networks[0].n_extra, self.dims[-1]))
        if isinstance(weights, Chain):
            if any(isinstance(l, DenseSN) for l in weights.layers):
                raise NotImplementedError("%s: DenseSN layers in the weight network" % name)
            weights = ContinuousNetwork(weights, ctx=self.ctx, seed=seed, stream=K)
        if isinstance(weights, ContinuousNetwork):
            if weights.is_spectral:
                raise NotImplementedError("%s: DenseSN layers in the weight network" % name)
            if weights.network.dims[0] != self.dims[0] or weights.network.dims[-1] != K:
                raise ValueError("%s: the weight network maps %d -> %d, expected %d -> %d" % (name, weights.network.dims[0], weights.network.dims[-1], self.dims[0], K))
        elif not isinstance(weights, ParamVector):
            alpha = np.asarray(weights, np.float32).reshape(-1)
            if alpha.size != K:
                raise ValueError("%s: %d constant weights for %d components" % (name, alpha.size, K))
            if not (alpha > 0).all():
                raise ValueError("%s: the constant weights must be positive (their logarithm enters the density)" % name)
            weights = ParamVector(alpha, ctx=self.ctx)
        self.weight_network = weights
        self.optimizer = None
        self._nets = (C.c_void_p * K)(*[n.h.value for n in networks])

    # ---- shapes -------------------------------------------------------------------------------------------------------------------------------------------------
    @property
    def K(self):
        return len(self.networks)

    @property
    def nd(self):
        return self.dims[-1]

    @property
    def constant_weights(self):
        return isinstance(self.weight_network, ParamVector)

    @property
    def network(self):
        raise NotImplementedError(NOT_A_SOLVER_POLICY)

    def action_space(self):
        """action_space(n.networks[1]) (policies.jl:203)"""
        return ContinuousSpace(self.nd)

    def params(self):
        return [a for n in self.networks for a in n.params()] + self.weight_network.params()

    def _s(self, s):
        s = np.asarray(s, np.float32)
        s = s.reshape(self.dims[0], 1) if s.ndim == 1 else s
        if s.shape[0] != self.dims[0]:
            raise ValueError("input has %d rows, the components expect %d" % (s.shape[0], self.dims[0]))
        return s

    def _rows(self, a, rows, B, what):
        a = np.asarray(a, np.float32)
        a = a.reshape(rows, B) if a.ndim == 1 else a
        if a.shape != (rows, B):
            raise ValueError("%s has shape %s, expected %s" % (what, a.shape, (rows, B)))
        return a

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------------------------
    def weights(self, s):
        """alpha [K x B] (policies.jl:205): the softmax of the weight network's rows, or the constant vector for every column"""
        return self._weights(s, False)[0]

    def _weights(self, s, members=True):
        s = self._s(s); B, K, n = s.shape[1], self.K, self.nd * s.shape[1]
        with _DeviceArrays(self.ctx) as d:
            ds, da = d.up(s), d.empty(K * B); dmu = d.empty(K * n) if members else None
            self.ctx.check(self.ctx.lib.crux_mixture_weights(self._nets, K, self.weight_network.h, ds, B, da, dmu))
            alpha = d.down(da, (K, B)); mus = None
            if members:
                mu = d.down(dmu, (n, K)); mus = [mu[:, k].reshape((self.nd, B), order="F") for k in range(K)]
        return alpha, mus

    def means(self, s):
        """[mu_k(s)] of the components, from the grouped forward pass"""
        return self._weights(s, True)[1]

    def logpdf(self, s, a):
        """logpdf(pi, s, a) [1 x B] (policies.jl:229-233, in the stable form of the module docstring)"""
        s = self._s(s); B = s.shape[1]; a = self._rows(a, self.nd, B, "a")
        with _DeviceArrays(self.ctx) as d:
            ds, da, do = d.up(s), d.up(a), d.empty(B)
            self.ctx.check(self.ctx.lib.crux_mixture_logpdf(self._nets, self.K, self.weight_network.h, ds, da, B, do))
            return d.down(do, (1, B))

    def exploration(self, s, seed=0, counter=0, stream=0):
        """exploration(pi, s) (policies.jl:213-227): (a [nd x B], logprob [1 x B], the chosen component per column, 0-based); a pure function of (seed, counter, stream)"""
        s = self._s(s); B = s.shape[1]
        with _DeviceArrays(self.ctx) as d:
            ds, da, dl, dk = d.up(s), d.empty(self.nd * B), d.empty(B), d.empty(B)
            self.ctx.check(self.ctx.lib.crux_mixture_explore(self._nets, self.K, self.weight_network.h, ds, B, int(seed), int(counter), int(stream), da, dl, dk))
            return d.down(da, (self.nd, B)), d.down(dl, (1, B)), self.ctx.d2h(dk, np.empty(B, np.int32))

    def action(self, s, **kw):
        """POMDPs.action(pi, s) = exploration(pi, s)[1] (policies.jl:211)"""
        return self.exploration(s, **kw)[0]

    def entropy(self, s=None):
        raise NotImplementedError("entropy(::MixtureNetwork): a Gaussian mixture's entropy has no closed form (the reference throws as well, policies.jl:235-237)")

    # ---- training -----------------------------------------------------------------------------------------------------------------------------------------------
    def attach_optimizer(self, opt):
        """one Adam over all K + 1 handles: element-wise, so one Adam per handle with the same hyper-parameters"""
        refuse_optimiser_chain(opt, "MixtureNetwork.attach_optimizer (the grouped Adam of the mixture step)")
        self.optimizer = opt
        for n in self.networks + [self.weight_network]:
            n.attach_optimizer(opt)

    def _info(self, raw):
        raw = np.asarray(raw, np.float32)
        return {"loss": float(raw[L.INFO["loss"]]), "grad_norm": float(raw[L.INFO["grad_norm"]]), "responsibilities": raw[L.INFO_N:L.INFO_N + self.K].copy()}

    def train_step(self, s, a, weights=None):
        """one gradient step of -mean(w .* logpdf(pi, s, a)) (train!, src/training.jl:13-25); raises CruxError(ENAN) and updates nothing on a NaN"""
        if self.optimizer is None:
            raise ValueError("train_step: attach_optimizer was not called")
        s = self._s(s); B = s.shape[1]; a = self._rows(a, self.nd, B, "a"); w = None if weights is None else self._rows(weights, 1, B, "weights")
        raw = np.zeros(L.INFO_N + self.K, np.float32)
        with _DeviceArrays(self.ctx) as d:
            ds, da, dw = d.up(s), d.up(a), (d.up(w) if w is not None else None)
            self.ctx.check(self.ctx.lib.crux_mixture_step(self._nets, self.K, self.weight_network.h, ds, da, dw, B, _vp(raw)))
        return self._info(raw)

    def fit(self, S, A, batch_size=128, epochs=1, weights=None, seed=0, max_batches=None):
        """batch_train! (src/training.jl:28-55) over (S, A): per epoch a permutation drawn from numpy's default_rng(seed), partitions of batch_size columns (a short last
        one runs). Returns the last epoch's info with "epochs" (one info per epoch run), "batches_trained" and "epochs_run"."""
        if self.optimizer is None:
            raise ValueError("fit: attach_optimizer was not called")
        S = self._s(S); N = S.shape[1]; A = self._rows(A, self.nd, N, "A"); W = None if weights is None else self._rows(weights, 1, N, "weights")
        rng = np.random.default_rng(seed); epochs = int(epochs)
        perms = np.ascontiguousarray(np.stack([rng.permutation(N) for _ in range(epochs)]), np.int64)
        return self.fit_with_permutations(S, A, W, batch_size, perms, max_batches)

    def fit_with_permutations(self, S, A, W, batch_size, perms, max_batches=None):
        if self.optimizer is None:
            raise ValueError("fit: attach_optimizer was not called")
        perms = np.ascontiguousarray(perms, np.int64); epochs, N = perms.shape; stride = L.INFO_N + self.K
        S = self._s(S); A = self._rows(A, self.nd, N, "A"); W = None if W is None else self._rows(W, 1, N, "weights")
        raw, rows = np.zeros(stride, np.float32), np.zeros((epochs, stride), np.float32)
        with _DeviceArrays(self.ctx) as d:
            dS, dA, dW = d.up(S), d.up(A), (d.up(W) if W is not None else None)
            self.ctx.check(self.ctx.lib.crux_mixture_train(self._nets, self.K, self.weight_network.h, dS, dA, dW, N, int(batch_size), epochs, int(max_batches or 0), _vp(perms), _vp(raw), _vp(rows)))
        out = self._info(raw); n_run = int(raw[L.INFO["epochs_run"]])
        out.update(batches_trained=int(raw[L.INFO["batches_trained"]]), epochs_run=n_run, epochs=[self._info(r) for r in rows[:n_run]])
        return out


__all__ = ["MixtureNetwork"]
