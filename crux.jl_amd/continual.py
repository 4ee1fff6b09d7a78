"""continual.py -- continual learning in parameter space: DiagonalFisherRegularizer (elastic weight consolidation, src/extras/fisher_information.jl) and the driver
continual_learning / log_multitask_performances! (src/extras/multitask_learning.jl).

The regulariser's state (F, theta_prev) lives on the device beside the handle it belongs to (csrc/fisher.hip). As the `regularizer` of a TrainingParams it rides in the
dense-engine learner's chain (crux_batch_train_fisher): no gradient crosses to the host. `crux_jl_amd.api` re-exports everything here."""
import copy
import ctypes as C

import numpy as np

from . import _lib as L
from .core import refuse_conv
from .core import CustomLoss, ParamLoss, Sampler, _ensure_opt, _info_dict, _train_cfg, _vp, clone_policy, refuse_two_headed, shuffle_device_, undiscounted_return


class DiagonalFisherRegularizer:
    """DiagonalFisherRegularizer(theta, lambda=1) (fisher_information.jl:1-8) for the parameters of ONE network handle `net`: F = 0, N = 0, theta_prev = copy(theta).
    R() = lam / A * sum_a mean_a(F .* (theta - theta_prev)^2) over the A parameter arrays of Flux.params(net) (:10-18): W_0, b_0, ..., then the trailing extras as one array.
    F, N and theta_prev read host copies; lam is settable; set_() loads a checkpoint."""

    def __init__(self, net, lam=1.0):
        refuse_two_headed(net, "DiagonalFisherRegularizer (EWC, continual_learning)"); refuse_conv(net, "DiagonalFisherRegularizer (EWC, continual_learning)")
        self.net, self.ctx = net, net.ctx
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.crux_fisher_create(net.h, float(np.float32(lam)), C.byref(h)))
        self.h, self._lam = h, float(np.float32(lam))

    def _get(self, want_F, want_prev):
        n = self.net.n_params
        F = np.empty(n, np.float32) if want_F else None; prev = np.empty(n, np.float32) if want_prev else None; N = C.c_int64(0)
        self.ctx.check(self.ctx.lib.crux_fisher_get(self.h, _vp(F), _vp(prev), C.byref(N)))
        return F, prev, int(N.value)

    @property
    def F(self):
        return self._get(True, False)[0]

    @property
    def theta_prev(self):
        return self._get(False, True)[1]

    @property
    def N(self):
        return self._get(False, False)[2]

    @property
    def lam(self):
        return self._lam

    @lam.setter
    def lam(self, v):
        self._lam = float(np.float32(v))
        self.ctx.check(self.ctx.lib.crux_fisher_set(self.h, None, None, -1, self._lam))

    def set_(self, F=None, theta_prev=None, N=None):
        n = self.net.n_params
        arrs = [None if a is None else np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (F, theta_prev)]
        for a in arrs:
            if a is not None and a.size != n:
                raise ValueError("DiagonalFisherRegularizer.set_: %d entries, the handle has %d parameters" % (a.size, n))
        self.ctx.check(self.ctx.lib.crux_fisher_set(self.h, _vp(arrs[0]), _vp(arrs[1]), -1 if N is None else int(N), self._lam))

    def __call__(self, accumulate=False):
        """R(pi) (:10-18). accumulate: its gradient 2 lam / (A numel_a) F (theta - theta_prev) is added to the handle's gradient buffer."""
        out = np.zeros(1, np.float32)
        self.ctx.check(self.ctx.lib.crux_fisher_reg(self.h, 1 if accumulate else 0, _vp(out)))
        return float(out[0])

    def snapshot_(self):
        """theta_prev = copy(theta) (:36)."""
        self.ctx.check(self.ctx.lib.crux_fisher_snapshot(self.h))

    def __del__(self):
        try:
            if getattr(self, "h", None) and self.ctx.h:
                self.ctx.lib.crux_fisher_destroy(self.h)
        except Exception:
            pass


def _loss_grad(R, p, P, D, ids0):
    """the gradient of p.loss on rows ids0 (0-based) into the handle's gradient buffer; no update"""
    pi = R.net
    if pi.optimizer is None:      # the learner entry wants an initialised optimiser state; one that is attached already stays (its moments are not reset)
        _ensure_opt(pi, p)
    raw = np.zeros(L.INFO_N, np.float32); cfg = _train_cfg(pi, p, P)
    ids0 = np.ascontiguousarray(ids0, np.int64)
    pi.ctx.check(pi.ctx.lib.crux_loss_grad(pi.h, D.h, C.byref(cfg), _vp(ids0), ids0.size, _vp(raw)))


def add_fisher_information_diagonal_(R, p=None, P=None, D=None, indices=None, times=1, grad=None):
    """add_fisher_information_diagonal!(R, neg_loss, theta) (fisher_information.jl:20-28): N += 1; F += (g .* g - F) / N with g the gradient of the loss of TrainingParams `p`
    on minibatch(D, indices) (1-based) -- the gradient of the batch loss, squared, not a per-sample square. grad: a flat gradient (uploaded) instead of a loss.
    times: that many consecutive calls with the same gradient, in one launch."""
    pi = R.net
    if grad is not None:
        g = np.ascontiguousarray(np.asarray(grad, np.float32).reshape(-1))
        if g.size != pi.n_params:
            raise ValueError("add_fisher_information_diagonal!: the gradient must have %d entries" % pi.n_params)
        pi.ctx.h2d(pi.ctx.lib.crux_mlp_grads_ptr(pi.h), g)
    else:
        _loss_grad(R, p, P if P is not None else {}, D, np.asarray(indices, np.int64) - 1)
    pi.ctx.check(pi.ctx.lib.crux_fisher_add(R.h, int(times)))


def update_fisher_(R, D, p, P, batch_size, per_minibatch=False, perm=None, shuffle_seed=0, shuffle_counter=0):
    """update_fisher!(R, D, loss, theta, batch_size) (fisher_information.jl:30-38): shuffle!(D), one add_fisher_information_diagonal! per
    partition(1:length(D), batch_size), then theta_prev = copy(theta). perm: the shuffle as a 1-based permutation (else the library's Philox shuffle).

    The reference's closure evaluates `loss(D)` -- the WHOLE buffer -- in every partition; the minibatch `mb` it builds is never used (:31-35). The default mirrors that
    literally: ONE whole-buffer gradient, added n_partitions times in one launch (the gradient is deterministic, so this is bit-identical to recomputing it each time).
    per_minibatch=True uses each partition's own gradient, the ragged last one included -- evidently what the reference meant."""
    n = len(D); batch_size = int(batch_size)
    if n < 1 or batch_size < 1:
        raise ValueError("update_fisher!: empty buffer or batch_size < 1")
    if perm is not None:
        D.shuffle_(np.asarray(perm, np.int64))
    else:
        shuffle_device_(D, shuffle_seed, shuffle_counter)
    P = P if P is not None else {}
    nparts = (n + batch_size - 1) // batch_size
    if per_minibatch:
        for st in range(0, n, batch_size):
            _loss_grad(R, p, P, D, np.arange(st, min(n, st + batch_size), dtype=np.int64))
            R.ctx.check(R.ctx.lib.crux_fisher_add(R.h, 1))
    else:
        _loss_grad(R, p, P, D, np.arange(n, dtype=np.int64))
        R.ctx.check(R.ctx.lib.crux_fisher_add(R.h, nparts))
    R.snapshot_()


def _batch_train_fisher(pi, p, P, D, info, perms):
    """batch_train! with p.regularizer a DiagonalFisherRegularizer of `pi` on the device (crux_batch_train_fisher); None = not a case of the chain (the caller's seam runs)."""
    R = p.regularizer
    if R.net is not pi or p.early_stopping is not None or isinstance(p.loss, (CustomLoss, ParamLoss)) or (p.loss.name not in L.LOSS and p.loss.name != "cost_value_mse") or p.loss.name == "lagrange_ppo":
        return None
    cfg = _train_cfg(pi, p, P)
    pp = None
    if perms is not None:
        pp = np.ascontiguousarray(np.asarray(perms, np.int64) - 1)
        if pp.shape != (p.epochs, len(D)):
            raise ValueError("batch_train!: perms must have shape (epochs, length(D))")
    raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((p.epochs, L.INFO_N), np.float32)
    rc = pi.ctx.lib.crux_batch_train_fisher(pi.h, R.h, D.h, C.byref(cfg), _vp(pp), _vp(raw), _vp(ep))
    if rc == L.EUNSUP:
        return None
    pi.ctx.check(rc)
    p.shuffle_counter += int(raw[L.INFO["epochs_run"]])
    info = info if info is not None else {}
    info.update(_info_dict(p, raw))
    info[p.name + "batches_trained"] = int(raw[L.INFO["batches_trained"]])
    info["_epochs_run"] = int(raw[L.INFO["epochs_run"]])
    info["_epoch_infos"] = ep[: info["_epochs_run"]]
    return info


# ---------------------------------------------------------------------------------------------- the driver (src/extras/multitask_learning.jl)
def _snapshot(solver):
    """deepcopy(S) as far as it can be mirrored: a shallow copy of the solver whose policy is a clone (ctypes handles cannot be deep-copied)"""
    snap = copy.copy(solver)
    ag = getattr(solver, "agent", None)
    if ag is not None and getattr(ag, "pi", None) is not None:
        pi = clone_policy(ag.pi)
        snap.agent = copy.copy(ag); snap.agent.pi = pi
        if ag.pi_explore is ag.pi:
            snap.agent.pi_explore = pi
    return snap


def continual_learning(tasks, solver_generator, solve=None):
    """continual_learning(tasks, solver_generator) (multitask_learning.jl:9-21): S = solver_generator(i=1, tasks=tasks[1:1], history=history); for every task solve(S, task),
    push a copy of S, and ask the generator for the next solver with (tasks=tasks[1:i+1], solvers=solvers, i=i+1, history=history). Returns the list of copies.
    The copies carry a clone_policy of the solver's policy. solve: the solve function (default: crux_jl_amd.api.solve)."""
    if solve is None:
        from . import api
        solve = api.solve
    tasks = list(tasks); solvers, history = [], []
    S = solver_generator(i=1, tasks=tasks[:1], history=history)
    for i in range(1, len(tasks) + 1):
        solve(S, tasks[i - 1])
        solvers.append(_snapshot(S))
        if i < len(tasks):
            S = solver_generator(tasks=tasks[:i + 1], solvers=solvers, i=i + 1, history=history)
    return solvers


def log_multitask_performances_(solver, tasks, logfn=None, Neps=10):
    """log_multitask_performances!(S, tasks, logfn) (multitask_learning.jl:5-7): one evaluation sampler per task on the solver's policy, logged as <name>/T<j> by the
    solver's LoggerParams. logfn(samplers) -> a log function; the default is the undiscounted return over Neps episodes per task."""
    from .logging import log_performance
    samplers = [Sampler(t, solver.agent, S=solver.S, max_steps=solver.max_steps) for t in tasks]
    fn = logfn(samplers) if logfn is not None else (lambda **kw: log_performance(samplers, "undiscounted_return", undiscounted_return, Neps=Neps))
    solver.log.fns.append(fn)
    return fn


__all__ = ["DiagonalFisherRegularizer", "add_fisher_information_diagonal_", "update_fisher_", "continual_learning", "log_multitask_performances_"]
