"""batch.py -- offline RL: the actor-critic form of BatchSolver, BatchSAC and CQL (src/model_free/batch.jl, batch/sac.jl, batch/cql.jl).

The actor-only BatchSolver (BC) keeps its path in imitation.py (_solve_batch); a BatchSolver with a critic or parameter optimisers runs the loop here.
Every train! is one C call on a minibatch gathered into a staging buffer on the device, with one info read-back per call.

Randomness (include/crux_rng.h, include/cruxhip.h CQL paragraph): the epoch shuffle is crux_buffer_shuffle(a_opt.shuffle_seed, epoch); minibatch g
(S.grad_steps, which continues across solve calls) takes the noise counters 8g + 0 (CQL alpha samples), + 1 (SAC temperature), + 2 (sac_target),
+ 3 (CQL critic samples), + 4 (actor), + 5 (AdVIL's gradient-penalty draws) of solver.noise_seed. The reference iterates param_optimizers in Dict order, which is unspecified; here the
order is fixed as CQL alpha first, then the SAC temperature (both updates are independent once the draws are counter-based).

AdVIL (il_batch.py) is the loop's other shape: a single ContinuousNetwork critic trained without a target (advil_d_loss) and a deterministic actor (advil_pi_loss
with an OrthogonalRegularizer), in the reference's order -- critic step first, then the actor step on the same minibatch with the updated critic (batch.jl:66-78)."""
import numpy as np

from . import _lib as L
from .core import (ActorCritic, ContinuousNetwork, DoubleNetwork, GaussianPolicy, OrthogonalRegularizer, ParamVector, PolicyParams, TrainingParams, _Loss,
                   _ensure_opt, _vp, buffer_like, clone_policy, copy_buffer, discount, normalize_, polyak_average_, shuffle_device_)
from .il_batch import advil_actor_step_, advil_d_loss, advil_d_step_, advil_pi_loss
from .imitation import BatchSolver
from .logging import aggregate_info
from .off_policy import double_Q_loss, sac_actor_loss, sac_temp_loss

cql_alpha_loss, cql_critic_loss = _Loss("cql_alpha"), _Loss("cql_critic")     # batch/cql.jl: cql_alpha_loss, cql_critic_loss() = double_Q_loss + conservative_loss

# noise counter offsets inside the block of 8 of one minibatch
CTR_CQL_ALPHA, CTR_SAC_TEMP, CTR_TARGET, CTR_CQL_CRITIC, CTR_ACTOR, CTR_ADVIL_GP, CTR_BLOCK = 0, 1, 2, 3, 4, 5, 8


class UniformBox:
    """product_distribution([Uniform(lo, hi) for i = 1:dim(A)]) -- the IS distribution of CQL (cql.jl, CQL_is_distribution); lo and hi are the same for every
    action dimension. The default of CQL is UniformBox(-1, 1)."""

    def __init__(self, lo=-1.0, hi=1.0):
        self.lo, self.hi = float(np.float32(lo)), float(np.float32(hi))
        if not self.hi > self.lo:
            raise ValueError("UniformBox: needs lo < hi")


def _check_actor_critic(pi, who):
    if not (isinstance(pi, ActorCritic) and isinstance(pi.A, GaussianPolicy) and isinstance(pi.C, DoubleNetwork)
            and isinstance(pi.C.N1, ContinuousNetwork) and isinstance(pi.C.N2, ContinuousNetwork)):
        raise TypeError("%s: pi must be ActorCritic(GaussianPolicy, DoubleNetwork(ContinuousNetwork, ContinuousNetwork))" % who)
    # (a constant-logSigma SquashedGaussianPolicy actor passes this test and is refused by the library -- CRUX_EUNSUP -- at the first step, as in SAC; the two-headed form
    #  -- logSigma a network on mu's trunk -- is taken, squashed or not)


def _check_advil(solver):
    """The shape AdVIL builds (AdVIL.jl:46-53): c_opt without a target_fn, a deterministic actor and a single critic."""
    pi, a_opt, c_opt = solver.agent.pi, solver.a_opt, solver.c_opt
    if not (isinstance(pi, ActorCritic) and isinstance(pi.A, ContinuousNetwork) and isinstance(pi.C, ContinuousNetwork)):
        raise TypeError("BatchSolver: advil_pi_loss / advil_d_loss need pi = ActorCritic(ContinuousNetwork, ContinuousNetwork)")
    if a_opt.loss is not advil_pi_loss or c_opt is None or c_opt.loss is not advil_d_loss:
        raise NotImplementedError("BatchSolver: advil_pi_loss and advil_d_loss are implemented as a pair (a_opt.loss, c_opt.loss)")
    if solver.target_fn is not None:
        raise NotImplementedError("BatchSolver: advil_d_loss takes no target (target_fn must be None)")
    if a_opt.regularizer is not None and not isinstance(a_opt.regularizer, OrthogonalRegularizer):
        raise NotImplementedError("BatchSolver: with advil_pi_loss the regularizer must be None or an OrthogonalRegularizer (it is evaluated on the device)")
    for k in ("lambda_GP", "lambda_BC"):
        if k not in solver.P:
            raise KeyError("BatchSolver: P[%r] is missing (AdVIL's λ_GP, λ_BC)" % k)


def _param_step(solver, theta, p, mb, base, info):
    """train!(theta, p_opt.loss(pi, P, mb), p_opt) (batch.jl:57-59) for the two parameter losses the library implements."""
    pi, P, ctx = solver.agent.pi, solver.P, mb.ctx
    _ensure_opt(theta, p)
    raw = np.zeros(L.INFO_N, np.float32)
    if p.loss is cql_alpha_loss:
        step = ctx.lib.crux_cql_alpha_step_sigma if pi.A.two_headed else ctx.lib.crux_cql_alpha_step      # (a two-headed actor got here through CQL(..., two_headed=True))
        ctx.check(step(pi.A.h, pi.C.N1.h, pi.C.N2.h, theta.h, mb.h, int(P["CQL_n_action_samples"]), P["CQL_is_distribution"].lo,
                       P["CQL_is_distribution"].hi, float(P["CQL_alpha_thresh"]), solver.noise_seed, base + CTR_CQL_ALPHA, _vp(raw)))
        info.update({p.name + "loss": float(raw[0]), p.name + "grad_norm": float(raw[1]), "CQL alpha": float(raw[L.INFO["alpha"]])})
    elif p.loss is sac_temp_loss:
        ctx.check(ctx.lib.crux_sac_temp_step(pi.A.h, theta.h, mb.h, float(P["SAC_H_target"]), solver.noise_seed, base + CTR_SAC_TEMP, _vp(raw)))
        info.update({p.name + "loss": float(raw[0]), p.name + "grad_norm": float(raw[1]), "SAC alpha": float(raw[L.INFO["alpha"]])})
    else:
        raise NotImplementedError("BatchSolver: parameter loss %r has no device implementation" % getattr(p.loss, "name", p.loss))


def _ordered_param_optimizers(solver):
    """CQL alpha before the SAC temperature (module docstring); any other entries keep their order after them."""
    rank = {cql_alpha_loss: 0, sac_temp_loss: 1}
    return sorted(solver.param_optimizers, key=lambda tp: rank.get(tp[1].loss, 2))


def _solve_batch_ac(solver, mdp=None):
    """POMDPs.solve(S::BatchSolver, mdp) (batch.jl:38-85) with a critic: for epoch in epoch:epoch + a_opt.epochs (inclusive: a_opt.epochs + 1 epochs), shuffle!,
    partition(1:n, batch_size) (the last minibatch may be short), and per minibatch: param optimisers -> y = target_fn -> train!(critic) -> target_update
    (polyak_average!(pi_minus, pi, 0.005) over the whole ActorCritic, :66-70, before the actor) -> train!(actor). After every epoch aggregate_info of the
    minibatch infos is appended to history and a_opt.early_stopping(history) is asked. c_opt.epochs and the other optimisers' batch sizes are ignored."""
    pi, pim, P, D = solver.agent.pi, solver.agent.pi_minus, solver.P, solver.D_train
    A, Q = pi.A, pi.C
    ctx, lib = D.ctx, D.ctx.lib
    a_opt, c_opt = solver.a_opt, solver.c_opt
    gamma = float(np.float32(discount(mdp))) if mdp is not None else float(np.float32(solver.gamma))
    _ensure_opt(A, a_opt)
    advil = a_opt.loss is advil_pi_loss or (c_opt is not None and c_opt.loss is advil_d_loss)
    if advil:
        _check_advil(solver)
        _ensure_opt(Q, c_opt)
    elif c_opt is not None:
        _ensure_opt(Q.N1, c_opt); _ensure_opt(Q.N2, c_opt)
    n, B = len(D), int(a_opt.batch_size)
    if n < 1:
        raise ValueError("BatchSolver: empty training data")
    if solver._mb is None or solver._mb.capacity < B:
        solver._mb = buffer_like(D, capacity=B)
        solver._dy = ctx.alloc(4 * B)
    mb, d_y = solver._mb, solver._dy
    la = P.get("SAC_log_alpha")
    pos = _ordered_param_optimizers(solver)
    e_total, first = a_opt.epochs, solver.epoch
    for solver.epoch in range(first, first + e_total + 1):
        shuffle_device_(D, a_opt.shuffle_seed, solver.epoch)                                       # shuffle!(D_train) (:50)
        mb_infos = []
        for k0 in range(0, n, B):                                                                   # partition(1:length(D), batch_size) (:53)
            m = min(B, n - k0)
            mb.clear_(); mb.push_(D, ids=np.arange(k0 + 1, k0 + m + 1))                             # minibatch(D_train, batch) (:55)
            base = CTR_BLOCK * solver.grad_steps
            info = {}
            for theta, p in pos:                                                                    # :58-60
                _param_step(solver, theta, p, mb, base, info)
            y = None
            if solver.target_fn == "sac":                                                           # sac_target(pi) (batch/sac.jl: current actor, target critics)
                ctx.check(lib.crux_sac_target(A.h, pim.C.N1.h, pim.C.N2.h, la.h, mb.h, gamma, solver.noise_seed, base + CTR_TARGET, d_y)); y = d_y
            elif callable(solver.target_fn):
                yh = np.ascontiguousarray(np.asarray(solver.target_fn(pim, P, mb, gamma), np.float32).reshape(-1))
                ctx.h2d(d_y, yh); y = d_y
            elif solver.target_fn is not None:
                raise NotImplementedError("BatchSolver: target_fn %r" % (solver.target_fn,))
            if c_opt is not None:                                                                   # :66-71
                raw = np.zeros(L.INFO_N, np.float32)
                if c_opt.loss is advil_d_loss:                                                      # no target: y stays None
                    raw, adv = advil_d_step_(A, Q, mb, P["lambda_GP"], solver.noise_seed, base + CTR_ADVIL_GP)
                    info.update({"D_expert": float(adv[0]), "D_policy": float(adv[1]), "grad_pen": float(adv[2])})
                elif y is None:
                    raise NotImplementedError("BatchSolver: a critic without a target_fn has no device implementation")
                elif c_opt.loss is cql_critic_loss:
                    step = lib.crux_cql_critic_step_sigma if A.two_headed else lib.crux_cql_critic_step
                    ctx.check(step(A.h, Q.N1.h, Q.N2.h, P["CQL_log_alpha"].h, mb.h, y, int(P["CQL_n_action_samples"]), P["CQL_is_distribution"].lo,
                                   P["CQL_is_distribution"].hi, float(P["CQL_alpha_thresh"]), 1 if solver.weighted_loss else 0, solver.noise_seed,
                                   base + CTR_CQL_CRITIC, _vp(raw)))
                elif c_opt.loss is double_Q_loss:
                    ctx.check(lib.crux_double_q_step(Q.N1.h, Q.N2.h, mb.h, y, 1 if solver.weighted_loss else 0, _vp(raw)))
                else:
                    raise NotImplementedError("BatchSolver: critic loss %r has no device implementation" % getattr(c_opt.loss, "name", c_opt.loss))
                info.update({c_opt.name + "loss": float(raw[0]), c_opt.name + "grad_norm": float(raw[1])})
                if c_opt.loss is not advil_d_loss:
                    info.update({"Q1avg": float(raw[L.INFO["q1avg"]]), "Q2avg": float(raw[L.INFO["q2avg"]])})
                if solver.target_fn is not None:
                    if solver.target_update is None:
                        polyak_average_(pim, pi, np.float32(0.005))                                 # the default target_update (batch.jl:30)
                    else:
                        solver.target_update(pim, pi)
            if a_opt.loss is sac_actor_loss:                                                        # :74
                raw = np.zeros(L.INFO_N, np.float32)
                ctx.check(lib.crux_sac_actor_step(A.h, Q.N1.h, Q.N2.h, la.h, mb.h, solver.noise_seed, base + CTR_ACTOR, _vp(raw)))
                info.update({a_opt.name + "loss": float(raw[0]), a_opt.name + "grad_norm": float(raw[1]), "entropy": float(raw[L.INFO["entropy"]])})
            elif a_opt.loss is advil_pi_loss:                                                       # with the critic this minibatch has just updated
                raw, adv = advil_actor_step_(A, Q, mb, P["lambda_BC"], a_opt.regularizer.beta if a_opt.regularizer is not None else 0.0)
                info.update({a_opt.name + "loss": float(raw[0]), a_opt.name + "grad_norm": float(raw[1]), "bc_mse": float(adv[1]), "orth_reg": float(adv[2])})
            else:
                raise NotImplementedError("BatchSolver: actor loss %r has no device implementation with a critic" % getattr(a_opt.loss, "name", a_opt.loss))
            solver.grad_steps += 1
            mb_infos.append(info)
        solver.history.append(aggregate_info(mb_infos))                                             # :80
        if solver.early_stopping and solver.early_stopping(solver.history):                        # :83
            break
    return solver.agent.pi


def BatchSAC(pi, S, D_train, dN=50, SAC_alpha=1.0, SAC_H_target=None, SAC_alpha_opt=None, a_opt=None, c_opt=None, P=None, param_optimizers=None,
             normalize_training_data=True, **kw):
    """BatchSAC(; pi::ActorCritic{GaussianPolicy, DoubleNetwork}, S, dN=50, SAC_alpha=1f0, SAC_H_target=-dim(A), D_train, SAC_alpha_opt, a_opt, c_opt, P,
    param_optimizers, normalize_training_data=true) (src/model_free/batch/sac.jl:27-55). With normalize_training_data the solver trains on
    normalize!(deepcopy(D_train), S, action_space(pi)): the caller's buffer is left as it is. param_optimizers: extra (ParamVector, TrainingParams) pairs."""
    _check_actor_critic(pi, "BatchSAC")
    ad = pi.A.act_dim if pi.A.two_headed else pi.A.network.dims[-1]      # SAC_H_target = -dim(A): the action's rows, not the two-headed output's 2 ad
    A = PolicyParams(pi).space
    if normalize_training_data:
        D_train = normalize_(copy_buffer(D_train), S, A)
    Pd = {"SAC_log_alpha": ParamVector([np.log(np.float32(SAC_alpha))], ctx=pi.A.ctx), "SAC_H_target": np.float32(-ad if SAC_H_target is None else SAC_H_target)}
    Pd.update(P or {})
    t = dict(SAC_alpha_opt or {}); t.setdefault("name", "temp_")
    a = dict(a_opt or {}); a.setdefault("name", "actor_")
    c = dict(c_opt or {}); c.setdefault("name", "critic_"); c.setdefault("epochs", dN)
    c_loss = c.pop("loss", double_Q_loss)
    pos = [(Pd["SAC_log_alpha"], TrainingParams(loss=sac_temp_loss, **t))] + list(param_optimizers or [])
    return BatchSolver(agent=PolicyParams(pi, pi_minus=clone_policy(pi)), S=S, D_train=D_train, P=Pd, param_optimizers=pos,
                       a_opt=TrainingParams(loss=sac_actor_loss, **a), c_opt=TrainingParams(loss=c_loss, **c), target_fn="sac", **kw)


def CQL(pi, S, D_train, CQL_alpha=1.0, CQL_is_distribution=None, CQL_alpha_thresh=10.0, CQL_n_action_samples=10, CQL_alpha_opt=None, a_opt=None, c_opt=None, two_headed=False,
        **kw):
    """CQL(; pi, solver_type=BatchSAC, CQL_alpha=1f0, CQL_is_distribution=product(Uniform(-1, 1)), CQL_alpha_thresh=10f0, CQL_n_action_samples=10, CQL_alpha_opt,
    a_opt, c_opt) (src/model_free/batch/cql.jl): BatchSAC plus the parameter optimiser CQL_alpha_ on CQL_log_alpha and the critic loss
    double_Q_loss + conservative_loss. CQL_is_distribution: None (U(-1, 1)^ad) or a UniformBox; anything else is not implemented.
    two_headed=True: a two-headed actor (logSigma a network on mu's trunk, the SAC_A() of examples/offline rl/hopper_medium.jl) is taken; cql_alpha_loss and cql_critic_loss then
    go to the crux_cql_*_sigma entries. Without the keyword such an actor is refused by name, as before (core.require_two_headed_opt_in: tests/test_gpu_sigma_head.py::test_refusals
    asserts that refusal of the plain call). With a constant-logSigma actor the keyword changes nothing."""
    _check_actor_critic(pi, "CQL")
    if pi.A.two_headed and not two_headed:
        raise NotImplementedError("CQL: a %s whose logSigma is a network (two-headed actor) is taken by this solver only when it is asked for with two_headed=True "
                                  "(the sampled-action terms then draw from logSigma(s): crux_cql_*_sigma); SAC / BatchSAC take it as it is" % type(pi.A).__name__)
    if CQL_is_distribution is None:
        CQL_is_distribution = UniformBox(-1.0, 1.0)
    if not isinstance(CQL_is_distribution, UniformBox):
        raise NotImplementedError("CQL: CQL_is_distribution must be None or a UniformBox (a product of Uniform(lo, hi)); got %r" % (CQL_is_distribution,))
    n_s = int(CQL_n_action_samples)
    if n_s < 1:
        raise ValueError("CQL: CQL_n_action_samples must be >= 1")
    P = {"CQL_log_alpha": ParamVector([np.log(np.float32(CQL_alpha))], ctx=pi.A.ctx), "CQL_is_distribution": CQL_is_distribution,
         "CQL_n_action_samples": n_s, "CQL_alpha_thresh": np.float32(CQL_alpha_thresh)}
    ca = dict(CQL_alpha_opt or {}); ca.setdefault("name", "CQL_alpha_")
    c = dict(c_opt or {}); c["loss"] = cql_critic_loss; c.setdefault("name", "critic_")
    P.update(kw.pop("P", None) or {})
    pos = [(P["CQL_log_alpha"], TrainingParams(loss=cql_alpha_loss, **ca))] + list(kw.pop("param_optimizers", None) or [])
    return BatchSAC(pi, S, D_train, a_opt=a_opt, c_opt=c, P=P, param_optimizers=pos, **kw)


__all__ = ["BatchSAC", "CQL", "UniformBox", "cql_alpha_loss", "cql_critic_loss"]
