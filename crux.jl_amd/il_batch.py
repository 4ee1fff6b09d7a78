"""il_batch.py -- imitation learning on the batch solver: AdVIL (src/model_free/il/AdVIL.jl).

AdVIL is a BatchSolver over the demonstrations with a Wasserstein critic: the discriminator loss advil_d_loss (with gradient_penalty at target 0.4) and the actor loss
advil_pi_loss (a DPG-style step through the critic plus a BC term) with an OrthogonalRegularizer. Both train! calls are one C call each on the staging minibatch
(csrc/advil.hip: crux_advil_d_step, crux_advil_actor_step); the loop is the actor-critic loop of batch.py."""
import numpy as np

from . import _lib as L
from .core import refuse_conv
from .core import ActorCritic, ContinuousNetwork, OrthogonalRegularizer, PolicyParams, TrainingParams, _Loss, _vp, copy_buffer, normalize_
from .imitation import BatchSolver

advil_pi_loss, advil_d_loss = _Loss("advil_pi"), _Loss("advil_d")     # AdVIL.jl:1-4, :6-10

ADVIL_GP_TARGET = 0.4      # gradient_penalty(critic(pi), expert_sa, pi_sa, target=0.4f0) (AdVIL.jl:9)


def advil_d_step_(A, D, mb, lambda_GP, seed, counter, target=ADVIL_GP_TARGET):
    """train!(critic(pi), advil_d_loss) on the staging minibatch (crux_advil_d_step): returns the raw info row and [mean D(expert), mean D(pi), P, lambda_GP P]."""
    refuse_conv(A, "advil_d_step_ (A)"); refuse_conv(D, "advil_d_step_ (D)")
    raw, adv = np.zeros(L.INFO_N, np.float32), np.zeros(4, np.float32)
    D.ctx.check(D.ctx.lib.crux_advil_d_step(A.h, D.h, mb.h, float(np.float32(lambda_GP)), float(np.float32(target)), int(seed), int(counter), _vp(raw), _vp(adv)))
    return raw, adv


def advil_actor_step_(A, D, mb, lambda_BC, beta_orth):
    """train!(actor(pi), advil_pi_loss + OrthogonalRegularizer(beta_orth)) on the staging minibatch (crux_advil_actor_step): returns the raw info row and
    [mean D(s, pi(s)), mse, beta_orth reg]."""
    refuse_conv(A, "advil_actor_step_ (A)"); refuse_conv(D, "advil_actor_step_ (D)")
    raw, adv = np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
    D.ctx.check(D.ctx.lib.crux_advil_actor_step(A.h, D.h, mb.h, float(np.float32(lambda_BC)), float(np.float32(beta_orth)), _vp(raw), _vp(adv)))
    return raw, adv


def AdVIL(pi, S, D_demo, normalize_demo=True, lambda_GP=10.0, lambda_orth=1e-4, lambda_BC=0.2, a_opt=None, c_opt=None, **kw):
    """AdVIL(; π, S, 𝒟_demo, normalize_demo=true, λ_GP=10f0, λ_orth=1f-4, λ_BC=2f-1, a_opt, c_opt, kwargs...) (AdVIL.jl:30-54): a BatchSolver on
    normalize!(deepcopy(𝒟_demo), S, action_space(π)) (the caller's buffer is left as it is) with 𝒫 = (λ_GP, λ_BC), a_opt named actor_ with loss advil_pi_loss and
    regularizer OrthogonalRegularizer(λ_orth), c_opt named discriminator_ with loss advil_d_loss; no target_fn, no pi_minus and no parameter optimisers."""
    if not (isinstance(pi, ActorCritic) and isinstance(pi.A, ContinuousNetwork) and isinstance(pi.C, ContinuousNetwork)):
        raise TypeError("AdVIL: pi must be ActorCritic(ContinuousNetwork, ContinuousNetwork)")
    agent = PolicyParams(pi)
    d = copy_buffer(D_demo)
    if normalize_demo:
        normalize_(d, S, agent.space)
    a = {"name": "actor_", "loss": advil_pi_loss, "regularizer": OrthogonalRegularizer(lambda_orth)}; a.update(a_opt or {})
    c = {"name": "discriminator_", "loss": advil_d_loss}; c.update(c_opt or {})
    return BatchSolver(agent=agent, S=S, D_train=d, P={"lambda_GP": np.float32(lambda_GP), "lambda_BC": np.float32(lambda_BC)},
                       a_opt=TrainingParams(**a), c_opt=TrainingParams(**c), **kw)


__all__ = ["AdVIL", "advil_pi_loss", "advil_d_loss", "advil_d_step_", "advil_actor_step_", "ADVIL_GP_TARGET"]
