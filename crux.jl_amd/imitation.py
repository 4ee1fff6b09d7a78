"""imitation.py -- OnPolicyGAIL, NDA_GAIL_JS and the BatchSolver family (BC) (src/model_free/il/on_policy_gail.jl, il/nda_gail_js.jl, il/bc.jl, src/model_free/batch.jl).

Split out of api.py in round 4; `crux_jl_amd.api` re-exports everything, so `crux.X` and `crux.api.X` resolve as before."""
import ctypes as C
import math
import numpy as np
from . import _lib as L
from .core import refuse_chain_params, refuse_conv
from .core import refuse_two_headed, require_two_headed_opt_in   # noqa: F401
from .core import (  # noqa: F401
    ActorCritic, Adam, CartPoleMDP, Chain, Context, ContinuousNetwork, ContinuousSpace, CustomLoss, Dense, DiscreteNetwork, DiscreteSpace, DoubleNetwork, EpsGreedyPolicy,
    ExperienceBuffer, GaussianNoiseExplorationPolicy, GaussianPolicy, GymMDP, LinearDecaySchedule, MultitaskDecaySchedule, NetworkPolicy, ParamLoss, ParamVector, PendulumMDP,
    PolicyParams, SAMPLE_SEED, Sampler, SimpleGridWorld, SquashedGaussianPolicy, SynthMDP, TrainingParams, _F32_KEYS, _Loss, _batch_train_seam, _ensure_opt, _fill_block,
    _fill_importance_weights, _info_dict, _leaves, _np_dtype, _rollout_cfg, _train_cfg, _train_seam, _uses_seam, _vp, a2c_loss, actor, batch_train_, buffer_like, capacity,
    clone_policy, copy_buffer, copyto_, cost_value_mse_loss, critic, default_context, dim, discount, discounted_return, episodes, episodes_, extra_columns, failure, fill_gae_,
    fill_returns_, get_episodes, hcat, lagrange_ppo_loss, mdp_data, normalize_, peer_attach_local, polyak_average_, ppo_loss, prioritized_sample_, rand_, reinforce_loss,
    reload_switches, set_default_context, set_sample_stream_, shuffle_device_, split, split_batches, steps_, steps_multi_, train_, trim_, undiscounted_return, uniform_sample_,
    value, value_mse_loss, whiten_, whiten_multi_)
from .on_policy import (  # noqa: F401
    A2C, LagrangePPO, OnPolicySolver, PPO, REINFORCE, allreduce_mean_, policy_gradient_training, policy_gradient_training_multi, policy_gradient_training_synced, solve)


# --------------------------------------------------------------------------------------------------------------
# OnPolicyGAIL (src/model_free/il/on_policy_gail.jl) -- the discriminator is trained by batch_train! over TWO buffers (training.jl:28-44)
# --------------------------------------------------------------------------------------------------------------
class GANLoss:
    """The discriminator losses of src/extras/gans.jl (abstract type GANLoss, :1); `kind` is the C ABI's CRUX_GAN_* number."""
    kind, name = -1, ""

    def __repr__(self):
        return "GAN_%s()" % self.name


class GAN_BCELoss(GANLoss):      # gans.jl:5-9
    kind, name = 0, "BCELoss"


class GAN_LSLoss(GANLoss):       # gans.jl:12-14
    kind, name = 1, "LSLoss"


class GAN_HingeLoss(GANLoss):    # gans.jl:17-19
    kind, name = 2, "HingeLoss"


class GAN_WLoss(GANLoss):        # gans.jl:22-24
    kind, name = 3, "WLoss"


class GAN_WLossGP(GANLoss):
    """GAN_WLossGP(; λ = 10f0, noise_range = 1f0) (gans.jl:28-40): the Wasserstein loss + λ gradient_penalty(D, x_E, x_π). noise_range is carried and never read, as in
    the reference (:31). seed: the Philox seed of the penalty's draws ε (stream IQ_GP); the counter is the step count kept on the TrainingParams (gp_counter)."""
    kind, name = 4, "WLossGP"

    def __init__(self, λ=10.0, noise_range=1.0, seed=0):
        self.λ, self.noise_range, self.seed = float(np.float32(λ)), float(np.float32(noise_range)), int(seed)

    def __repr__(self):
        return "GAN_WLossGP(λ=%g, noise_range=%g, seed=%d)" % (self.λ, self.noise_range, self.seed)


GANLosses = {"BCE": GAN_BCELoss(), "LS": GAN_LSLoss(), "Hinge": GAN_HingeLoss(), "W": GAN_WLoss(), "WGP": GAN_WLossGP()}      # src/extras/gans.jl, exported by src/Crux.jl:83


class _GailDLoss(_Loss):
    """gail_d_loss(gan_loss) (on_policy_gail.jl:1-5): a loss that carries its GANLoss. The module-level object `gail_d_loss` is the BCE one, so TrainingParams(loss=gail_d_loss)
    means what it always did; calling it -- gail_d_loss(GAN_HingeLoss()) -- returns the loss of that kind."""

    def __init__(self, gan_loss=None):
        super().__init__("gail_d")
        self.gan_loss = gan_loss if gan_loss is not None else GAN_BCELoss()
        if not isinstance(self.gan_loss, GANLoss):
            raise TypeError("gail_d_loss: %r is not a GANLoss" % (gan_loss,))

    def __call__(self, gan_loss):
        return _GailDLoss(gan_loss)


gail_d_loss = _GailDLoss()     # gail_d_loss(GAN_BCELoss()) (on_policy_gail.jl:1-5, extras/gans.jl:7-9)


def _gan(p):
    """the GANLoss a TrainingParams' loss carries (BCE for anything that carries none)"""
    return getattr(p.loss, "gan_loss", None) or GAN_BCELoss()


def _gail_pairs(n_ex, n_pi, B):
    """zip(partition(1:n_ex, B), partition(1:n_pi, B)) (training.jl:40) as (offset, n_ex, n_pi): the shorter buffer ends the epoch"""
    nb = min(-(-n_ex // B), -(-n_pi // B))
    return [(k * B, min(B, n_ex - k * B), min(B, n_pi - k * B)) for k in range(nb)]


def batch_train_gail_d_(Dnet, p, D_expert, D_policy, info=None):
    """batch_train!(D, d_opt, (;), D_demo, deepcopy(D)) (on_policy_gail.jl:47, training.jl:28-55): every epoch shuffles both buffers, zips their
    minibatch partitions (the shorter buffer ends the epoch) and takes one discriminator step per pair. Shuffle k of this TrainingParams uses
    permutation counter 2k for the expert buffer and 2k+1 for the policy buffer. Epoch info = its last minibatch, result = mean over epochs.
    The loss kind is p.loss's (gail_d_loss(gan_loss)); BCE makes the calls it always made. GAN_WLossGP draws step t's ε from (gan_loss.seed, p.gp_counter), which advances
    by one per step taken, and needs equal halves in every pair: checked here for the whole epoch before any step (the reference throws DimensionMismatch in the
    first unequal pair, after the steps before it)."""
    refuse_conv(Dnet, "batch_train_gail_d_")
    _ensure_opt(Dnet, p)
    B, infos, total = p.batch_size, [], 0
    nb = min(-(-len(D_expert) // B), -(-len(D_policy) // B))
    gl = _gan(p)
    if gl.kind == GAN_WLossGP.kind:
        bad = [(ne, npi) for _, ne, npi in _gail_pairs(len(D_expert), len(D_policy), B) if ne != npi]
        if bad:
            raise ValueError("gail_d_loss(GAN_WLossGP): the gradient penalty needs as many expert rows as policy rows in every minibatch pair; buffers of %d and %d rows "
                             "under batch_size %d give a pair of %d and %d" % (len(D_expert), len(D_policy), B, bad[0][0], bad[0][1]))
    stop = False
    for _ in range(p.epochs):
        shuffle_device_(D_expert, p.shuffle_seed, 2 * p.shuffle_counter); shuffle_device_(D_policy, p.shuffle_seed, 2 * p.shuffle_counter + 1)
        p.shuffle_counter += 1
        raw = np.zeros(L.INFO_N, np.float32)
        for k in range(nb):
            ne, npi = min(B, len(D_expert) - k * B), min(B, len(D_policy) - k * B)
            if gl.kind == GAN_BCELoss.kind:
                Dnet.ctx.check(Dnet.ctx.lib.crux_gail_d_step(Dnet.h, D_expert.h, k * B, ne, D_policy.h, k * B, npi, _vp(raw)))
            else:
                Dnet.ctx.check(Dnet.ctx.lib.crux_gail_d_step_gan(Dnet.h, D_expert.h, k * B, ne, D_policy.h, k * B, npi, gl.kind, getattr(gl, "λ", 0.0), getattr(gl, "seed", 0),
                                                                 p.gp_counter, _vp(raw)))
                p.gp_counter += 1 if gl.kind == GAN_WLossGP.kind else 0
            total += 1
            if total >= p.max_batches:
                stop = True; break
        infos.append({p.name + "loss": float(raw[L.INFO["loss"]]), p.name + "grad_norm": float(raw[L.INFO["grad_norm"]])})
        if stop:
            break
    out = {k: float(np.mean([d[k] for d in infos])) for k in infos[0]}
    out[p.name + "batches_trained"] = total
    if info is not None:
        info.update(out)
    return out


def gail_reward_(Dnet, buf, alpha_r=0.5, Rscale=1.0):
    """r = ar*logsigmoid(D(a,s)) - (1-ar)*logcompsigmoid(D(a,s)); buf[:r] .= r .* Rscale; returns mean(r) (on_policy_gail.jl:50-55)."""
    refuse_conv(Dnet, "gail_reward_")
    m = np.zeros(1, np.float32)
    Dnet.ctx.check(Dnet.ctx.lib.crux_gail_reward(Dnet.h, buf.h, float(alpha_r), float(Rscale), _vp(m)))
    return float(m[0])


def OnPolicyGAIL(pi, S, gamma, D, demo, lambda_gae=0.95, alpha_r=0.5, normalize_demo=True, solver=None, d_opt=None, Rscale=1.0, gan_loss=None, **kw):
    """OnPolicyGAIL(; pi, S, gamma, lambda_gae, D_demo, alpha_r, normalize_demo, D::ContinuousNetwork, solver=PPO, gan_loss=GAN_BCELoss(), d_opt, Rscale)
    (src/model_free/il/on_policy_gail.jl:26-69): PPO whose post_batch_callback trains the discriminator on (demo, copy of the fresh batch),
    overwrites the rewards with the discriminator's, and refills GAE / returns / whitened advantages. gan_loss: one of GANLosses (None: GAN_BCELoss()); the reward
    does not depend on it (:51)."""
    refuse_conv(pi, "OnPolicyGAIL (pi)"); refuse_conv(D, "OnPolicyGAIL (D)")
    d = dict(d_opt or {}); d.setdefault("name", "discriminator_")
    dp = TrainingParams(loss=gail_d_loss if gan_loss is None else gail_d_loss(gan_loss), **d)
    A = pi.space if hasattr(pi, "space") else ContinuousSpace(actor(pi).network.dims[-1])
    demo = copy_buffer(demo)
    if normalize_demo:
        normalize_(demo, S, A)
    sv = (solver or PPO)(pi=pi, S=S, lambda_gae=lambda_gae, **kw)

    def GAIL_callback(buf, info):
        batch_train_gail_d_(D, dp, demo, copy_buffer(buf), info=info)                    # :47
        info["disc_reward"] = gail_reward_(D, buf, alpha_r, Rscale)                    # :50-56
        fill_gae_(buf, sv.agent.pi, lambda_gae, gamma); fill_returns_(buf, gamma)        # :58-63
        whiten_(buf, "advantage")                                                       # :64
    sv.post_batch_callback = GAIL_callback
    sv.discriminator, sv.d_opt, sv.demo = D, dp, demo
    return sv


# --------------------------------------------------------------------------------------------------------------
# NDA_GAIL_JS (src/model_free/il/nda_gail_js.jl) -- LagrangePPO whose post_batch_callback trains two discriminators and rewrites :r and :cost
# --------------------------------------------------------------------------------------------------------------
def _max_batches(p):
    return 0 if p.max_batches in (None, math.inf) else int(p.max_batches)


def _d_info(p, rows, raw):
    """aggregate_info over the epoch rows of a discriminator chain: epoch info = its last pair, result = mean over epochs"""
    e = int(raw[L.INFO["epochs_run"]]); rows = rows[:e]
    return {p.name + "loss": float(np.mean(rows[:, L.INFO["loss"]])), p.name + "grad_norm": float(np.mean(rows[:, L.INFO["grad_norm"]])),
            p.name + "batches_trained": int(raw[L.INFO["batches_trained"]])}


def batch_train_gail_d_chain_(Dnet, p, D_expert, D_policy, info=None):
    """batch_train_gail_d_ as one C call (crux_gail_d_batch_train; crux_gail_d_batch_train_gan for LS, hinge and W): the same shuffles, pairs and steps, bit for bit, with one
    host synchronisation. GAN_WLossGP is refused by the entry (CRUX_EUNSUP: the penalty takes its scratch per step); batch_train_gail_d_ is its path."""
    refuse_conv(Dnet, "batch_train_gail_d_chain_")
    _ensure_opt(Dnet, p)
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((p.epochs, L.INFO_N), np.float32)
    gl, lib = _gan(p), Dnet.ctx.lib
    try:
        if gl.kind == GAN_BCELoss.kind:
            Dnet.ctx.check(lib.crux_gail_d_batch_train(Dnet.h, D_expert.h, D_policy.h, p.batch_size, p.epochs, _max_batches(p), p.shuffle_seed, p.shuffle_counter, _vp(raw), _vp(rows)))
        else:
            Dnet.ctx.check(lib.crux_gail_d_batch_train_gan(Dnet.h, D_expert.h, D_policy.h, p.batch_size, p.epochs, _max_batches(p), p.shuffle_seed, p.shuffle_counter, gl.kind, _vp(raw), _vp(rows)))
    finally:
        p.shuffle_counter += int(raw[L.INFO["epochs_run"]]) if raw[L.INFO["epochs_run"]] > 0 else 0
    out = _d_info(p, rows, raw)
    if info is not None:
        info.update(out)
    out["_epoch_infos"] = rows[:int(raw[L.INFO["epochs_run"]])]
    return out


def nda_reward_cost_(Dnet, Dnda, buf, alpha_r=0.5):
    """buf[:r] and buf[:cost] from the two discriminators (nda_gail_js.jl:33-49, crux_nda_reward_cost); returns (mean(r), sum(c) / sum(episode_end), sum(episode_end))."""
    refuse_conv(Dnet, "nda_reward_cost_ (Dnet)"); refuse_conv(Dnda, "nda_reward_cost_ (Dnda)")
    out = np.zeros(3, np.float32)
    Dnet.ctx.check(Dnet.ctx.lib.crux_nda_reward_cost(Dnet.h, Dnda.h, buf.h, float(alpha_r), _vp(out)))
    return float(out[0]), float(out[1]), float(out[2])


def nda_advantages_(buf, V, Vc, lambda_gae, gamma):
    """fill_gae! / fill_returns! of :r and :cost with V and Vc and both whitens (nda_gail_js.jl:51-61) as one C call (crux_nda_advantages)."""
    refuse_conv(V, "nda_advantages_ (V)"); refuse_conv(Vc, "nda_advantages_ (Vc)")
    buf.ctx.check(buf.ctx.lib.crux_nda_advantages(buf.h, V.h, Vc.h, float(lambda_gae), float(gamma)))


def nda_gail_round_(Dnet, Dnda, dp, dpn, demo, nda, buf, copyD, copyN, V, Vc, alpha_r, lambda_gae, gamma, info=None):
    """The whole GAIL_callback (nda_gail_js.jl:28-63) as one C call (crux_nda_gail_round; crux_nda_gail_round_gan for LS, hinge and W, the kind of dp.loss for both
    discriminators); both shuffle counters advance by the epochs run."""
    refuse_conv(Dnet, "nda_gail_round_ (Dnet)"); refuse_conv(Dnda, "nda_gail_round_ (Dnda)"); refuse_conv(V, "nda_gail_round_ (V)"); refuse_conv(Vc, "nda_gail_round_ (Vc)")
    _ensure_opt(Dnet, dp); _ensure_opt(Dnda, dpn)
    rD, rN, out3 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
    gl, lib = _gan(dp), Dnet.ctx.lib
    head = (Dnet.h, Dnda.h, demo.h, nda.h, buf.h, copyD.h, copyN.h, V.h, Vc.h, dp.batch_size, dp.epochs, _max_batches(dp), dp.shuffle_seed, dp.shuffle_counter,
            dpn.batch_size, dpn.epochs, _max_batches(dpn), dpn.shuffle_seed, dpn.shuffle_counter, float(alpha_r), float(lambda_gae), float(gamma))
    try:
        if gl.kind == GAN_BCELoss.kind:
            Dnet.ctx.check(lib.crux_nda_gail_round(*head, _vp(rD), _vp(rN), _vp(out3)))
        else:
            Dnet.ctx.check(lib.crux_nda_gail_round_gan(*head, gl.kind, _vp(rD), _vp(rN), _vp(out3)))
    finally:
        for p, raw in ((dp, rD), (dpn, rN)):
            p.shuffle_counter += int(raw[L.INFO["epochs_run"]]) if raw[L.INFO["epochs_run"]] > 0 else 0
    info = info if info is not None else {}
    for p, raw in ((dp, rD), (dpn, rN)):      # the round hands back each chain's last epoch row (its last pair), not the mean over epochs batch_train_gail_d_chain_ forms
        info[p.name + "loss"], info[p.name + "grad_norm"] = float(raw[L.INFO["loss"]]), float(raw[L.INFO["grad_norm"]])
        info[p.name + "batches_trained"] = int(raw[L.INFO["batches_trained"]])
    info["disc_reward"], info["disc_nda_cost"] = float(out3[0]), float(out3[1])
    return info


def NDA_GAIL_JS(pi, S, D_demo, D_nda, Vc, gamma, D, Dnda, lambda_gae=0.95, alpha_r=0.5, normalize_demo=True, solver=None, d_opt=None, d_opt_nda=None, gan_loss=None, **kw):
    """NDA_GAIL_JS(; π, S, 𝒟_demo, 𝒟_nda, Vc, γ, λ_gae=0.95, αr=0.5, normalize_demo=true, D, Dnda, solver=LagrangePPO, gan_loss=GAN_BCELoss(), d_opt, d_opt_nda)
    (src/model_free/il/nda_gail_js.jl:1-65): the solver (LagrangePPO: cost critic Vc, :cost columns, PID penalty) with a post_batch_callback that trains D on
    (demonstrations, copy of the fresh batch) and Dnda on (negative demonstrations, another copy), sets :r from D, :cost = max(0, r_nda - r), and refills GAE, returns
    and both whitened advantages with the actor-critic's critic and Vc. The callback replaces the solver's own (the later keyword wins in the reference, :64) and is one
    C call (crux_nda_gail_round). Both demonstration buffers are copied, and normalised when asked; the caller's stay as they were.
    gan_loss: one kind for both discriminators (:19-20; None: GAN_BCELoss()). LS, hinge and W take the round's _gan form; GAN_WLossGP cannot run inside a chain, so its
    callback is the round's parts in turn: batch_train_gail_d_ per discriminator (a host loop of steps), nda_reward_cost_, nda_advantages_."""
    refuse_conv(pi, "NDA_GAIL_JS (pi)"); refuse_conv(Vc, "NDA_GAIL_JS (Vc)"); refuse_conv(D, "NDA_GAIL_JS (D)"); refuse_conv(Dnda, "NDA_GAIL_JS (Dnda)")
    d = dict(d_opt or {}); d.setdefault("name", "discriminator_")
    dn = dict(d_opt_nda or {}); dn.setdefault("name", "nda_discriminator_")
    loss = gail_d_loss if gan_loss is None else gail_d_loss(gan_loss)
    dp, dpn = TrainingParams(loss=loss, **d), TrainingParams(loss=loss, **dn)
    A = pi.space if hasattr(pi, "space") else ContinuousSpace(actor(pi).network.dims[-1])
    demo, nda = copy_buffer(D_demo), copy_buffer(D_nda)
    if normalize_demo:
        normalize_(demo, S, A); normalize_(nda, S, A)
    sv = (solver or LagrangePPO)(pi=pi, S=S, Vc=Vc, lambda_gae=lambda_gae, **kw)
    copies = []

    def GAIL_callback(buf, info):
        if _gan(dp).kind == GAN_WLossGP.kind:
            batch_train_gail_d_(D, dp, demo, copy_buffer(buf), info=info); batch_train_gail_d_(Dnda, dpn, nda, copy_buffer(buf), info=info)      # :29, :30
            info["disc_reward"], info["disc_nda_cost"], _ = nda_reward_cost_(D, Dnda, buf, alpha_r)                                             # :33-49
            nda_advantages_(buf, critic(sv.agent.pi), Vc, lambda_gae, gamma)                                                                     # :51-61
            return
        if not copies or copies[0].capacity < len(buf):
            copies[:] = [buffer_like(buf, capacity=buf.capacity), buffer_like(buf, capacity=buf.capacity)]      # the two deepcopy(𝒟) (:29, :30), refilled on the device every round
        nda_gail_round_(D, Dnda, dp, dpn, demo, nda, buf, copies[0], copies[1], critic(sv.agent.pi), Vc, alpha_r, lambda_gae, gamma, info=info)
    sv.post_batch_callback = GAIL_callback
    sv.discriminator, sv.nda_discriminator, sv.d_opt, sv.d_opt_nda, sv.demo, sv.nda = D, Dnda, dp, dpn, demo, nda
    return sv


mse_action_loss, logpdf_bc_loss = _Loss("mse_action"), _Loss("logpdf_bc")   # src/model_free/il/bc.jl:1,10-18


def loss_value(pi, p, P, D):
    """loss(pi, P, D) evaluated on the whole buffer, no update (the validation error of stop_on_validation_increase, src/utils.jl:59-72)."""
    refuse_conv(pi, "loss_value")
    _ensure_opt(pi, p)
    cfg = _train_cfg(pi, p, P); n = len(D)
    ids = np.arange(n, dtype=np.int64); raw = np.zeros(L.INFO_N, np.float32)
    pi.ctx.check(pi.ctx.lib.crux_loss_grad(pi.h, D.h, C.byref(cfg), _vp(ids), n, _vp(raw)))
    return float(raw[L.INFO["loss"]])


class BatchSolver:
    """BatchSolver(; agent, S, D_train, a_opt, c_opt, param_optimizers, target_fn, target_update, P, ...) (src/model_free/batch.jl:20-36).

    Without a critic and parameter optimisers (BC) solve runs the actor-only path below; otherwise the actor-critic loop of batch.py (BatchSAC, CQL).
    param_optimizers: a list of (ParamVector, TrainingParams) pairs; target_fn: "sac" or a callable (pi_minus, P, mb, gamma) -> y; target_update: None
    (polyak_average!(pi_minus, pi, 0.005)) or a callable (pi_minus, pi); grad_steps: the global minibatch index, continued across solve calls (it numbers
    the noise counters); gamma: the discount when solve is called without an mdp."""

    def __init__(self, agent, S, D_train, a_opt, P=None, early_stopping=None, max_steps=100, c_opt=None, param_optimizers=None, target_fn=None,
                 target_update=None, grad_steps=0, noise_seed=0, gamma=0.99, weighted_loss=False):
        refuse_chain_params("BatchSolver (BC / BatchSAC / CQL / AdVIL)", a_opt, c_opt, *[p for _, p in (param_optimizers or [])])
        self.agent, self.S, self.D_train, self.a_opt, self.P = agent, S, D_train, a_opt, dict(P or {})
        self.early_stopping, self.max_steps, self.epoch, self.history = early_stopping, int(max_steps), 0, []
        self.c_opt, self.param_optimizers, self.target_fn, self.target_update = c_opt, list(param_optimizers or []), target_fn, target_update
        self.grad_steps, self.noise_seed, self.gamma, self.weighted_loss = int(grad_steps), int(noise_seed), float(gamma), bool(weighted_loss)
        self._mb = self._dy = None        # staging buffer of one minibatch and its target column (device), made on first use


def _solve_batch(solver, mdp=None):
    """POMDPs.solve(S::BatchSolver, mdp) (src/model_free/batch.jl:38-85): per epoch shuffle!, partition, train! per minibatch (one persistent
    launch per epoch here), then the early-stopping test on the list of epoch infos. Note the inclusive range: a_opt.epochs + 1 epochs (:47).
    A solver with a critic or parameter optimisers runs the actor-critic loop of batch.py instead."""
    if getattr(solver, "c_opt", None) is not None or getattr(solver, "param_optimizers", None):
        from .batch import _solve_batch_ac
        return _solve_batch_ac(solver, mdp)
    A, p = actor(solver.agent.pi), solver.a_opt
    e_total, first = p.epochs, solver.epoch
    try:
        p.epochs = 1
        for solver.epoch in range(first, first + e_total + 1):
            info = batch_train_(A, p, solver.P, solver.D_train)
            solver.history.append({k: v for k, v in info.items() if not k.startswith("_")})
            if solver.early_stopping and solver.early_stopping(solver.history):
                break
    finally:
        p.epochs = e_total
    return solver.agent.pi


def stop_on_validation_increase(pi, P, D_val, p, window=5):
    """stop_on_validation_increase(pi, P, D_val, loss; window) (src/utils.jl:59-72)."""
    def f(infos):
        infos[-1]["validation_error"] = loss_value(pi, p, P, D_val)
        N = len(infos)
        if N >= 2 * window:
            cur = np.mean([infos[i]["validation_error"] for i in range(N - window, N)])
            old = np.mean([infos[i]["validation_error"] for i in range(N - 2 * window, N - window)])
            return bool(cur >= old)
        return False
    return f


def BC(pi, S, D_demo, normalize_demo=True, loss=None, validation_fraction=0.3, window=100, lambda_e=1e-3, opt=None, shuffle_perm=None, two_headed=False, **kw):
    """BC(; pi, S, D_demo, normalize_demo, loss, validation_fraction=0.3, window=100, lambda_e=1f-3, opt) (src/model_free/il/bc.jl:37-70):
    mse_action_loss for a ContinuousNetwork, logpdf_bc_loss otherwise; the demonstrations are normalised, shuffled once and split into
    training / validation parts; early stopping on the validation error. shuffle_perm: optional 1-based permutation for the initial shuffle!."""
    require_two_headed_opt_in(actor(pi), "BC", two_headed)      # (two_headed=True: a two-headed Gaussian actor with logpdf_bc_loss; without the keyword it is refused as before -- the keyword's only purpose, see core.require_two_headed_opt_in)
    loss = loss or (mse_action_loss if type(pi) is ContinuousNetwork else logpdf_bc_loss)
    if getattr(actor(pi), "two_headed", False) and (isinstance(loss, CustomLoss) or loss.name != "logpdf_bc"):      # a two-headed actor: logpdf_bc_loss only (k_pg_head_sigma)
        refuse_two_headed(actor(pi), "BC with %s" % ("a CustomLoss" if isinstance(loss, CustomLoss) else loss.name + "_loss"))
    A = pi.space if hasattr(pi, "space") else (DiscreteSpace(len(pi.outputs), pi.outputs) if isinstance(pi, DiscreteNetwork)
                                               else ContinuousSpace(getattr(pi, "act_dim", None) or pi.network.dims[-1]))
    D = buffer_like(D_demo, capacity=len(D_demo)); D.push_({k: D_demo[k] for k in D_demo.keys()})      # deepcopy(D_demo) (:52)
    if normalize_demo:
        normalize_(D, S, A)
    n = len(D)
    perm = np.asarray(shuffle_perm, np.int64) if shuffle_perm is not None else np.random.default_rng(0xBC).permutation(n).astype(np.int64) + 1
    D.shuffle_(perm)                                                                                    # shuffle!(D_demo) (:55)
    D_train, D_val = split(D, [1 - validation_fraction, validation_fraction])                         # (:56)
    P = {"lambda_e": lambda_e, "lambda_p": 1.0}
    o = dict(opt or {}); o.setdefault("name", "")
    p = TrainingParams(loss=loss, **o)
    return BatchSolver(agent=PolicyParams(pi), S=S, D_train=D_train, a_opt=p, P=P,
                       early_stopping=stop_on_validation_increase(pi, P, D_val, p, window=window), **kw)
