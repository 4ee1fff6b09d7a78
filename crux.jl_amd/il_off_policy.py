"""il_off_policy.py -- off-policy imitation learning: OnlineIQLearn and SQIL (src/model_free/il/iqlearn.jl, il/sqil.jl), gradient_penalty
(src/extras/gradient_penalty.jl), OffPolicyGAIL (il/off_policy_gail.jl) and AdRIL (il/AdRIL.jl).

Both constructors add a normalised copy of the demonstrations to an off-policy solver as an extra buffer drawn at buffer_fractions = [1/2, 1/2]. The staging
minibatch is then laid out by split_batches as B_p buffer rows followed by B - B_p demo rows, so where the reference marks demo rows with a Bool :expert column
(iq_callback, required_columns=[:expert]) this module passes B_p to the critic step instead: the reference's column is false on every buffer row and true on every
demo row. No buffer column is added. iq_loss's critic step, the penalty and its second-order pass are HIP (csrc/iq.hip: crux_iq_step, crux_gradient_penalty).

OffPolicyGAIL's callback (discriminator epochs on freshly drawn rows of every source, then the reward rewrite of the staging batch) is one C call,
crux_offgail_round; AdRIL's rewrite of the ring's rewards is crux_adril_relabel, run on the device through OffPolicySolver.post_sample_device (csrc/gail_off.hip)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .logging import aggregate_info
from .core import (ContinuousNetwork, ContinuousSpace, DiscreteNetwork, DiscreteSpace, ExperienceBuffer, TrainingParams, _Loss, _ensure_opt, _vp, copy_buffer, normalize_,
                   split_batches)
from .core import refuse_conv
from .core import refuse_two_headed
from .off_policy import SAC, SoftQ


class _IqLoss(_Loss):
    """iq_loss(; gamma=0.9, reg=true, alpha_reg=0.5, gp=true, lambda_gp=10) (iqlearn.jl:49-95): the marker value_training routes to crux_iq_step."""

    def __init__(self, gamma, reg, alpha_reg, gp, lambda_gp):
        super().__init__("iq")
        self.gamma, self.reg, self.alpha_reg = float(np.float32(gamma)), bool(reg), float(np.float32(alpha_reg))
        self.gp, self.lambda_gp = bool(gp), float(np.float32(lambda_gp))


def iq_loss(gamma=0.9, reg=True, alpha_reg=0.5, gp=True, lambda_gp=10.0):
    """iq_loss(; γ=0.9f0, reg=true, α_reg=0.5f0, gp=true, λ_gp=10f0) (iqlearn.jl:49). γ is the loss's own discount, not the MDP's; soft values use alpha = 1."""
    return _IqLoss(gamma, reg, alpha_reg, gp, lambda_gp)


def _dev_cols(ctx, a):
    a = np.asfortranarray(np.asarray(a, np.float32))
    if a.ndim != 2:
        raise ValueError("gradient_penalty: states are (features, batch) arrays")
    d = ctx.alloc(4 * a.size); ctx.h2d(d, a)
    return d, a.shape


def gradient_penalty(net, x, xtilde=None, target=1.0, seed=0, counter=0):
    """gradient_penalty(D, x[, xtilde]; target=1f0) (extras/gradient_penalty.jl): mean over columns of (|d sum(D(xhat)) / d xhat| - target)^2 with
    xhat = eps xtilde + (1 - eps) x, eps_j ~ U(0, 1) per column (include/crux_rng.h, IQ_GP; xtilde=None: xhat = x). Returns the value.

    The draws are a pure function of (seed, counter): calls with the same pair interpolate with the same eps. The reference draws fresh uniforms on every call,
    so a caller that wants that must pass a counter of its own per call (OnlineIQLearn passes noise_seed and i epochs + epoch)."""
    refuse_conv(net, "gradient_penalty")
    ctx = net.ctx
    d_in = net.network.dims[0]
    for name, v in (("x", x), ("xtilde", xtilde)):
        if v is not None and (np.ndim(v) != 2 or np.shape(v)[0] != d_in):
            raise ValueError("gradient_penalty: %s has shape %s, the network expects (%d, batch)" % (name, np.shape(v), d_in))
    dx, shp = _dev_cols(ctx, x); dxt = None
    try:
        if xtilde is not None:
            dxt, shp2 = _dev_cols(ctx, xtilde)
            if shp2 != shp:
                raise ValueError("gradient_penalty: x and xtilde differ in shape (%s, %s)" % (shp, shp2))
        out = np.zeros(1, np.float32)
        ctx.check(ctx.lib.crux_gradient_penalty(net.h, dx, dxt, shp[1], float(np.float32(target)), 1.0, 0, int(seed), int(counter), _vp(out)))
        return float(out[0])
    finally:
        ctx.free(dx)
        if dxt is not None:
            ctx.free(dxt)


def _demo_buffer(demo, S, A, normalize_demo):
    """normalize_demo && (D_demo = normalize!(deepcopy(D_demo), S, A)): the caller's buffer is never modified"""
    d = copy_buffer(demo)
    if normalize_demo:
        normalize_(d, S, A)
    return d


def _space(pi, demo):
    """action_space(pi): a DiscreteNetwork's own; for the continuous policies of SAC a unit ContinuousSpace, which leaves the demo actions unchanged"""
    return DiscreteSpace(len(pi.outputs), pi.outputs) if isinstance(pi, DiscreteNetwork) else ContinuousSpace(demo.act_dim)


def OnlineIQLearn(pi, S, demo, gamma=0.9, normalize_demo=True, solver=SoftQ, reg=True, alpha_reg=0.5, gp=True, lambda_gp=10.0, **kw):
    """OnlineIQLearn(; π, S, 𝒟_demo, γ=0.9f0, normalize_demo=true, solver=SoftQ, reg=true, α_reg=0.5f0, gp=true, λ_gp=10f0, kwargs...) (iqlearn.jl:98-138):
    `solver` with the demonstrations as an extra buffer at [1/2, 1/2], c_opt.loss = iq_loss(...) and no target (target_fn returns nothing). Only SoftQ:
    the reference defines soft_value for a DiscreteNetwork alone. The penalty interpolates between the two halves of the minibatch, so an odd batch size
    (or any split other than half and half) is refused."""
    if solver is SAC:
        raise NotImplementedError("OnlineIQLearn with SAC: iq_loss needs soft_value, which the reference defines for a DiscreteNetwork only (softq.jl:7)")
    if not isinstance(pi, DiscreteNetwork):
        raise NotImplementedError("OnlineIQLearn: pi must be a DiscreteNetwork (iq_loss uses soft_value(pi, s), softq.jl:7)")
    c = dict(kw.pop("c_opt", None) or {})
    bs = int(c.get("batch_size", 128))
    if bs % 2:
        raise ValueError("OnlineIQLearn: batch_size %d is odd; the gradient penalty pairs every demo row with a policy row" % bs)
    d = _demo_buffer(demo, S, _space(pi, demo), normalize_demo)
    sv = solver(pi=pi, S=S, c_opt=c, extra_buffers=[d], buffer_fractions=[0.5, 0.5], **kw)
    sv.c_opt.loss = iq_loss(gamma=gamma, reg=reg, alpha_reg=alpha_reg, gp=gp, lambda_gp=lambda_gp)
    sv.target_fn = None                  # target_fn = (args...; kwargs...) -> nothing
    sv.demo = d
    return sv


def _value_training_iq(solver, D, gamma):
    """value_training(S, D, gamma) (off_policy.jl:66-111) when c_opt.loss is iq_loss: per epoch rand! -> post_batch_callback -> train!(Q, iq_loss) (no target,
    no priorities); then the final target update (:108). Philox counters: sampling i epochs + epoch (as every value_training), penalty draws noise_seed with the same
    counter. Info keys as the reference's train! and iq_loss name them."""
    pi, p, ctx, lo = solver.agent.pi, solver.c_opt, solver.buffer.ctx, solver.c_opt.loss
    _ensure_opt(pi, p)
    B = D.capacity
    fr = [0.0 if len(b) == 0 else f for b, f in zip(solver._sources(), solver.buffer_fractions)]
    n_policy = split_batches(B, [f / sum(fr) for f in fr])[0]
    infos = []
    for epoch in range(p.epochs):
        ctr = solver.i * p.epochs + epoch
        info = {}
        solver._rand(D, ctr)                                                                           # :71
        if solver.post_batch_callback is not None:
            solver.post_batch_callback(D, S=solver, info=info)                                         # :77
        if epoch % p.update_every == 0:                                                                # :91
            raw, iq = np.zeros(L.INFO_N, np.float32), np.zeros(6, np.float32)
            ctx.check(ctx.lib.crux_iq_step(pi.h, D.h, n_policy, lo.gamma, 1 if lo.reg else 0, lo.alpha_reg, 1 if lo.gp else 0, lo.lambda_gp,
                                           solver.noise_seed, ctr, _vp(raw), _vp(iq)))
            info.update({"softQloss": float(iq[0]), "valueloss": float(iq[1]), "avg_R_expert_IQ": float(iq[2]), "avg_R_demo_IQ": float(iq[3])})
            if lo.gp:
                info["grad_pen"] = float(iq[4])
            if lo.reg:
                info["reg_loss"] = float(iq[5])
            info.update({p.name + "loss": float(raw[L.INFO["loss"]]), p.name + "grad_norm": float(raw[L.INFO["grad_norm"]])})
        infos.append(info)
    solver._update_target(final=True)                                                                  # :108
    return aggregate_info(infos)


def sqil_callback(D, S=None, info=None):
    """sqil_callback(D; kwargs...) = D[:r] .= 0 (sqil.jl:1-3): the freshly sampled rows get reward 0, the demonstrations keep theirs."""
    D["r"][...] = 0


def SQIL(pi, S, demo, normalize_demo=True, solver=SAC, **kw):
    """SQIL(; π, S, 𝒟_demo, normalize_demo=true, solver=SAC, kwargs...) (sqil.jl:20-39): `solver` (SAC or SoftQ) with post_sample_callback = sqil_callback and the
    demonstrations, which must carry :r, as an extra buffer at [1/2, 1/2]."""
    if not demo.haskey("r"):
        raise ValueError("SQIL requires a reward value for the demonstrations")
    refuse_two_headed(pi, "SQIL")
    d = _demo_buffer(demo, S, _space(pi, demo), normalize_demo)
    sv = solver(pi=pi, S=S, post_sample_callback=sqil_callback, extra_buffers=[d], buffer_fractions=[0.5, 0.5], **kw)
    sv.demo = d
    return sv


def _handles(bufs):
    return (C.c_void_p * len(bufs))(*[b.h for b in bufs])


def offgail_d_step_(D, sources, Bd, seed, counter):
    """One discriminator step of OffPolicyGAIL (off_policy_gail.jl:65-98) over `sources` = [demo, buffer, ndas...]: returns the raw info row (crux_offgail_d_step)."""
    refuse_conv(D, "offgail_d_step_")
    raw = np.zeros(L.INFO_N, np.float32)
    D.ctx.check(D.ctx.lib.crux_offgail_d_step(D.h, _handles(sources), len(sources), int(Bd), int(seed), int(counter), _vp(raw)))
    return raw


def offgail_round_(D, sources, Bd, d_epochs, batch, seed, counter0):
    """GAIL_callback (off_policy_gail.jl:64-125) as one call: d_epochs discriminator steps, then batch[:r] rewritten; returns the last step's raw info row."""
    refuse_conv(D, "offgail_round_")
    raw = np.zeros(L.INFO_N, np.float32)
    D.ctx.check(D.ctx.lib.crux_offgail_round(D.h, _handles(sources), len(sources), int(Bd), int(d_epochs), batch.h, int(seed), int(counter0), _vp(raw)))
    return raw


def offgail_reward_(D, batch, K):
    """batch[:r] .= sum((log.(softmax(D(s, a)) .+ 1f-5) .- log.(1f0 .- softmax(D(s, a)) .+ 1f-5)) .* w, dims=1) (off_policy_gail.jl:121-124); returns mean(r)."""
    refuse_conv(D, "offgail_reward_")
    out = np.zeros(1, np.float32)
    D.ctx.check(D.ctx.lib.crux_offgail_reward(D.h, batch.h, int(K), _vp(out)))
    return float(out[0])


def offgail_gather(sources, Bd, seed, counter):
    """The columns X = vcat(s, a) one discriminator step with (seed, counter) forms, source k in columns [k Bd, (k + 1) Bd) (crux_offgail_gather)."""
    ctx, K = sources[0].ctx, len(sources)
    sd = sources[0].obs_dim + sources[0].act_dim
    X = np.empty((sd, K * int(Bd)), np.float32, order="F")
    d = ctx.alloc(4 * X.size)
    try:
        ctx.check(ctx.lib.crux_offgail_gather(_handles(sources), K, int(Bd), int(seed), int(counter), d))
        ctx.d2h(d, X)
    finally:
        ctx.free(d)
    return X


def adril_relabel_(buf, n_new, buffer_init, dN):
    """AdRIL_callback (AdRIL.jl:39-50) on the ring after the push of its n_new newest rows (crux_adril_relabel); returns (max_i, k)."""
    mx, k = C.c_int64(), C.c_int64()
    buf.ctx.check(buf.ctx.lib.crux_adril_relabel(buf.h, int(n_new), int(buffer_init), int(dN), C.byref(mx), C.byref(k)))
    return mx.value, k.value


def OffPolicyGAIL(pi, S, demo, D, ndas=(), normalize_demo=True, solver=SAC, d_opt=None, **kw):
    """OffPolicyGAIL(; π, S, 𝒟_demo, 𝒟_ndas=[], normalize_demo=true, D::ContinuousNetwork, solver=SAC, d_opt=(epochs=5,), kwargs...) (off_policy_gail.jl:18-129):
    `solver` with post_batch_callback = GAIL_callback. After every rand! of value_training the callback runs d_opt.epochs discriminator steps, each over
    d_opt.batch_size freshly drawn rows of the demonstrations, the solver's buffer and every NDA buffer (logitcrossentropy over 2 + N_nda classes), and then
    replaces the staging batch's rewards by the discriminator's: one crux_offgail_round. Draws: key solver.sample_seed, counters round * epochs + epoch with a
    round counter kept on the solver (`gail_rounds`, continued across solve calls), streams 16 + k (include/crux_rng.h).

    Works with every solver whose value_training honours post_batch_callback (SAC, DDPG / TD3, DQN / SoftQ). Deviation: normalize_demo=False with NDA buffers
    is allowed and leaves them as they are; the reference assigns `false` to 𝒟_ndas[i] in that case (:44), which fails at the first rand!."""
    refuse_conv(pi, "OffPolicyGAIL (pi)"); refuse_conv(D, "OffPolicyGAIL (D)")
    refuse_two_headed(pi, "OffPolicyGAIL")
    d = dict(d_opt or {}); d.setdefault("epochs", 5); d.setdefault("name", "discriminator_")
    dp = TrainingParams(loss=None, **d)                                                                  # loss = () -> nothing (:31)
    ndas = list(ndas)
    K = 2 + len(ndas)
    if not isinstance(D, ContinuousNetwork):
        raise TypeError("OffPolicyGAIL: D must be a ContinuousNetwork")
    sd = demo.obs_dim + demo.act_dim
    if D.network.dims[0] != sd or D.network.dims[-1] != K:
        raise ValueError("OffPolicyGAIL: D must map vcat(s, a) (%d) to 2 + length(ndas) = %d outputs, not %d -> %d" % (sd, K, D.network.dims[0], D.network.dims[-1]))
    A = _space(pi.A if hasattr(pi, "A") else pi, demo)
    dm = _demo_buffer(demo, S, A, normalize_demo)
    nd = [_demo_buffer(b, S, A, normalize_demo) for b in ndas]
    sv = solver(pi=pi, S=S, **kw)
    if sv.buffer.isprioritized():
        raise NotImplementedError("OffPolicyGAIL with a prioritized buffer: the discriminator's rand! would go through prioritized_sample! and rewrite :weight")
    sv.gail_rounds = 0

    def GAIL_callback(batch, S=None, info=None):
        _ensure_opt(D, dp)
        raw = offgail_round_(D, [dm, sv.buffer] + nd, dp.batch_size, dp.epochs, batch, sv.sample_seed, sv.gail_rounds * dp.epochs)
        sv.gail_rounds += 1
        if info is not None:
            info[dp.name + "loss"] = float(raw[L.INFO["loss"]]); info[dp.name + "grad_norm"] = float(raw[L.INFO["grad_norm"]])
    sv.post_batch_callback = GAIL_callback
    sv.discriminator, sv.d_opt, sv.demo, sv.ndas = D, dp, dm, nd
    return sv


def AdRIL(pi, S, demo, dN=50, solver=SAC, normalize_demo=True, expert_frac=0.5, buffer_size=1000, buffer_init=0, buffer=None, **kw):
    """AdRIL(; π, S, ΔN=50, solver=SAC, 𝒟_demo, normalize_demo=true, expert_frac=0.5, buffer_size=1000, buffer_init=0, buffer=ExperienceBuffer(S, A, buffer_size, [:i]),
    kwargs...) (AdRIL.jl:20-64): `solver` with the demonstrations, which must carry :r, as an extra buffer at [1 - expert_frac, expert_frac] and AdRIL_callback after every
    steps!: fresh rows get reward 0, rows at least ΔN iterations old -1/k. The rewrite covers the whole ring, so it runs on the device (post_sample_device ->
    crux_adril_relabel) instead of through post_sample_callback's host copies."""
    if not demo.haskey("r"):
        raise ValueError("AdRIL requires a reward value for the demonstrations")
    refuse_two_headed(pi, "AdRIL")
    A = _space(pi.A if hasattr(pi, "A") else pi, demo)
    d = _demo_buffer(demo, S, A, normalize_demo)
    if buffer is None:
        buffer = ExperienceBuffer(S, A, buffer_size, ["i"], ctx=demo.ctx)
    sv = solver(pi=pi, S=S, dN=dN, extra_buffers=[d], buffer_fractions=[1 - expert_frac, expert_frac], buffer_size=buffer_size, buffer_init=buffer_init, buffer=buffer, **kw)
    b0 = int(buffer_init)

    def AdRIL_callback(solver_, n_new, info):
        adril_relabel_(solver_.buffer, n_new, b0, dN)
    sv.post_sample_device = AdRIL_callback
    sv.demo = d
    return sv
