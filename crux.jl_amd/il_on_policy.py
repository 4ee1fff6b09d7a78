"""il_on_policy.py -- imitation learning on the on-policy solver: ASAF (src/model_free/il/asaf.jl).

ASAF is an OnPolicySolver without a critic and without a discriminator network: the policy is its own discriminator against a frozen copy piG of itself, taken in
post_batch_callback (asaf.jl:57). piG is constant for the whole batch_train!, so its log-densities over the fresh rollout (gG) and over the demonstrations (gE) are formed
once per iteration (crux_asaf_freeze) and the steps forward one network only (csrc/asaf.hip). Deviation from the reference, whose buffer has no extra column: the
solver's buffer carries a :logprob column that the freeze overwrites with gG, so that the epoch shuffles permute gG with the rows; gE lives in a device array of the
solver. The sampler's exploration log-density in that column is NOT gG (for the squashed policy it is the density of the pre-tanh sample, not of
atanh(clamp(a / ascale)) of the stored action) and is never used as such."""
import math

import numpy as np

from . import _lib as L
from .core import refuse_conv
from .core import ContinuousSpace, DiscreteNetwork, GaussianPolicy, PolicyParams, TrainingParams, _Loss, _ensure_opt, _vp, copy_buffer, normalize_
from .on_policy import OnPolicySolver

asaf_loss = _Loss("asaf")     # asaf_actor_loss(piG, D_demo) (asaf.jl:1-21)

ASAF_ROW = L.INFO_N + 4       # one epoch row of crux_asaf_batch_train: the info row, then entropy, the expert term, the policy term, one spare


def asaf_freeze_(pi, buf, d_out, first_row=0, n_rows=None):
    """d_out[i] = logpdf(pi, s_i, a_i) over rows [first_row, first_row + n_rows) of buf (crux_asaf_freeze); d_out: a device pointer, n_rows floats."""
    refuse_conv(pi, "asaf_freeze_")
    n = len(buf) - first_row if n_rows is None else n_rows
    pi.ctx.check(pi.ctx.lib.crux_asaf_freeze(pi.h, buf.h, int(first_row), int(n), d_out))


def _clip(clip_value):
    return 0.0 if clip_value is None else float(np.float32(clip_value))


def asaf_actor_step_(pi, buf, off, n, d_gG, demo, d_gE, clip_value=None):
    """train!(actor(pi), asaf_actor_loss) on rows [off, off + n) of buf (0-based) and all rows of demo (crux_asaf_actor_step): returns the raw info row and
    [entropy, the expert term, the policy term]. d_gG is aligned with buf's rows, d_gE with demo's."""
    refuse_conv(pi, "asaf_actor_step_")
    raw, out = np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
    pi.ctx.check(pi.ctx.lib.crux_asaf_actor_step(pi.h, buf.h, int(off), int(n), d_gG, demo.h, d_gE, _clip(clip_value), _vp(raw), _vp(out)))
    return raw, out


class _DeviceVec:
    """n floats of device memory, freed with its owner"""

    def __init__(self, ctx, n):
        self.ctx, self.n, self.p = ctx, int(n), ctx.alloc(4 * int(n))

    def get(self):
        return self.ctx.d2h(self.p, np.empty(self.n, np.float32))

    def __del__(self):
        try:
            if self.p and self.ctx.h:
                self.ctx.free(self.p)
        except Exception:
            pass


def batch_train_asaf_(solver, D, info=None):
    """batch_train!(actor(pi), a_opt, P, D) (training.jl:28-55) with asaf_actor_loss, as one C call (crux_asaf_batch_train): per epoch the device shuffle
    (a_opt.shuffle_seed, a_opt.shuffle_counter), then one step per minibatch; gG is D[:logprob] as the freeze left it, gE the solver's device array. Epoch info = its
    last minibatch, result = mean over epochs (aggregate_info)."""
    pi, p = solver.agent.pi, solver.a_opt
    _ensure_opt(pi, p)
    mb = 0 if p.max_batches in (None, math.inf) else int(p.max_batches)
    raw, rows = np.zeros(L.INFO_N, np.float32), np.zeros((p.epochs, ASAF_ROW), np.float32)
    try:
        pi.ctx.check(pi.ctx.lib.crux_asaf_batch_train(pi.h, D.h, solver.demo.h, solver.gE.p, p.batch_size, p.epochs, mb, p.shuffle_seed, p.shuffle_counter,
                                                      _clip(solver.clip_value), _vp(raw), _vp(rows)))
    finally:
        p.shuffle_counter += int(raw[L.INFO["epochs_run"]]) if raw[L.INFO["epochs_run"]] > 0 else 0
    e = int(raw[L.INFO["epochs_run"]]); rows = rows[:e]
    out = {p.name + "loss": float(np.mean(rows[:, L.INFO["loss"]])), p.name + "grad_norm": float(np.mean(rows[:, L.INFO["grad_norm"]])),
           "entropy": float(np.mean(rows[:, L.INFO_N]))}
    out[p.name + "batches_trained"] = int(raw[L.INFO["batches_trained"]])
    info = info if info is not None else {}
    info.update(out)
    info["_epochs_run"], info["_epoch_infos"] = e, rows
    return info


def ASAF(pi, S, D_demo, normalize_demo=True, dN=50, lambda_orth=1e-4, a_opt=None, c_opt=None, clip_value=None, log=None, required_columns=(), two_headed=False, **kw):
    """ASAF(; π, S, 𝒟_demo, normalize_demo=true, ΔN=50, λ_orth=1f-4, a_opt, c_opt, log, kwargs...) (asaf.jl:40-61): an OnPolicySolver with no critic whose
    post_batch_callback freezes the policy; a_opt is named actor_ with loss asaf_loss. lambda_orth and c_opt are accepted and unused, as in the reference.
    normalize_demo normalises a copy of the demonstrations (the caller's buffer stays as it was). clip_value: element-wise gradient clamp before Adam
    (Optimiser(ClipValue(c), Adam), examples/il/pendulum.jl); None = off. log: a dict of LoggerParams arguments over the reference's defaults dir="log/ASAF",
    period=100 ({} for exactly those); None, as for every solver here, logs nothing.
    The freeze writes gG = logpdf(piG, s, a) into the buffer's :logprob column (see the module docstring) and gE into solver.gE.
    two_headed=True: a policy whose logSigma is a network on mu's trunk is taken (csrc/asaf.hip: k_asaf_logpdf_sigma, k_asaf_head_sigma); the freeze and batch_train_asaf_ go
    through the same entries, and the Sampler rolls such a policy out on the generic kernels. Without the keyword it is refused by name, as before
    (core.require_two_headed_opt_in: tests/test_gpu_sigma_pg.py::test_host_mirror_refuses_by_name asserts that refusal of the plain call)."""
    if isinstance(pi, DiscreteNetwork):
        raise NotImplementedError("ASAF: the categorical head (DiscreteNetwork) is not implemented; the policy must be a GaussianPolicy or SquashedGaussianPolicy")
    if not isinstance(pi, GaussianPolicy):
        raise TypeError("ASAF: pi must be a GaussianPolicy or SquashedGaussianPolicy (logpdf and entropy are needed)")
    two = getattr(pi, "two_headed", False)
    if two and not two_headed:
        raise NotImplementedError("ASAF: a %s whose logSigma is a network (two-headed actor) is taken by this solver only when it is asked for with two_headed=True; "
                                  "SAC / BatchSAC take it as it is" % type(pi).__name__)
    agent = PolicyParams(pi, space=ContinuousSpace(pi.act_dim if two else pi.network.dims[-1]))
    demo = copy_buffer(D_demo)
    if normalize_demo:
        normalize_(demo, S, agent.space)
    a = {"name": "actor_", "loss": asaf_loss}; a.update(a_opt or {})
    if log is not None:
        from .logging import LoggerParams
        lg = {"dir": "log/ASAF", "period": 100}; lg.update(log)
        kw["log"] = LoggerParams(**lg)
    cols = list(dict.fromkeys(list(required_columns) + ["logprob"]))
    sv = OnPolicySolver(agent=agent, S=S, dN=dN, a_opt=TrainingParams(**a), c_opt=None, required_columns=cols, two_headed=bool(two_headed), **kw)
    sv.demo, sv.gE, sv.clip_value, sv.lambda_orth = demo, _DeviceVec(pi.ctx, max(len(demo), 1)), clip_value, lambda_orth

    def freeze(D, info):                                                        # S.a_opt.loss = asaf_actor_loss(deepcopy(S.agent.pi), D_demo) (:57)
        asaf_freeze_(pi, D, D.column_ptr("logprob"))
        asaf_freeze_(pi, sv.demo, sv.gE.p)
    sv.post_batch_callback = freeze
    return sv


__all__ = ["ASAF", "asaf_loss", "asaf_freeze_", "asaf_actor_step_", "batch_train_asaf_", "ASAF_ROW"]
