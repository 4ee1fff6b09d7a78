"""Float64 restatement of what NDA-GAIL-JS's callback computes (src/model_free/il/nda_gail_js.jl:28-63): the yardstick of tests/test_gpu_nda_gail.py.

  gail_d_loss(GAN_BCELoss())   on_policy_gail.jl:1-5, extras/gans.jl:7-9: logitbinarycrossentropy(D(a_E, s_E), 1) + logitbinarycrossentropy(D(a_pi, s_pi), 0), each
                               a mean over its half; torch autograd gives the gradient (the closed-form seeds (sigmoid - 1) / n_ex and sigmoid / n_pi of csrc/sac.hip
                               do not appear here)
  reward, cost                 :34, :43, :44: r = ar logsigmoid(z) - (1 - ar) logcompsigmoid(z), logcompsigmoid(z) = logsigmoid(z) - z (utils.jl:140-143),
                               c = max(0, r_nda - r)
  gae_returns                  fill_gae! / fill_returns! over episodes() (sampler.jl:255-281, experience_buffer.jl:194-212), a trailing open episode closed at the end
  whiten                       (v - mean(v)) / std(v) with Bessel's correction (utils.jl:41-42)
  partition_plan               batch_train! over two buffers (training.jl:28-55): per epoch the zipped partitions, the shorter buffer ends the epoch, max_batches
"""
import numpy as np
import torch

import cql_reference as CR

mlp_params, mlp, flat_grad, adam_first_step = CR.mlp_params, CR.mlp, CR.flat_grad, CR.adam_first_step


def _t(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def vcat_as(a, s):
    """vcat(a, s): the ACTION first (value(D, a, s), :33); one-hot Bool actions enter as 0/1"""
    return np.vstack([np.asarray(a, np.float64), np.asarray(s, np.float64)])


def d_out(p, dims, acts, a, s):
    """D(vcat(a, s)) as plain float64 numbers: [n]"""
    with torch.no_grad():
        return mlp(mlp_params(p, dims), acts, _t(vcat_as(a, s)))[0].numpy()


def logsigmoid(z):
    return -np.logaddexp(0.0, -np.asarray(z, np.float64))


def gail_d_loss(layers, acts, a_ex, s_ex, a_pi, s_pi):
    """Lᴰ of GAN_BCELoss over the two halves: a torch scalar"""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    ze, zp = mlp(layers, acts, _t(vcat_as(a_ex, s_ex)))[0], mlp(layers, acts, _t(vcat_as(a_pi, s_pi)))[0]
    return bce(ze, torch.ones_like(ze)) + bce(zp, torch.zeros_like(zp))


def d_step(p, dims, acts, a_ex, s_ex, a_pi, s_pi):
    """loss and the flat float64 gradient of one discriminator step"""
    layers = mlp_params(p, dims)
    loss = gail_d_loss(layers, acts, a_ex, s_ex, a_pi, s_pi)
    loss.backward()
    return loss.item(), flat_grad(layers)


def reward(z, alpha_r):
    """r = ar logsigmoid(z) - (1 - ar) logcompsigmoid(z) (:34); ar is the Float32 the reference holds"""
    ar = float(np.float32(alpha_r)); ls = logsigmoid(z)
    return ar * ls - (1.0 - ar) * (ls - np.asarray(z, np.float64))


def hinge_cost(r, r_nda):
    """c = max.(0, r_nda .- r) (:44)"""
    return np.maximum(0.0, np.asarray(r_nda, np.float64) - np.asarray(r, np.float64))


def episodes(episode_end):
    """0-based inclusive (start, stop) pairs from :episode_end; a trailing open episode is closed at the last row"""
    ee = np.asarray(episode_end).reshape(-1).astype(bool); n = ee.size
    ends = list(np.flatnonzero(ee)); starts = [0] + [e + 1 for e in ends[:-1]]
    if not ends:
        return [(0, n - 1)] if n else []
    if ends[-1] != n - 1:
        starts.append(ends[-1] + 1); ends.append(n - 1)
    return list(zip(starts, ends))


def gae_returns(r, done, episode_end, Vs, Vsp, lam, gamma):
    """A = c A + r + (1 - done) gamma V(sp) - V(s) with c = lambda gamma, R = r + gamma R, both backwards over every episode (sampler.jl:263-280)"""
    r, done, Vs, Vsp = (np.asarray(x, np.float64).reshape(-1) for x in (r, done, Vs, Vsp))
    lam, gamma = float(np.float32(lam)), float(np.float32(gamma))
    adv, ret = np.zeros_like(r), np.zeros_like(r)
    for a, z in episodes(episode_end):
        A = R = 0.0
        for k in range(z, a - 1, -1):
            A = lam * gamma * A + r[k] + (1.0 - done[k]) * gamma * Vsp[k] - Vs[k]; adv[k] = A
            R = r[k] + gamma * R; ret[k] = R
    return adv, ret


def whiten(v):
    v = np.asarray(v, np.float64)
    return (v - v.mean()) / v.std(ddof=1)


def partition_plan(n_expert, n_policy, batch_size, epochs, max_batches=None):
    """the steps of batch_train!(D, d_opt, (;), D_expert, D_policy): a list of (epoch, off_ex, n_ex, off_pi, n_pi) with 0-based offsets into the freshly shuffled
    buffers; partition(1:length, batch_size) of each, zipped (the shorter ends the epoch), the count checked against max_batches after every step (:45, :50)"""
    B, out = int(batch_size), []
    for ep in range(epochs):
        pe = [(o, min(B, n_expert - o)) for o in range(0, n_expert, B)]; pp = [(o, min(B, n_policy - o)) for o in range(0, n_policy, B)]
        for (oe, ne), (op, np_) in zip(pe, pp):
            out.append((ep, oe, ne, op, np_))
            if max_batches is not None and len(out) >= max_batches:
                return out
    return out
