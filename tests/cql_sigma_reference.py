"""Float64 yardstick of CQL's conservative term (src/model_free/batch/cql.jl) with a two-headed actor -- a GaussianPolicy / SquashedGaussianPolicy whose logSigma is a network on
mu's trunk, the SAC_A() of examples/offline rl/hopper_medium.jl -- for tests/test_cql_sigma_reference.py and tests/test_gpu_cql_sigma.py. Nothing new is derived here: the
actor, its exploration and its cases are tests/sigma_head_reference.py's (SR), the draws, the uniform samples, conservative_loss and double_Q_loss are tests/cql_reference.py's (CR).

Policy sample k of state column j, action dimension d takes randn(Philox(seed, counter, stream (k B + j) ad + d, NOISE)): e = CR.randn(SEED, ctr, CR.streams(N, B, ad)), then
SR.explore(c, s, e[k]) per k (k = 0 is SR.philox_normals, the draw of exploration(pi, s)). Columns of the [ad x 2 N B] sample matrix: policy sample block k at k B + j, then
the uniform blocks; logprobs alike. No gradient reaches the actor (ignore_derivatives, cql.jl:12-19), so the samples enter the losses as numbers.
"""
import functools

import numpy as np
import torch

import cql_reference as CR
import ensemble_reference as ER
import sigma_head_reference as SR

SEED, CTR, THRESH, LO, HI, LR = SR.SEED, 40, 10.0, -1.0, 1.0, 1e-3
# (shape, B, ascale, N): batch sizes 1 / 37 / 257 = a lone column, a ragged block, one past a block of 256 columns
CASES = [("2-32-2x1", 37, 0.0, 3), ("2-32-2x1", 1, 2.0, 2), ("5-100-100-2x3", 37, 2.0, 4), ("5-100-100-2x3", 257, 0.0, 2), ("4-256-256-2x2", 257, 1.0, 3),
         ("4-256-256-2x2", 37, 2.0, 10), ("17-256-256-2x6", 37, 2.0, 4)]
CLAMP_CASE = ("5-100-100-2x3", 37, 1.0, 2)      # SR.case(..., clamp=0): logSigma head biases -6 / 0 / 3, below, inside and above the squashed head's clamp
BETA_CLAMP = float(np.log(2e6))                 # beta = clamp(exp(x), 0, 1f6) sits at its bound: the alpha gradient is 0
WEIGHTED_CASE = ("5-100-100-2x3", 37, 2.0, 4)


@functools.lru_cache(maxsize=None)
def case(name, B, sc, clamp=None):
    return SR.case(name, B, sc, clamp)


def log_alphas(c):
    """the two temperatures of every case: the case's own (alpha 0.08 .. 0.22) and 0 (CQL_alpha = 1, the solver's default)"""
    return (float(c["log_alpha"]), 0.0)


def normals(c, N, ctr=CTR, seed=SEED):
    """[N][ad x B] standard normals of the policy samples"""
    B, ad = c["B"], c["ad"]
    e = CR.randn(seed, ctr, CR.streams(N, B, ad)).reshape(N, B, ad)
    return [np.ascontiguousarray(e[k].T) for k in range(N)]


def policy_samples(c, N, ctr=CTR, dtype=np.float64, seed=SEED):
    """([ad x N B] actions, [N B] logprobs) of exploration(pi, s), N times"""
    out = [SR.explore(c, c["s"], e, dtype)[:2] for e in normals(c, N, ctr, seed)]
    return np.concatenate([a for a, _ in out], 1), np.concatenate([lp for _, lp in out])


def samples(c, N, ctr=CTR, seed=SEED):
    """the whole sample matrix of conservative_loss in float64: policy blocks, then uniform blocks"""
    pa, plp = policy_samples(c, N, ctr, seed=seed); ua, ulp = CR.uniform_samples(seed, ctr, N, c["B"], c["ad"], LO, HI)
    return np.concatenate([pa, ua.astype(np.float64)], 1), np.concatenate([plp, ulp.astype(np.float64)])


def lp_error32(c, N, ctr=CTR):
    """the largest absolute error of the float32 restatement of (the sampled actions, their logprobs) against float64 over the case's own N B samples"""
    a32, l32 = policy_samples(c, N, ctr, np.float32); a64, l64 = policy_samples(c, N, ctr)
    assert a32.dtype == np.float32 and l32.dtype == np.float32
    return float(np.abs(a32 - a64).max()), float(np.abs(l32 - l64).max())


def lp_tolerance(c, N, ctr=CTR):
    """absolute tolerance of the device's logprobs: SR.tolerance's rule (four times float32's own error; the margin covers the tile GEMMs' other summation order and the
    device's exp / log / tanh) over the case's own samples"""
    return 4.0 * lp_error32(c, N, ctr)[1]


def target(c):
    """y of the critic step: sac_target of the case (float32, as the device column it becomes)"""
    return SR.sac_target(c).astype(np.float32)


def weights(c):
    return np.random.default_rng(77).uniform(0.5, 1.5, c["B"]).astype(np.float32)


def conservative(c, a_samp, lp_samp, log_alpha, q1=None, q2=None):
    """(mean lse, mean qbar(s, a_data), beta, beta (5 L - thresh)) as float64 torch scalars"""
    q1 = CR.mlp_params(c["q1"], c["qdims"]) if q1 is None else q1; q2 = CR.mlp_params(c["q2"], c["qdims"]) if q2 is None else q2
    return CR.conservative(q1, q2, list(c["qacts"]), c["s"], c["a"], a_samp, lp_samp, log_alpha, THRESH)


def critic_step(c, a_samp, lp_samp, log_alpha, y, w=None, lr=LR):
    """train!(critics, double_Q_loss + conservative_loss): (info, [g1, g2], [p1, p2] after Adam's first step)"""
    q1, q2 = CR.mlp_params(c["q1"], c["qdims"]), CR.mlp_params(c["q2"], c["qdims"]); acts = list(c["qacts"])
    cons = conservative(c, a_samp, lp_samp, log_alpha, q1, q2)[3]
    mse, q1avg, q2avg = CR.double_q(q1, q2, acts, c["s"], c["a"], y, w)
    total = mse + cons; total.backward()
    gs = [CR.flat_grad(q1), CR.flat_grad(q2)]; gn = float(np.sqrt(sum((g ** 2).sum() for g in gs)))
    ps = [ER.Adam64(g.size, lr=lr).step(np.asarray(c[k], np.float64), g) for k, g in zip(("q1", "q2"), gs)]
    return {"loss": total.item(), "grad_norm": gn, "q1avg": q1avg.item(), "q2avg": q2avg.item()}, gs, ps


def alpha_step(c, a_samp, lp_samp, log_alpha, lr=LR):
    """train!(CQL_log_alpha, -conservative_loss): (info, gradient, log alpha after Adam's first step)"""
    x = torch.tensor(float(log_alpha), dtype=torch.float64, requires_grad=True)
    cons = conservative(c, a_samp, lp_samp, x)[3]
    (-cons).backward(); g = float(x.grad)
    x1 = float(ER.Adam64(1, lr=lr).step(np.array([float(log_alpha)]), np.array([g]))[0])      # (g = 0 beyond the clamp: m = v = 0, no move)
    return {"loss": -cons.item(), "grad_norm": abs(g), "alpha": float(np.exp(float(log_alpha)))}, g, x1


def skipped_shares(c, N, log_alpha, w=None):
    """the share of each critic's parameters the Adam comparison leaves out (ER.skipped_share), from the yardstick's own samples"""
    a, lp = samples(c, N)
    return [ER.skipped_share(g) for g in critic_step(c, a, lp, log_alpha, target(c), w)[1]]
