"""Plain NumPy reference of one behaviour-cloning minibatch over trunk + dense head (csrc/conv_bc.hip), every operand and intermediate in `dtype`. logpdf_bc_loss (il/bc.jl:10-18)
is a2c_loss with advantage 1, lambda_p 1 and old log-probability 0, so the categorical and Gaussian heads, trunk, head and norms are conv_pg_reference's and
conv_gauss_reference's own; only Flux.mse(mu, a) (bc.jl:1) is new. tests/test_conv_bc_reference.py pins the gradients against torch autograd in float64."""
import numpy as np

import conv_gauss_reference as GR
import conv_pg_reference as PG
import dense_reference as R
import pool_reference as PR

FORMS = ("categorical", "gaussian", "mse")


def head(form, z, a, ls, lambda_e, dtype):
    """loss, entropy, logpdf (= -mean log pi, the info row's slot), d(loss)/dz [n x B] and d(loss)/d(logSigma) [ad] (zeros under mse: action(pi, s) = mu)"""
    dtype = np.dtype(dtype); B = z.shape[1]; one, zero = np.ones(B, np.float32), np.zeros(B, np.float32)
    if form == "mse":
        d = z.astype(dtype) - np.asarray(a).astype(dtype)
        return {"loss": float((d * d).mean()), "entropy": 0.0, "logpdf": 0.0, "dz": (dtype.type(2) * d / dtype.type(d.size)).astype(dtype), "g_ls": np.zeros(0 if ls is None else len(ls), dtype)}
    r = PG.actor_seed("a2c", z, a, one, one, zero, 0.2, 1.0, lambda_e, dtype) if form == "categorical" else GR.actor_seed("a2c", z, a, ls, one, one, zero, 0.2, 1.0, lambda_e, dtype)
    return {"loss": r["loss"], "entropy": r["entropy"], "logpdf": r["kl"], "dz": r["dz"], "g_ls": r.get("g_ls", np.zeros(0, dtype))}


def head_dims(sp, nout):
    return [PR.n_features(sp) if "pools" in sp else PG.head_dims(sp, nout)[0], PG.HIDDEN, nout]


def _pooled_network(sp, p_trunk, dims, p_head, s, seed_fn, dtype):
    """conv_pg_reference.network over a trunk with pools (pool_reference.reference, as its td_reference composes it)"""
    B = np.asarray(s).shape[1]; f = PR.reference(p_trunk, sp, s, np.zeros((dims[0], B)), dtype)["y"]
    z = R.chain_reference(p_head, dims, PG.ACTS, f, np.zeros((dims[-1], B)), dtype)["y"]
    rh = R.chain_reference(p_head, dims, PG.ACTS, f, seed_fn(z), dtype)
    return z, PR.flat_gradient(PR.reference(p_trunk, sp, s, rh["dx"], dtype), sp), R.flat_gradient(rh, dims)


def bc_reference(form, sp, net, ls, s, a, lambda_e=1e-3, dtype=np.float64):
    """one crux_conv_bc_step up to the gradients. net: (flat trunk parameters, flat head parameters without logSigma); ls: the logSigma vector or None"""
    out = {}
    def seed(z):
        out.update(head(form, z, a, ls, lambda_e, dtype)); return out["dz"]
    out["z"], out["g_trunk"], out["g_head"] = (_pooled_network if "pools" in sp else PG.network)(sp, net[0], head_dims(sp, np.asarray(a).shape[0]), net[1], s, seed, np.dtype(dtype))
    out["grad_norm"] = float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in (out["g_trunk"], out["g_head"], out["g_ls"]))))
    return out


def inputs(form, sp, B, seed, ad=3):
    """(net, logSigma or None, observations, actions): conv_pg_reference's for one-hot actions, conv_gauss_reference's for Float32 ones (ad = 3 = N_ACTIONS, one head shape)"""
    if form == "categorical":
        net, _, s, a = PG.inputs(sp, B, seed)[:4]
        return net, None, s, a
    net, ls, _, s, a = GR.inputs(sp, B, ad, seed)[:5]
    return net, ls, s, a
