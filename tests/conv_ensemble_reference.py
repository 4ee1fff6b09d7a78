"""One training_loss step of an ensemble of conv chains from conv_reference (trunk), dense_reference (head) and ensemble_reference (seeds, losses); pinned by torch autograd."""
import numpy as np

import conv_reference as CR
import dense_reference as R
import ensemble_reference as ER

# the step shape of tests/test_gpu_conv_ensemble.py: 10x10x2 -> 6@(3,3)/1 tanh -> flatten -> 384-8-nout, tanh then identity (no relu kinks to avoid)
SPEC = CR.spec(10, 10, 2, [CR.layer((3, 3), 2, 6, "tanh", 1)])
ACTS = ["tanh", "identity"]


def head_dims(nout):
    return [CR.n_features(SPEC), 8, nout]


def inputs(kind, M, B, seed):
    """(trunk parameters, head parameters) per member, x, y, w (Gaussian kind only)"""
    rng = np.random.default_rng(seed); nout = 4 if kind == ER.GAUSS else 3; dims = head_dims(nout)
    pts = [CR.perturbed(CR.glorot_params(SPEC, rng), rng) for _ in range(M)]; phs = [R.perturbed_params(R.glorot_params(dims, rng), rng) for _ in range(M)]
    x = np.asfortranarray(rng.normal(0, 1, (200, B)).astype(np.float32))
    if kind == ER.GAUSS:
        return pts, phs, x, np.asfortranarray(rng.normal(0, 1, (2, B)).astype(np.float32)), np.asfortranarray(rng.uniform(0.2, 1.5, (2, B)).astype(np.float32))
    return pts, phs, x, np.asfortranarray(np.eye(3, dtype=np.float32)[:, rng.integers(0, 3, B)]), None


def step_reference(kind, sp, dims, acts, pts, phs, x, y, w=None, dtype=np.float64):
    """forward, seeds and pullback of every member with the passes in `dtype` (the seeds and losses from those outputs in float64, ensemble_reference's)"""
    B = np.asarray(x).shape[1]; zf, zo = np.zeros((CR.n_features(sp), B)), np.zeros((dims[-1], B))
    fs = [CR.trunk_reference(pt, sp, x, zf, dtype, want_dx=False)["y"] for pt in pts]
    os = [R.chain_reference(ph, dims, acts, f, zo, dtype)["y"] for ph, f in zip(phs, fs)]; o64 = [o.astype(np.float64) for o in os]
    sd = ER.seeds(kind, o64, y, w); lm = ER.member_losses(kind, o64, y, w)
    rh = [R.chain_reference(ph, dims, acts, f, d, dtype) for ph, f, d in zip(phs, fs, sd)]
    gt = [CR.flat_gradient(CR.trunk_reference(pt, sp, x, r["dx"], dtype, want_dx=False), sp) for pt, r in zip(pts, rh)]; gh = [R.flat_gradient(r, dims) for r in rh]
    ssq = [float((a.astype(np.float64) ** 2).sum() + (b.astype(np.float64) ** 2).sum()) for a, b in zip(gt, gh)]
    return {"o": os, "seeds": sd, "dfeat": [r["dx"] for r in rh], "g_trunk": gt, "g_head": gh, "losses": lm, "loss": float(np.mean(lm)), "norms": [float(np.sqrt(s)) for s in ssq],
            "grad_norm": float(np.sqrt(sum(ssq)))}
