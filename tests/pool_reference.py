"""Host-only float64 reference of a conv trunk with pooling layers (csrc/conv_pool.hip): torch on the CPU -- conv2d, max_pool2d / avg_pool2d(count_include_pad=True), autograd.

A spec is conv_reference's with one more key, "pools": per conv layer None or {"kind": "max" | "mean", "k": (k1, k2), "stride": (s1, s2), "pad": (p1, p2)}. Layouts are the
trunk's (conv_reference.py): observations [W H C x B] with index w + W (h + H c), parameters in Flux.params order, Conv a true convolution (torch's conv2d is a cross-correlation:
the kernel is flipped on the way in). Axis 1 of every pair is W, which is torch's LAST axis.

The bound of tests/test_gpu_conv_pool.py per tensor: max |T - T64| <= (M max(e32, u) + mean_extra u) max |T64|, M = conv_reference.M_MARGIN (chosen on the CPU for the conv
kernels), e32 the same graph in float32. Max pooling adds nothing. Mean pooling: a pooled value is an n-term float32 sum and one division, n = k1 k2, so its error is at most
n u sum|taps| / (k1 k2); a gathered gradient likewise with n = ceil(k1 / s1) ceil(k2 / s2) covering windows. mean_extra is those two, each relative to its tensor's largest
entry (to first order what a relative perturbation of that size becomes in every tensor computed from it, like any other rounding of the chain)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_reference as CR
from conv_reference import M_MARGIN, U32, rel_err      # noqa: F401


def pool(kind, k, stride=None, pad=0):
    two = lambda v: (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))      # noqa: E731
    return {"kind": kind, "k": two(k), "stride": two(k if stride is None else stride), "pad": two(pad)}


def spec(W, H, C, layers, pools, scale=1.0):
    sp = CR.spec(W, H, C, layers, scale); sp["pools"] = list(pools)
    assert len(sp["pools"]) == len(sp["layers"])
    return sp


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def extents(sp):
    """[(W, H, C)] entering layer 0, 1, ..., and leaving the last one (behind its pool)"""
    out = [(sp["W"], sp["H"], sp["C"])]
    for ly, q in zip(sp["layers"], sp["pools"]):
        w, h, _ = out[-1]
        w, h = (_out(n, ly["k"][a], ly["stride"][a], ly["pad"][a]) for a, n in enumerate((w, h)))
        if q:
            w, h = (_out(n, q["k"][a], q["stride"][a], q["pad"][a]) for a, n in enumerate((w, h)))
        out.append((w, h, ly["cout"]))
    return out


def n_features(sp):
    w, h, c = extents(sp)[-1]
    return w * h * c


def pool2d(y, q):
    """y [B, C, H, W] -> the pooled tensor; the rules of the device kernels are torch's defaults"""
    k, s, p = (q["k"][1], q["k"][0]), (q["stride"][1], q["stride"][0]), (q["pad"][1], q["pad"][0])
    return F.max_pool2d(y, k, s, p) if q["kind"] == "max" else F.avg_pool2d(y, k, s, p, count_include_pad=True)


def _to_img(a, ext, B, dt):
    return torch.tensor(np.ascontiguousarray(np.asarray(a).reshape(tuple(ext) + (B,), order="F").transpose(3, 2, 1, 0)), dtype=dt)


def _to_cols(t):
    a = t.detach().numpy().transpose(3, 2, 1, 0)
    return np.asfortranarray(a.reshape((-1, a.shape[3]), order="F"))


_ACT = {"identity": lambda z: z, "relu": torch.relu, "tanh": torch.tanh}


def reference(params, sp, x, dy, dtype=np.float64):
    """{"y", "dx" [.. x B], "dW", "db" (per layer, Flux layout), "z", "Y", "P" (per layer, torch [B, C, H, W]: pre-activation, act(conv), the layer's output),
    "dY", "dP" (their gradients)} with every operand and intermediate in dtype; gradients unscaled"""
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    Ws, bs = CR.weights(params, sp, dtype); B = np.asarray(x).shape[1]
    tw = [torch.tensor(w, dtype=dt, requires_grad=True) for w in Ws]; tb = [torch.tensor(b, dtype=dt, requires_grad=True) for b in bs]
    tx = _to_img(x, (sp["W"], sp["H"], sp["C"]), B, dt).requires_grad_(True)
    h = tx * torch.tensor(float(np.float32(sp["scale"])), dtype=dt); zs, Ys, Ps = [], [], []
    for l, (ly, q) in enumerate(zip(sp["layers"], sp["pools"])):
        z = F.conv2d(h, torch.flip(tw[l].permute(3, 2, 1, 0), (2, 3)), tb[l], (ly["stride"][1], ly["stride"][0]), (ly["pad"][1], ly["pad"][0]))
        y = _ACT[ly["act"]](z); y.retain_grad(); h = pool2d(y, q) if q else y
        if q:
            h.retain_grad()
        zs.append(z.detach()); Ys.append(y); Ps.append(h)
    h.backward(_to_img(dy, extents(sp)[-1], B, dt))
    out = {"y": _to_cols(h), "dx": _to_cols(tx.grad), "dW": [w.grad.numpy() for w in tw], "db": [b.grad.numpy() for b in tb], "z": zs,
           "Y": [y.detach() for y in Ys], "P": [p.detach() for p in Ps], "dY": [y.grad for y in Ys], "dP": [p.grad for p in Ps]}
    assert out["y"].dtype == np.dtype(dtype) and out["dx"].dtype == np.dtype(dtype)
    return out


def flat_gradient(ref, sp):
    return CR.flat_gradient(ref, sp)


# ---- the condition on the inputs of a max-pooled trunk, and the add-on of a mean-pooled one -------------------------------------------------------------------------------
def near_tie(r64, r32, sp):
    """per sample: does a max-pool window of the float64 reference hold its largest and second-largest element within twice the forward bound of that layer's Y
    (M max(e32, u) max|Y|)? The device compares float32 values: inside that gap it may choose another element, and a whole gradient moves. Windows under relu whose elements
    are all equal (all zero) are exempt: act' kills their gradient whichever element is chosen."""
    bad = torch.zeros(r64["Y"][0].shape[0], dtype=torch.bool)
    for ly, q, y64, y32 in zip(sp["layers"], sp["pools"], r64["Y"], r32["Y"]):
        if not q or q["kind"] != "max":
            continue
        bound = M_MARGIN * max(rel_err(y32.numpy(), y64.numpy()), U32) * float(y64.abs().max())
        (k1, k2), (s1, s2), (p1, p2) = q["k"], q["stride"], q["pad"]; Bn, Cn = y64.shape[:2]
        cols = F.unfold(F.pad(y64, (p1, p1, p2, p2), value=-np.inf), (k2, k1), stride=(s2, s1)).reshape(Bn, Cn, k1 * k2, -1)
        top = cols.topk(2, dim=2).values; first, second = top[:, :, 0], top[:, :, 1]
        exempt = (first == 0) if ly["act"] == "relu" else torch.zeros_like(first, dtype=torch.bool)      # relu >= 0: a largest element of 0 means every tap inside is 0
        bad |= (~((first - second > 2 * bound) | exempt)).flatten(1).any(dim=1)
    return bad.numpy()


def near_kink(r64, sp, delta=1e-4):
    bad = np.zeros(r64["z"][0].shape[0], bool)
    for ly, z in zip(sp["layers"], r64["z"]):
        if ly["act"] == "relu":
            bad |= (z.abs() < delta).flatten(1).any(dim=1).numpy()
    return bad


def mean_extra(r64, sp):
    """in units of u: sum over the mean-pooled layers of n_f max(avgpool |Y|) / max|P| + n_b max(avgpool' |dP|) / max|dY| (see the module's head)"""
    tot = 0.0
    for q, y, p, dy, dp in zip(sp["pools"], r64["Y"], r64["P"], r64["dY"], r64["dP"]):
        if not q or q["kind"] != "mean":
            continue
        ya = y.abs().requires_grad_(True); pa = pool2d(ya, q); (ga,) = torch.autograd.grad(pa, ya, dp.abs()); pa = pa.detach()
        n_b = -(-q["k"][0] // q["stride"][0]) * -(-q["k"][1] // q["stride"][1])
        tot += q["k"][0] * q["k"][1] * float(pa.max()) / float(p.abs().max()) + n_b * float(ga.max()) / max(float(dy.abs().max()), 1e-300)
    return tot


def clean_images(p, sp, B, rng):
    """N(0, 1) observations [W H C x B]; columns within delta of a relu kink of the trunk or with a near tie in a max-pool window are redrawn until none is left"""
    n_in = sp["W"] * sp["H"] * sp["C"]; x = np.asfortranarray(rng.normal(0, 1, (n_in, B)).astype(np.float32)); zero = np.zeros((n_features(sp), B), np.float32)
    for _ in range(32):
        r64, r32 = reference(p, sp, x, zero, np.float64), reference(p, sp, x, zero, np.float32)
        bad = near_kink(r64, sp) | near_tie(r64, r32, sp)
        if not bad.any():
            return x
        x[:, bad] = rng.normal(0, 1, (n_in, int(bad.sum()))).astype(np.float32)
    raise RuntimeError("clean_images: %d of %d columns still near a kink or a tie" % (int(bad.sum()), B))


def td_reference(sp, p_trunk, dims, acts, p_head, s, a_onehot, y, dtype=np.float64):
    """conv_reference.td_reference over a pooled trunk: the flat gradients of trunk and head of mean((Q - y)^2), Q = sum(value .* onehot), and the trunk's reference"""
    import dense_reference as R
    dtype = np.dtype(dtype); B = np.asarray(s).shape[1]; a = np.asarray(a_onehot).astype(dtype)
    f = reference(p_trunk, sp, s, np.zeros((n_features(sp), B)), dtype)["y"]
    z = R.chain_reference(p_head, dims, acts, f, np.zeros((dims[-1], B)), dtype)["y"]
    d = ((z * a).sum(axis=0) - np.asarray(y).reshape(-1).astype(dtype)).astype(dtype)
    rh = R.chain_reference(p_head, dims, acts, f, (a * (dtype.type(2) * d / dtype.type(B))[None, :]).astype(dtype), dtype)
    rt = reference(p_trunk, sp, s, rh["dx"], dtype)
    return {"g_trunk": flat_gradient(rt, sp), "g_head": R.flat_gradient(rh, dims), "trunk": rt}


# ---- the grid of tests/test_gpu_conv_pool.py ------------------------------------------------------------------------------------------------------------------------------
POOLS = {"2x2s2": ((2, 2), (2, 2), (0, 0)), "3x3s2": ((3, 3), (2, 2), (0, 0)), "3x2s2x1p1x0": ((3, 2), (2, 1), (1, 0)), "2x2s3": ((2, 2), (3, 3), (0, 0))}


def grid_spec(window, kind, where, act):
    """7 x 6 x 2 -> Conv((3,3), 2=>5, pad 1) -> Conv((3,3), 5=>17, pad 1): both Y are 7 x 6, so every window drops trailing rows or columns; the pool sits behind layer
    `where` (0: an inner layer, the next Conv reads P_0; 1: the last layer, flatten reads P_1)"""
    k, s, p = POOLS[window]; pools = [None, None]; pools[where] = pool(kind, k, s, p)
    return spec(7, 6, 2, [CR.layer((3, 3), 2, 5, act, 1, 1), CR.layer((3, 3), 5, 17, act, 1, 1)], pools)


@functools.lru_cache(maxsize=None)
def grid_case(window, kind, where, act, B, seed=3):
    """(spec, parameters, observations, output gradient, float64 reference, float32 reference): observations whose columns lie within delta of a relu kink or hold a near tie
    in a max-pool window were redrawn until none is left. Computed once and shared; callers do not modify it."""
    sp = grid_spec(window, kind, where, act); rng = np.random.default_rng(seed)
    p = CR.perturbed(CR.glorot_params(sp, rng), rng)
    x = clean_images(p, sp, B, rng)
    dy = np.asfortranarray(rng.normal(0, 1, (n_features(sp), B)).astype(np.float32))
    return sp, p, x, dy, reference(p, sp, x, dy, np.float64), reference(p, sp, x, dy, np.float32)
