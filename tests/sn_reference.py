"""Float64 numpy restatement of a Chain of Dense and DenseSN layers (spectrally normalised Dense): the yardstick of tests/test_sn_reference.py and
tests/test_gpu_sn.py. Written from the equations, not from any implementation.

A DenseSN layer with weight W (out x in), bias b, activation act, a persistent non-trainable u (out) and n_iterations does in EVERY forward call
    n_iterations times:  t = W'u, v = t / (|t| + eps);  s = W v, u <- s / (|s| + eps)         eps = 2^-23 (eps(Float32))
    sigma = u' W v
    y = act((W / sigma) x + b)
u and v are constants of the pullback, sigma is differentiated through W. With G = dL/d(W / sigma):
    dL/dW = G / sigma - (sum_ik G_ik W_ik / sigma^2) u v'            dL/db unchanged
Parameters are one flat vector in the order W1, b1, W2, b2, ... with W column-major (out x in), the trainables of a plain Dense chain.
"""
import numpy as np

import advil_reference as AR
import offgail_reference as OR

EPS = 2.0 ** -23
Adam64 = AR.Adam64


def power_iteration(W, u, n_iterations=1):
    """(u, v) after n_iterations rounds from u"""
    W = np.asarray(W, np.float64); u = np.asarray(u, np.float64).reshape(-1); v = None
    for _ in range(n_iterations):
        t = W.T @ u; v = t / (np.sqrt(t @ t) + EPS)
        s = W @ v; u = s / (np.sqrt(s @ s) + EPS)
    return u, v


def msv(W, u, v):
    return float(u @ np.asarray(W, np.float64) @ v)


def unflatten(flat, dims):
    flat = np.asarray(flat, np.float64); Ws, bs, off = [], [], 0
    for l in range(len(dims) - 1):
        n = dims[l + 1] * dims[l]
        Ws.append(flat[off:off + n].reshape((dims[l + 1], dims[l]), order="F")); off += n
        bs.append(flat[off:off + dims[l + 1]]); off += dims[l + 1]
    return Ws, bs


def flatten(Ws, bs):
    return np.concatenate([np.concatenate([W.reshape(-1, order="F"), b]) for W, b in zip(Ws, bs)])


def _act(a, z):
    return np.maximum(z, 0.0) if a == "relu" else np.tanh(z) if a == "tanh" else z


def _dact(a, y, d):
    return d * (y > 0) if a == "relu" else d * (1.0 - y * y) if a == "tanh" else d


def forward(flat, dims, acts, sn, us, x):
    """One forward call of the chain. sn: n_iterations per layer (0 = plain Dense); us: one u per SN layer. Returns (y, cache); cache["us"] are the advanced u,
    cache["vs"] / cache["sigmas"] the v and sigma of this call (per SN layer)."""
    Ws, bs = unflatten(flat, dims); h = np.asarray(x, np.float64); hs, k = [h], 0
    new_us, vs, sg, eff = [], [], [], []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        if sn[l]:
            u, v = power_iteration(W, us[k], sn[l]); s = msv(W, u, v); k += 1
            new_us.append(u); vs.append(v); sg.append(s); eff.append(W / s)
        else:
            eff.append(W)
        h = _act(acts[l], eff[-1] @ h + b[:, None]); hs.append(h)
    return h, {"dims": dims, "acts": acts, "sn": sn, "Ws": Ws, "eff": eff, "hs": hs, "us": new_us, "vs": vs, "sigmas": sg}


def backward(cache, dy, gscale=1.0):
    """(flat parameter gradient * gscale, d loss / d x) for d loss / d y = dy, through the analytic DenseSN gradient"""
    Ws, eff, hs, acts, sn = cache["Ws"], cache["eff"], cache["hs"], cache["acts"], cache["sn"]
    L = len(Ws); d = np.asarray(dy, np.float64); gW, gb = [None] * L, [None] * L
    k = sum(1 for q in sn if q)
    for l in range(L - 1, -1, -1):
        dz = _dact(acts[l], hs[l + 1], d)
        G = dz @ hs[l].T; gb[l] = dz.sum(1); d = eff[l].T @ dz
        if sn[l]:
            k -= 1; s, u, v = cache["sigmas"][k], cache["us"][k], cache["vs"][k]
            G = G / s - ((G * Ws[l]).sum() / (s * s)) * np.outer(u, v)
        gW[l] = G
    return gscale * flatten(gW, gb), d


def _logsigmoid(z):
    return -(np.log1p(np.exp(-np.abs(z))) + np.maximum(-z, 0.0))


def bce_seed(z, n_ex, n_pi):
    """gail_d_loss(GAN_BCELoss): logitbinarycrossentropy(D(expert), 1) + logitbinarycrossentropy(D(policy), 0), mean over each half; (loss, dL/dz)"""
    z = np.asarray(z, np.float64).reshape(-1); ls = _logsigmoid(z); sgm = 1.0 / (1.0 + np.exp(-z))
    loss = (-ls[:n_ex]).mean() + (z[n_ex:] - ls[n_ex:]).mean()
    dz = np.concatenate([(sgm[:n_ex] - 1.0) / n_ex, sgm[n_ex:] / n_pi])
    return float(loss), dz.reshape(1, -1)


def bce_step(flat, dims, acts, sn, us, x_ex, x_pi, two_call=False):
    """loss, flat gradient and the advanced u of one discriminator step of the BCE form. two_call=False: one forward call on hcat(expert, policy) (what the
    device does, u advances once). two_call=True: the reference's form, D(expert) then D(policy) -- u advances twice and the halves see their own sigma."""
    n_ex, n_pi = x_ex.shape[1], x_pi.shape[1]
    if not two_call:
        z, c = forward(flat, dims, acts, sn, us, np.concatenate([x_ex, x_pi], 1))
        loss, dz = bce_seed(z, n_ex, n_pi); g, _ = backward(c, dz)
        return loss, g, c["us"], c
    z1, c1 = forward(flat, dims, acts, sn, us, x_ex); z2, c2 = forward(flat, dims, acts, sn, c1["us"], x_pi)
    loss, dz = bce_seed(np.concatenate([z1, z2], 1), n_ex, n_pi)
    g1, _ = backward(c1, dz[:, :n_ex]); g2, _ = backward(c2, dz[:, n_ex:])
    return loss, g1 + g2, c2["us"], c2


def ce_step(flat, dims, acts, sn, us, X, K, Bd):
    """OffPolicyGAIL's discriminator step: logitcrossentropy(D(X), labels) with one call of D on the concatenation; loss, flat gradient, advanced u, cache"""
    z, c = forward(flat, dims, acts, sn, us, X); N = z.shape[1]
    m = z.max(0); lse = m + np.log(np.exp(z - m).sum(0))
    loss = float((lse - z[OR.labels(K, Bd), np.arange(N)]).mean())
    g, _ = backward(c, OR.ce_seed(z, K, Bd))
    return loss, g, c["us"], c


def adam_first_step(flat, g, lr=1e-3):
    """the parameters after the first Adam step (Flux semantics, float64)"""
    return Adam64(len(flat), lr=lr).step(np.asarray(flat, np.float64), g)
