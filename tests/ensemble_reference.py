"""Float64 numpy restatement of DeepEnsemble and DeepClassificationEnsemble: the yardstick of tests/test_ensemble_reference.py and tests/test_gpu_ensemble.py.
Written from the equations, not from any implementation.

A member is a Chain of Dense layers; its parameters are one flat vector W1, b1, W2, b2, ... with W column-major (out x in). Arrays are (features, batch).
Regression member: o = model(x) has 2 nd rows; mu = o[:nd], var = softplus(o[nd:]) + 1e-3, softplus(x) = log1p(exp(-|x|)) + max(x, 0), softplus' = logistic.
    ensemble       mu* = mean_m mu_m,  var* = mean_m (var_m + mu_m^2) - mu*^2
    log-density    lp(mu, var, y) = -log(var) / 2 - (y - mu)^2 / (2 var)                   (no 2 pi term)
    training loss  L = mean_m [ -mean(w * lp(mu_m, var_m, y)) ], the inner mean over all n = nd B elements
                   dL/dmu_m = w (mu - y) / var / (n M);  dL/dvar_m = w (1 / (2 var) - (y - mu)^2 / (2 var^2)) / (n M);  dvar/dz = logistic(z)
Classification member: p = softmax(model(x)) over the rows.
    ensemble       p* = mean_m p_m;  logpdf = log(sum_c p*_c y_c + 1e-10)
    training loss  L = mean_m [ mean_j -sum_c xlogy(y_cj, p_cj + eps) ], eps = 2^-23, xlogy(0, .) = 0; the weights argument is accepted and IGNORED
                   dL/dp_c = -y_c / (p_c + eps) / (B M);  dL/do_k = p_k (dL/dp_k - sum_c p_c dL/dp_c)
One optimiser step: Adam (Flux semantics) on every member with the same hyper-parameters -- one Adam over all members' parameters is element-wise.
fit: batch_train! over injected permutations -- per epoch the columns perm[q bs : (q + 1) bs] for every partition q (a short last one runs), max_batches ends the call.
"""
import numpy as np

EPS32 = 2.0 ** -23
GAUSS, CLASS = "gauss", "class"

# name -> (dims, acts, kind): the shapes of the GPU tests (the issue's list)
SHAPES = {
    "3-12-2": ((3, 12, 2), ("relu", "identity"), GAUSS),                        # sub-tile, nd = 1
    "5-100-100-4": ((5, 100, 100, 4), ("tanh", "tanh", "identity"), GAUSS),     # no multiple of 16, nd = 2
    "4-256-256-2": ((4, 256, 256, 2), ("relu", "relu", "identity"), GAUSS),     # K >= 128: the split-K tiles, nd = 1
    "6-300-6": ((6, 300, 6), ("relu", "identity"), GAUSS),                      # nd = 3, K = 300
    "4-100-100-3": ((4, 100, 100, 3), ("tanh", "tanh", "identity"), CLASS),     # three classes
}
CASE_SEED = {"3-12-2": 11, "5-100-100-4": 12, "4-256-256-2": 13, "6-300-6": 14, "4-100-100-3": 15}
MS, BS = (1, 3, 5), (1, 37, 256)


def case(name, M, B, seed=None):
    """dims, acts, kind, M Glorot-uniform parameter vectors with small positive biases, x, y (regression targets of order one, or one-hot classes), positive weights w and an
    output gradient per member: numpy alone"""
    dims, acts, kind = SHAPES[name]
    rng = np.random.default_rng((CASE_SEED[name] if seed is None else seed) * 1000 + 17 * M + B)
    ps = []
    for _ in range(M):
        p = []
        for i, o in zip(dims[:-1], dims[1:]):
            lim = np.sqrt(6.0 / (i + o)); p += [rng.uniform(-lim, lim, i * o), np.abs(rng.normal(0, 0.3, o))]
        ps.append(np.concatenate(p).astype(np.float32))
    x = np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    if kind == GAUSS:
        nd = dims[-1] // 2; y = np.asfortranarray(rng.normal(0, 1, (nd, B)).astype(np.float32))
    else:
        C = dims[-1]; y = np.zeros((C, B), np.float32, order="F"); y[rng.integers(0, C, B), np.arange(B)] = 1.0
    w = np.asfortranarray(rng.uniform(0.5, 1.5, y.shape).astype(np.float32))
    dys = [np.asfortranarray(rng.normal(0, 1, (dims[-1], B)).astype(np.float32)) for _ in range(M)]
    return {"name": name, "dims": dims, "acts": acts, "kind": kind, "ps": ps, "x": x, "y": y, "w": w, "dys": dys, "M": M, "B": B, "rng": rng}


def unflatten(flat, dims, dtype=np.float64):
    flat = np.asarray(flat, dtype); Ws, bs, off = [], [], 0
    for l in range(len(dims) - 1):
        n = dims[l + 1] * dims[l]
        Ws.append(flat[off:off + n].reshape((dims[l + 1], dims[l]), order="F")); off += n
        bs.append(flat[off:off + dims[l + 1]]); off += dims[l + 1]
    return Ws, bs


def _act(a, z):
    return np.maximum(z, 0) if a == "relu" else np.tanh(z) if a == "tanh" else z


def forward(flat, dims, acts, x, dtype=np.float64):
    """(output, the activations h_0 .. h_L) of one member"""
    Ws, bs = unflatten(flat, dims, dtype); h = np.asarray(x, dtype); hs = [h]
    for W, b, a in zip(Ws, bs, acts):
        h = _act(a, W @ h + b[:, None]); hs.append(h)
    return h, hs


def backward(flat, dims, acts, hs, dy):
    """the flat parameter gradient of sum(dy * output)"""
    Ws, _ = unflatten(flat, dims); d = np.asarray(dy, np.float64); out = []
    for l in range(len(acts) - 1, -1, -1):
        y = hs[l + 1]
        d = d * (y > 0) if acts[l] == "relu" else d * (1.0 - y * y) if acts[l] == "tanh" else d
        out.append(np.concatenate([(d @ hs[l].T).reshape(-1, order="F"), d.sum(1)]))
        d = Ws[l].T @ d
    return np.concatenate(out[::-1])


def softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0)


def logistic(x):
    t = np.exp(-np.abs(x)); return np.where(x >= 0, 1 / (1 + t), t / (1 + t))


def softmax(o):
    e = np.exp(o - o.max(0, keepdims=True)); return e / e.sum(0, keepdims=True)


def members(kind, os):
    """individual_forward: ([mu_m], [var_m]) or ([p_m], None)"""
    if kind == CLASS:
        return [softmax(o) for o in os], None
    nd = os[0].shape[0] // 2; one = os[0].dtype.type(1e-3)
    return [o[:nd] for o in os], [softplus(o[nd:]) + one for o in os]


def mixture(kind, os):
    """the ensemble call: (mu*, var*) or (p*, None), members added in ascending order, one division"""
    a, b = members(kind, os); M = len(os)
    sm = a[0]
    for m in range(1, M):
        sm = sm + a[m]
    mean = sm / a[0].dtype.type(M)
    if kind == CLASS:
        return mean, None
    st = b[0] + a[0] * a[0]
    for m in range(1, M):
        st = st + (b[m] + a[m] * a[m])
    return mean, st / a[0].dtype.type(M) - mean * mean


def gauss_logpdf(mu, var, y):
    two = mu.dtype.type(2)
    return -np.log(var) / two - (y - mu) ** 2 / (two * var)


def logpdf(kind, os, y):
    mean, evar = mixture(kind, os); y = np.asarray(y, mean.dtype)
    if kind == CLASS:
        return np.log((mean * y).sum(0, keepdims=True) + mean.dtype.type(1e-10))
    return gauss_logpdf(mean, evar, y)


def xlogy(y, p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((y == 0) & ~np.isnan(p), 0.0, y * np.log(p))


def member_losses(kind, os, y, w=None):
    y = np.asarray(y, np.float64); a, b = members(kind, os)
    if kind == CLASS:      # the weights are ignored
        return [float((-xlogy(y, p + EPS32).sum(0)).mean()) for p in a]
    w = np.ones_like(y) if w is None else np.asarray(w, np.float64)
    return [float(-(w * gauss_logpdf(mu, var, y)).mean()) for mu, var in zip(a, b)]


def training_loss(kind, os, y, w=None):
    return float(np.mean(member_losses(kind, os, y, w)))


def seeds(kind, os, y, w=None):
    """dL/do per member, analytic"""
    y = np.asarray(y, np.float64); M = len(os); a, b = members(kind, os); out = []
    if kind == CLASS:
        B = y.shape[1]
        for p in a:
            dp = -y / (p + EPS32) / (B * M); out.append(p * (dp - (p * dp).sum(0, keepdims=True)))
        return out
    w = np.ones_like(y) if w is None else np.asarray(w, np.float64); n = y.size; nd = y.shape[0]
    for o, mu, var in zip(os, a, b):
        dmu = w * (mu - y) / var / (n * M); dvar = w * (1 / (2 * var) - (y - mu) ** 2 / (2 * var * var)) / (n * M)
        out.append(np.concatenate([dmu, dvar * logistic(o[nd:])], 0))
    return out


def loss_and_grads(ps, dims, acts, kind, x, y, w=None):
    """(ensemble loss, [loss_m], [flat gradient of member m])"""
    fw = [forward(p, dims, acts, x) for p in ps]; os = [f[0] for f in fw]
    sd = seeds(kind, os, y, w)
    gs = [backward(p, dims, acts, f[1], d) for p, f, d in zip(ps, fw, sd)]
    lm = member_losses(kind, os, y, w)
    return float(np.mean(lm)), lm, gs


class Adam64:
    """Flux.Optimise.Adam in float64: one state per member"""

    def __init__(self, n, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
        self.m, self.v, self.bp, self.h = np.zeros(n), np.zeros(n), [b1, b2], (lr, b1, b2, eps)

    def step(self, p, g):
        lr, b1, b2, eps = self.h
        self.m = b1 * self.m + (1 - b1) * g; self.v = b2 * self.v + (1 - b2) * g * g
        d = self.m / (1 - self.bp[0]) / (np.sqrt(self.v / (1 - self.bp[1])) + eps) * lr
        self.bp = [self.bp[0] * b1, self.bp[1] * b2]
        return p - d


def step(ps, opts, dims, acts, kind, x, y, w=None):
    """one training step: (info, gradients, new parameters); info = {loss, grad_norm, losses, norms}. A NaN norm updates nothing"""
    loss, lm, gs = loss_and_grads(ps, dims, acts, kind, x, y, w)
    norms = [float(np.sqrt(g @ g)) for g in gs]; gn = float(np.sqrt(sum(g @ g for g in gs)))
    info = {"loss": loss, "grad_norm": gn, "losses": lm, "norms": norms}
    if np.isnan(gn):
        return info, gs, [np.asarray(p, np.float64) for p in ps]
    return info, gs, [o.step(np.asarray(p, np.float64), g) for o, p, g in zip(opts, ps, gs)]


def minibatches(N, batch_size, epochs, perms, max_batches=None):
    """[(epoch, column indices)] in the order batch_train! takes them"""
    out, total = [], 0
    for ep in range(epochs):
        for q in range(0, N, batch_size):
            out.append((ep, np.asarray(perms[ep][q:q + batch_size]))); total += 1
            if max_batches and total >= max_batches:
                return out
    return out


def fit(ps, dims, acts, kind, X, Y, W, batch_size, epochs, perms, max_batches=None, lr=1e-3):
    """(parameters, one info per epoch run: that of its last step)"""
    opts = [Adam64(len(p), lr=lr) for p in ps]; ps = [np.asarray(p, np.float64) for p in ps]; rows = {}
    for ep, idx in minibatches(X.shape[1], batch_size, epochs, perms, max_batches):
        info, _, ps = step(ps, opts, dims, acts, kind, X[:, idx], Y[:, idx], None if W is None else W[:, idx])
        rows[ep] = info
    return ps, [rows[e] for e in sorted(rows)]


# ---- the float32 restatement in the reference's operand order: what Float32 itself loses in var* and in the ensemble logpdf ---------------------------------------
def mixture32(c):
    """(mean, var* or None, logpdf) in float32: float32 parameters, products and sums; the formulas in the order the reference writes them"""
    f = np.float32
    os = [forward(p, c["dims"], c["acts"], c["x"], f)[0] for p in c["ps"]]
    assert all(o.dtype == f for o in os)
    mean, evar = mixture(c["kind"], os)
    return mean, evar, logpdf(c["kind"], os, c["y"])


def mixture64(c):
    os = [forward(p, c["dims"], c["acts"], c["x"])[0] for p in c["ps"]]
    mean, evar = mixture(c["kind"], os)
    return mean, evar, logpdf(c["kind"], os, c["y"])


def float32_error(name):
    """per shape, over its (M, B) grid: the largest absolute error of the float32 restatement against float64 in var* and in the ensemble logpdf"""
    ev, el = 0.0, 0.0
    for M in MS:
        for B in BS:
            c = case(name, M, B); _, v32, l32 = mixture32(c); _, v64, l64 = mixture64(c)
            if v32 is not None:
                ev = max(ev, float(np.abs(v32 - v64).max()))
            el = max(el, float(np.abs(l32 - l64).max()))
    return ev, el


def mixture_tolerance(name):
    """absolute tolerance of the GPU's var* and ensemble logpdf for a shape: four times float32's own error there (the margin covers the tile GEMMs' other summation
    order and the device's exp / log / tanh)"""
    ev, el = float32_error(name)
    return 4.0 * ev, 4.0 * el


def skipped_share(g):
    """the share of parameters whose float64 gradient is within 1e-3 of the gradient scale of zero (not compared after an Adam step: it is lr sign(g) there)"""
    return float((np.abs(g) <= 1e-3 * np.abs(g).max()).mean())
