"""Float64 numpy restatement of MixtureNetwork: the yardstick of tests/test_mixture_reference.py and tests/test_gpu_mixture.py. Written from the equations, not from any
implementation; the Chain forward / backward passes, Adam64 and the minibatch order are those of tests/ensemble_reference.py.

A component is a Chain of Dense layers giving mu_k(s) [nd x B]; its flat parameters are W1, b1, ..., then logSigma_k [nd]. The weights are a Chain in -> K whose rows go
through a softmax, alpha_.j = softmax(z_.j), or a constant positive vector alpha [K] used raw (not renormalised). Arrays are (features, batch).
    l_kj = sum_d [ -(a_dj - mu_kdj)^2 / (2 sigma_kd^2) - log(2 pi) / 2 - logSigma_kd ]        t_kj = log alpha_kj + l_kj
    lp_j = m_j + log sum_k exp(t_kj - m_j),  m_j = max_k t_kj                                 naive form: log(sum_k alpha_kj exp(l_kj))
    L = -(1 / B) sum_j w_j lp_j;  r_kj = exp(t_kj - lp_j)
    dL/dmu_kdj = -(w_j / B) r_kj (a - mu) / sigma^2          dL/dlogSigma_kd = -(1 / B) sum_j w_j r_kj ((a - mu)^2 / sigma^2 - 1)
    dL/dz_kj = -(w_j / B) (r_kj - alpha_kj)                  dL/dalpha_k = -(1 / B) sum_j w_j r_kj / alpha_k
One optimiser step: Adam (Flux semantics) on all K + 1 handles with the same hyper-parameters; a NaN norm updates nothing. fit: batch_train! over injected permutations.
"""
import numpy as np

import ensemble_reference as ER

HALF_LOG_2PI = 0.9189385332046727

# name -> (component dims, component acts, weight dims with None for K or None for constant weights, weight acts)
SHAPES = {
    "2-32-1": ((2, 32, 1), ("relu", "identity"), (2, 32, None), ("relu", "identity")),                        # the reference's DeepGMM, nd = 1
    "5-100-100-3": ((5, 100, 100, 3), ("tanh", "tanh", "identity"), None, None),                              # no multiple of 16, nd = 3, constant weights
    "4-256-256-2": ((4, 256, 256, 2), ("relu", "relu", "identity"), (4, 64, None), ("relu", "identity")),     # K >= 128: the split-K tiles, nd = 2
}
CASE_SEED = {"2-32-1": 21, "5-100-100-3": 22, "4-256-256-2": 23}
KS, BS = (1, 3, 5), (1, 37, 257)
# (shape, K, B, weighted): with and without w, a weight network and constant alpha, every shape, K = 1 and 16 once
STEP_CASES = [("2-32-1", 3, 37, True), ("2-32-1", 5, 257, False), ("2-32-1", 16, 37, True), ("5-100-100-3", 3, 37, True), ("5-100-100-3", 5, 257, False),
              ("5-100-100-3", 1, 37, False), ("4-256-256-2", 3, 257, True), ("4-256-256-2", 5, 37, False),
              ("2-32-1", 3, 4200, True)]      # past 64 head blocks of 64 columns: a block walks a second stride
MIN_RESPONSIBILITY = 0.05


def _glorot(rng, dims, out_scale=1.0):
    p = []
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        lim = np.sqrt(6.0 / (i + o)) * (out_scale if l == len(dims) - 2 else 1.0)
        p += [rng.uniform(-lim, lim, i * o), rng.normal(0, 0.3, o) * out_scale if l == len(dims) - 2 else np.abs(rng.normal(0, 0.3, o))]      # hidden biases positive: few dead relu units
    return np.concatenate(p)


def case(name, K, B, seed=None):
    """dims, acts, K component vectors (Glorot-uniform, logSigma in [-0.1, 0.4]), the weight handle's vector (a Glorot network whose output layer shrinks likewise, or K positive
    numbers that do not add up to one), s, targets a drawn from the case's own mixture, positive column weights w: numpy alone. A component is one common Glorot draw
    plus a draw of its own that shrinks with K, so that the components overlap and every one keeps a mean responsibility >= 0.05 (asserted): a component without
    responsibility has vanishing gradients."""
    dims, acts, wdims, wacts = SHAPES[name]; nd = dims[-1]
    rng = np.random.default_rng((CASE_SEED[name] if seed is None else seed) * 1000 + 17 * K + B)
    spread = 0.6 / K ** 0.75; base = _glorot(rng, dims)
    ps = [np.concatenate([base + spread * _glorot(rng, dims), rng.uniform(-0.1, 0.4, nd)]).astype(np.float32) for _ in range(K)]
    if wdims is None:
        wp = (rng.uniform(0.8, 1.2, K) * 1.3 / K).astype(np.float32)
    else:
        wdims = tuple(K if d is None else d for d in wdims); wp = _glorot(rng, wdims, 0.5 * spread).astype(np.float32)
    s = np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    c = {"name": name, "dims": dims, "acts": acts, "wdims": wdims, "wacts": wacts, "ps": ps, "wp": wp, "s": s, "K": K, "B": B, "nd": nd}
    al = alphas(c, s); mus = [ER.forward(p[:-nd], dims, acts, s)[0] for p in ps]
    cdf = np.cumsum(al / al.sum(0, keepdims=True), 0); pick = np.minimum((rng.uniform(0, 1, B)[None, :] > cdf).sum(0), K - 1)
    a = np.stack([mus[k][:, j] + np.exp(np.asarray(ps[k][-nd:], np.float64)) * rng.normal(0, 1, nd) for j, k in enumerate(pick)], 1)
    c["a"] = np.asfortranarray(a.astype(np.float32)); c["w"] = np.asfortranarray(rng.uniform(0.5, 1.5, (1, B)).astype(np.float32))
    c["resp"] = density(c)[2].mean(1)
    assert c["resp"].min() >= MIN_RESPONSIBILITY, (name, K, B, c["resp"])
    return c


def alphas(c, s, dtype=np.float64):
    """alpha [K x B]"""
    if c["wdims"] is None:
        return np.repeat(np.asarray(c["wp"], dtype)[:, None], np.asarray(s).shape[1], 1)
    return ER.softmax(ER.forward(c["wp"], c["wdims"], c["wacts"], s, dtype)[0])


def component_logpdfs(c, s, a, dtype=np.float64):
    """l [K x B] in the operand order gaussian_logpdf writes it, and the components' (mu, activations)"""
    nd = c["nd"]; a = np.asarray(a, dtype); two, half = dtype(2), dtype(HALF_LOG_2PI); ls, fw = [], []
    for p in c["ps"]:
        mu, hs = ER.forward(p[:-nd], c["dims"], c["acts"], s, dtype); lsg = np.asarray(p[-nd:], dtype)[:, None]; sg = np.exp(lsg)
        ls.append((-(a - mu) ** 2 / (two * sg * sg) - half - lsg).sum(0)); fw.append((mu, hs))
    return np.stack(ls), fw


def density(c, s=None, a=None, dtype=np.float64):
    """(lp [B], t [K x B], r [K x B]) in the stable form"""
    s = c["s"] if s is None else s; a = c["a"] if a is None else a
    l, _ = component_logpdfs(c, s, a, dtype)
    with np.errstate(divide="ignore"):
        t = np.log(alphas(c, s, dtype)) + l
    m = t.max(0); lp = m + np.log(np.exp(t - m).sum(0))
    return lp, t, np.exp(t - lp)


def logpdf(c, s=None, a=None):
    return density(c, s, a)[0]


def naive_logpdf(c, s=None, a=None, dtype=np.float64):
    """log(sum(alpha .* exp.(logpdf_k))) as policies.jl:229-233 evaluates it (alpha per column): -Inf once every term underflows"""
    s = c["s"] if s is None else s; a = c["a"] if a is None else a
    l, _ = component_logpdfs(c, s, a, dtype)
    with np.errstate(divide="ignore"):
        return np.log((alphas(c, s, dtype) * np.exp(l)).sum(0))


def logpdf32(c):
    """lp in float32 throughout: float32 parameters, products and sums, the Gaussian term and the softmax in the order the reference writes them"""
    lp = density(c, dtype=np.float32)[0]; assert lp.dtype == np.float32
    return lp


def float32_error(name):
    """per shape, over its K x B grid: the largest absolute error of the float32 restatement of lp against float64"""
    return max(float(np.abs(logpdf32(c) - logpdf(c)).max()) for c in (case(name, K, B) for K in KS for B in BS))


def mixture_tolerance(name):
    """absolute tolerance of the GPU's lp for a shape: four times float32's own error there (the margin covers the tile GEMMs' other summation order and the device's
    exp / log / tanh) -- the rule of ER.mixture_tolerance"""
    return 4.0 * float32_error(name)


def loss_and_grads(c, s=None, a=None, w=None):
    """(loss, [flat gradient of component k], the weight handle's gradient, mean responsibilities)"""
    s = c["s"] if s is None else s; a = np.asarray(c["a"] if a is None else a, np.float64); B = a.shape[1]; nd = c["nd"]
    w = np.ones((1, B)) if w is None else np.asarray(w, np.float64).reshape(1, B)
    l, fw = component_logpdfs(c, s, a); al = alphas(c, s)
    with np.errstate(divide="ignore"):
        t = np.log(al) + l
    m = t.max(0); lp = m + np.log(np.exp(t - m).sum(0)); r = np.exp(t - lp)
    loss = float(-(w[0] * lp).sum() / B); gs = []
    for k, (p, (mu, hs)) in enumerate(zip(c["ps"], fw)):
        s2 = np.exp(2.0 * np.asarray(p[-nd:], np.float64))[:, None]; wr = w * r[k][None, :]
        dmu = -(wr / B) * (a - mu) / s2; dls = -(wr * ((a - mu) ** 2 / s2 - 1.0)).sum(1) / B
        gs.append(np.concatenate([ER.backward(p[:-nd], c["dims"], c["acts"], hs, dmu), dls]))
    if c["wdims"] is None:
        gw = -((w * r).sum(1) / B) / np.asarray(c["wp"], np.float64)
    else:
        _, hs = ER.forward(c["wp"], c["wdims"], c["wacts"], s); gw = ER.backward(c["wp"], c["wdims"], c["wacts"], hs, -(w / B) * (r - al))
    return loss, gs, gw, r.mean(1)


def step(c, opts, s=None, a=None, w=None):
    """one training step on a copy of the case: (info, gradients [K + 1], new parameter vectors [K + 1]); info = {loss, grad_norm, resp}. A NaN norm updates nothing"""
    loss, gs, gw, resp = loss_and_grads(c, s, a, w); gs = gs + [gw]; old = [np.asarray(p, np.float64) for p in c["ps"] + [c["wp"]]]
    gn = float(np.sqrt(sum(g @ g for g in gs))); info = {"loss": loss, "grad_norm": gn, "resp": resp}
    if np.isnan(gn):
        return info, gs, old
    return info, gs, [o.step(p, g) for o, p, g in zip(opts, old, gs)]


def optimisers(c, lr=1e-3):
    return [ER.Adam64(len(p), lr=lr) for p in c["ps"] + [c["wp"]]]


def fit(c, S, A, W, batch_size, epochs, perms, max_batches=None, lr=1e-3):
    """(parameter vectors [K + 1], one info per epoch run: that of its last step)"""
    opts = optimisers(c, lr); cur = dict(c); rows = {}; K = c["K"]
    for ep, idx in ER.minibatches(S.shape[1], batch_size, epochs, perms, max_batches):
        info, _, new = step(cur, opts, S[:, idx], A[:, idx], None if W is None else W[:, idx])
        cur = dict(cur, ps=new[:K], wp=new[K]); rows[ep] = info
    return cur["ps"] + [cur["wp"]], [rows[e] for e in sorted(rows)]


def skipped_share(g):
    return ER.skipped_share(g)


def far_actions(c, sigmas=30.0):
    """targets 30 sigma (of the widest component) beyond every component's mean: every l_k < -200"""
    nd = c["nd"]; mus = np.stack([ER.forward(p[:-nd], c["dims"], c["acts"], c["s"])[0] for p in c["ps"]]); sg = max(float(np.exp(p[-nd:]).max()) for p in c["ps"])
    return np.asfortranarray((mus.max(0) + sigmas * sg).astype(np.float32))


def bimodal(N, seed):
    """the reference's DeepGMM target (mixture_network_tests.jl): 0.5 N(1, 0.2) + 0.5 N(-1, 1), with the constant input 0.1"""
    rng = np.random.default_rng(seed); first = rng.uniform(0, 1, N) < 0.5
    y = np.where(first, rng.normal(1.0, 0.2, N), rng.normal(-1.0, 1.0, N)).astype(np.float32).reshape(1, N)
    return np.asfortranarray(np.full((2, N), 0.1, np.float32)), np.asfortranarray(y)
