"""Float64 numpy restatement of the two-headed Gaussian actors (GaussianPolicy / SquashedGaussianPolicy whose logSigma is a network sharing its trunk with mu) and of SAC's
three pieces on them: the yardstick of tests/test_sigma_head_reference.py and tests/test_gpu_sigma_head.py. Written from the equations (src/policies.jl:333-398,
src/model_free/rl/sac.jl:4-52), not from any implementation; the Chain passes and Adam64 are those of tests/ensemble_reference.py.

The actor is ONE Chain whose last layer has 2 ad rows: z = net(s), mu = z[:ad], l = z[ad:] (two Dense(h, ad) heads on one trunk). Arrays are (features, batch).
    Gaussian   sigma = exp(l);                u = mu + sigma eps;  a = u;               lp_j = sum_d [-(u - mu)^2 / (2 sigma^2) - c0 - l]
    squashed   sigma = exp(clamp(l, -5, 2));  u = mu + sigma eps;  a = ascale tanh(u);  lp_j = sum_d [... - l - 2 (log 2 - u - softplus(-2 u))]      (-l unclamped)
    logpdf(s, a): u = a (Gaussian) or atanh(clamp(a / ascale, -1 + 1f-5, 1 - 1f-5));  entropy: 1.4189385332046727 + sum(l) (Gaussian: over everything; squashed: per column)
    sac_target   y = r + gamma (1 - done) (min(Q1t, Q2t)(sp, a') - alpha lp')                 sac_temp_loss  -mean(alpha (lp + H)), d/dlog_alpha = the same value
    sac_actor_loss  L = mean(alpha lp - min(Q1, Q2)(s, a)); with c = alpha / B and g_a = dL/da through the critics (it carries -1 / B):
      Gaussian   abar = -c (a - mu) / sigma^2 + g_a;  dmu = c (a - mu) / sigma^2 + abar;  dl = c ((a - mu)^2 / sigma^2 - 1) + abar eps sigma
      squashed   ubar = g_a ascale (1 - tanh^2 u) + c (-(u - mu) / sigma^2 + 2 tanh u);  dmu = c (u - mu) / sigma^2 + ubar;  dl = [-5 < l < 2] (c (u - mu)^2 / sigma^2 + ubar eps sigma) - c
    and the seed [dmu; dl] goes through the Chain's backward pass: the trunk's gradient is the sum of both heads' paths.
"""
import numpy as np

import cql_reference as CR
import ensemble_reference as ER

C0 = 0.9189385332046727
ENT0 = 1.4189385332046727
LO, HI = -1.0 + 1.0e-5, 1.0 - 1.0e-5      # (the reference writes them in Float32: -1f0 + 1f-5)

# name -> (trunk + output dims of the ACTOR as one chain, activations, act_dim)
SHAPES = {
    "2-32-2x1": ((2, 32, 2), ("relu", "identity"), 1),
    "5-100-100-2x3": ((5, 100, 100, 6), ("tanh", "tanh", "identity"), 3),      # nothing a multiple of 16, odd ad
    "4-256-256-2x2": ((4, 256, 256, 4), ("relu", "relu", "identity"), 2),      # split-K tiles
    "17-256-256-2x6": ((17, 256, 256, 12), ("relu", "relu", "identity"), 6),
}
CASE_SEED = {"2-32-2x1": 31, "5-100-100-2x3": 32, "4-256-256-2x2": 33, "17-256-256-2x6": 34}
BS = (1, 37, 257)
ASCALES = (0.0, 1.0, 2.0)      # 0 = GaussianPolicy
GRID_SHAPES = ("2-32-2x1", "5-100-100-2x3", "4-256-256-2x2")
# (shape, B, ascale) of the step cases: every shape, every batch size, every head; the 17-wide shape once; one actor step past 16 head blocks
STEP_CASES = ([(n, B, sc) for n in GRID_SHAPES for B, sc in ((37, 0.0), (257, 1.0), (37, 2.0))] + [(n, 1, 2.0) for n in GRID_SHAPES]
              + [("17-256-256-2x6", 37, 2.0), ("2-32-2x1", 4200, 1.0)])
SEED_OF = {("2-32-2x1", 1, 2.0): 44}      # (the default seed of this lone column leaves 0.43 of the 2-32 relu handle without gradient)
# A lone column through two 256-wide relu layers leaves every W2 entry next to a dead unit without gradient: with the default hidden biases |N(0, 0.3)| that is >= 0.32 of the
# handle, above the quarter the Adam comparison may leave out. This case's hidden biases are 0.5 + |N(0, 0.3)| (the pre-activations' own scale is about 0.3), which keeps 100 % / 84 % of the two layers' units alive.
HIDDEN_BIAS_OF = {("4-256-256-2x2", 1, 2.0): 0.5}
SEED = 0x51C3A      # the Philox seed of the GPU tests' draws
CLAMP_BIAS = (-6.0, 0.0, 3.0)


def philox_normals(ctr, B, ad, seed=SEED):
    """GaussExploreOp's / SigmaExploreOp's draws: column j, row d = randn(Philox(seed, counter, stream = j ad + d, NOISE)); [ad x B]. No GPU."""
    return CR.randn(seed, ctr, np.arange(B * ad)).reshape(B, ad).T.copy()


ACTOR_CTR = 13      # the counter of the GPU test's actor step: the CPU test of the skipped share takes the same normals


def _glorot(rng, dims, heads=1, hbias=0.0):
    p = []
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        last = l == len(dims) - 2
        lim = np.sqrt(6.0 / (i + (o // heads if last else o)))      # each head is a layer of its own: fan_out = ad
        p += [rng.uniform(-lim, lim, i * o), rng.normal(0, 0.1, o) if last else hbias + np.abs(rng.normal(0, 0.3, o))]      # hidden biases positive: few dead relu units
    return np.concatenate(p)


def head_offsets(dims):
    """(offset of the last layer's W, of its bias) in the flat vector"""
    off = sum(i * o + o for i, o in zip(dims[:-2], dims[1:-1]))
    return off, off + dims[-2] * dims[-1]


def case(name, B, ascale=0.0, clamp=None, seed=None):
    """The actor's flat vector, twin critics and their targets (od + ad -> hidden -> 1), log alpha, a batch (s, sp, a, r, done) and standard normals for the three draws:
    numpy alone. clamp = None: the logSigma head's biases in [-1, 0.2] and its weights shrunk so that every l lies inside (-5, 2). clamp = k: bias row d is
    CLAMP_BIAS[(d + k) % 3] (-6 / 0 / 3: below, inside, above the clamp); no l within 1e-3 of an edge (asserted). log alpha in [-2.5, -1.5] (alpha 0.08 .. 0.22, a trained SAC's
    range): the output layer's logSigma bias gradient is -alpha + ..., and at alpha ~ 1 it sets a gradient scale under which 0.4 of a 256-wide trunk counts as zero."""
    dims, acts, ad = SHAPES[name]; od = dims[0]
    seed = SEED_OF.get((name, B, float(ascale)) if clamp is None else None) if seed is None else seed
    rng = np.random.default_rng((CASE_SEED[name] if seed is None else seed) * 1000 + B + int(10 * ascale) * 7 + (0 if clamp is None else 100 + clamp))
    p = _glorot(rng, dims, heads=2, hbias=HIDDEN_BIAS_OF.get((name, B, float(ascale)), 0.0) if clamp is None else 0.0); wo, bo = head_offsets(dims); h = dims[-2]
    W = p[wo:bo].reshape((2 * ad, h), order="F"); W[ad:] *= 0.15; p[wo:bo] = W.reshape(-1, order="F")
    p[bo + ad:bo + 2 * ad] = rng.uniform(-1.0, 0.2, ad) if clamp is None else [CLAMP_BIAS[(d + clamp) % 3] for d in range(ad)]
    qdims = (od + ad,) + tuple(dims[1:-1]) + (1,); qacts = tuple("relu" for _ in dims[1:-1]) + ("identity",)
    qs = [_glorot(rng, qdims).astype(np.float32) for _ in range(4)]      # q1, q2, q1 target, q2 target
    c = {"name": name, "dims": dims, "acts": acts, "ad": ad, "od": od, "B": B, "ascale": float(ascale), "p": p.astype(np.float32), "qdims": qdims, "qacts": qacts,
         "q1": qs[0], "q2": qs[1], "q1t": qs[2], "q2t": qs[3], "log_alpha": np.float32(rng.uniform(-2.5, -1.5)), "gamma": np.float32(0.99), "H": np.float32(-ad)}
    c["s"] = np.asfortranarray(rng.normal(0, 1, (od, B)).astype(np.float32)); c["sp"] = np.asfortranarray(rng.normal(0, 1, (od, B)).astype(np.float32))
    c["r"] = rng.normal(0, 1, B).astype(np.float32); c["done"] = rng.uniform(0, 1, B) < 0.2
    c["eps"] = [rng.normal(0, 1, (ad, B)).astype(np.float32) for _ in range(3)]      # the target's, the temperature's, the actor's draw
    c["a"] = np.asfortranarray(explore(c, c["s"], rng.normal(0, 1, (ad, B)))[0].astype(np.float32))      # stored actions: drawn from the policy itself
    for s in (c["s"], c["sp"]):
        l = forward(c, s)[1]
        assert np.abs(l + 5.0).min() > 1e-3 and np.abs(l - 2.0).min() > 1e-3, (name, B, clamp)
        if clamp is None:
            assert l.min() > -5.0 and l.max() < 2.0, (name, B, float(l.min()), float(l.max()))
    return c


def forward(c, s, dtype=np.float64, p=None):
    """(mu, l, activations)"""
    z, hs = ER.forward(c["p"] if p is None else p, c["dims"], c["acts"], s, dtype); ad = c["ad"]
    return z[:ad], z[ad:], hs


def _sigma(c, l):
    return np.exp(np.clip(l, -5, 2)) if c["ascale"] > 0 else np.exp(l)


def _logprob(c, mu, l, u, dtype=np.float64):
    """the column sums, in the operand order the reference writes them"""
    sg = _sigma(c, l); two, c0 = dtype(2), dtype(C0)
    t = -(u - mu) ** 2 / (two * (sg * sg)) - c0 - l
    if c["ascale"] > 0:
        x = -two * u; sp = np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0)
        t = t - two * (np.log(two) - u - sp)
    return t.sum(0)


def explore(c, s, eps, dtype=np.float64, p=None):
    """exploration(pi, s) from given standard normals: (a, lp, u)"""
    mu, l, _ = forward(c, s, dtype, p); eps = np.asarray(eps, dtype)
    u = eps * _sigma(c, l) + mu
    a = dtype(c["ascale"]) * np.tanh(u) if c["ascale"] > 0 else u
    return a, _logprob(c, mu, l, u, dtype), u


def action(c, s, dtype=np.float64):
    mu = forward(c, s, dtype)[0]
    return dtype(c["ascale"]) * np.tanh(mu) if c["ascale"] > 0 else mu


def logpdf(c, s, a, dtype=np.float64):
    mu, l, _ = forward(c, s, dtype); a = np.asarray(a, dtype)
    u = np.arctanh(np.clip(a / dtype(c["ascale"]), dtype(np.float32(-1.0) + np.float32(1e-5)), dtype(np.float32(1.0) - np.float32(1e-5)))) if c["ascale"] > 0 else a
    return _logprob(c, mu, l, u, dtype)


def entropy(c, s, dtype=np.float64):
    """[1 x B] for the squashed policy, the reference's scalar over everything for the Gaussian one (policies.jl:348, 398)"""
    l = forward(c, s, dtype)[1]
    return dtype(ENT0) + (l.sum(0, keepdims=True) if c["ascale"] > 0 else l.sum())


def _q(c, key, x, dtype=np.float64):
    return ER.forward(c[key], c["qdims"], c["qacts"], x, dtype)


def sac_target(c, eps=None, dtype=np.float64):
    ap, lp, _ = explore(c, c["sp"], c["eps"][0] if eps is None else eps, dtype)
    x = np.vstack([np.asarray(c["sp"], dtype), ap]); mn = np.minimum(_q(c, "q1t", x, dtype)[0], _q(c, "q2t", x, dtype)[0])[0]
    alpha = np.exp(dtype(c["log_alpha"]))
    return np.asarray(c["r"], dtype) + dtype(c["gamma"]) * (dtype(1) - c["done"].astype(dtype)) * (mn - alpha * lp)


def sac_temp_loss(c, eps=None):
    """(loss, d loss / d log_alpha)"""
    lp = explore(c, c["s"], c["eps"][1] if eps is None else eps)[1]
    v = float(-np.mean(np.exp(np.float64(c["log_alpha"])) * (lp + np.float64(c["H"]))))
    return v, v


def _input_grad(flat, dims, acts, hs, dy):
    """d sum(dy * output) / d input of a Chain"""
    Ws, _ = ER.unflatten(flat, dims); d = np.asarray(dy, np.float64)
    for l in range(len(acts) - 1, -1, -1):
        y = hs[l + 1]
        d = d * (y > 0) if acts[l] == "relu" else d * (1.0 - y * y) if acts[l] == "tanh" else d
        d = Ws[l].T @ d
    return d


def sac_actor_loss(c, eps=None):
    """(loss, entropy, flat gradient of the actor, the seed [dmu; dl]) by hand"""
    eps = np.asarray(c["eps"][2] if eps is None else eps, np.float64); B, ad, od, sc = c["B"], c["ad"], c["od"], c["ascale"]
    mu, l, hs = forward(c, c["s"]); sg = _sigma(c, l); u = eps * sg + mu
    a = sc * np.tanh(u) if sc > 0 else u; lp = _logprob(c, mu, l, u)
    x = np.vstack([np.asarray(c["s"], np.float64), a])
    (z1, h1), (z2, h2) = _q(c, "q1", x), _q(c, "q2", x); second = z2[0] < z1[0]; mn = np.where(second, z2[0], z1[0])
    alpha = np.exp(np.float64(c["log_alpha"])); loss = float(np.mean(alpha * lp - mn)); cc = alpha / B
    g1 = _input_grad(c["q1"], c["qdims"], c["qacts"], h1, np.where(second, 0.0, -1.0 / B)[None, :])
    g2 = _input_grad(c["q2"], c["qdims"], c["qacts"], h2, np.where(second, -1.0 / B, 0.0)[None, :])
    ga = (g1 + g2)[od:]; s2 = sg * sg
    if sc > 0:
        th = np.tanh(u); ubar = ga * sc * (1.0 - th * th) + cc * (-(u - mu) / s2 + 2.0 * th)
        dmu = cc * (u - mu) / s2 + ubar
        dl = ((l > -5.0) & (l < 2.0)) * (cc * (u - mu) ** 2 / s2 + ubar * eps * sg) - cc
    else:
        abar = -cc * (a - mu) / s2 + ga
        dmu = cc * (a - mu) / s2 + abar
        dl = cc * ((a - mu) ** 2 / s2 - 1.0) + abar * eps * sg
    dz = np.vstack([dmu, dl])
    return loss, float(-np.mean(lp)), ER.backward(c["p"], c["dims"], c["acts"], hs, dz), dz


def actor_step(c, eps=None, lr=1e-3):
    """one train!(actor, sac_actor_loss): (info, gradient, parameters after Adam's first step). A NaN norm updates nothing"""
    loss, ent, g, _ = sac_actor_loss(c, eps); gn = float(np.sqrt(g @ g)); p = np.asarray(c["p"], np.float64)
    return {"loss": loss, "entropy": ent, "grad_norm": gn}, g, (p if np.isnan(gn) else ER.Adam64(p.size, lr=lr).step(p, g))


def temp_step(c, eps=None, lr=1e-3):
    v, g = sac_temp_loss(c, eps); la = np.array([np.float64(c["log_alpha"])])
    return {"loss": v, "grad_norm": abs(g), "alpha": float(np.exp(la[0]))}, ER.Adam64(1, lr=lr).step(la, np.array([g]))[0]


def skipped_share(g):
    return ER.skipped_share(g)


# ---- float32 restatement of the forward quantities: what the format itself costs ---------------------------------------------------------------------------------
def forward32(c):
    """{lp of the three draws' kind (explore at s), lp of the stored actions, y} in float32 throughout"""
    f = np.float32
    out = {"lp": explore(c, c["s"], c["eps"][2], f)[1], "logpdf": logpdf(c, c["s"], c["a"], f), "y": sac_target(c, dtype=f)}
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def forward64(c):
    return {"lp": explore(c, c["s"], c["eps"][2])[1], "logpdf": logpdf(c, c["s"], c["a"]), "y": sac_target(c)}


_ERR = {}


def float32_error(name):
    """per shape, over its B x ascale grid: the largest absolute error of the float32 restatement of (lp, y) against float64"""
    if name not in _ERR:
        elp = ey = 0.0
        for B in BS:
            for sc in ASCALES:
                c = case(name, B, sc); a, b = forward32(c), forward64(c)
                elp = max(elp, float(np.abs(a["lp"] - b["lp"]).max()), float(np.abs(a["logpdf"] - b["logpdf"]).max())); ey = max(ey, float(np.abs(a["y"] - b["y"]).max()))
        _ERR[name] = (elp, ey)
    return _ERR[name]


def tolerance(name):
    """absolute tolerances of the GPU's (lp, y) for a shape: four times float32's own error there (the margin covers the tile GEMMs' other summation order and the device's
    exp / log / tanh) -- the rule of mixture_reference.mixture_tolerance"""
    elp, ey = float32_error(name)
    return 4.0 * elp, 4.0 * ey
