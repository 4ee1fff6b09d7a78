"""Host-only references of the convolutional trunk (csrc/conv.hip): Chain([x -> c x,] Conv..., flatten) forward and pullback in Flux's semantics, in a requested precision.

A trunk is described by a spec: {"W", "H", "C", "scale", "layers": [{"k": (k1, k2), "cin", "cout", "stride": (s1, s2), "pad": (p1, p2), "act"}]}. Parameters are the flat vector of
the trunk's parameter handle: per layer the (k1, k2, cin, cout) column-major weights, then cout biases (Flux.params order). Observations are [W H C x B] with one sample's
features contiguous (index w + W (h + H c)); the output is [OW OH cout x B] in flatten's order. Conv is a TRUE convolution (NNlib flips the kernel; CrossCor is the unflipped one).

  trunk_reference      y, dx and per layer dW, db in float64 (THE reference) or float32 through NumPy's matmul (the error scale: another summation order of the same length).
                       Every product is written as a matrix product over explicit patch matrices, so that the kernel's summation order can be substituted:
  emulated_reference   float32 emulation of the order conv.hip DEFINES: every output element one chain over the reduction index in the order the MFMA steps meet it
                       (within each block of 16: k = 4 g + r for r = 0..3, g = 0..3), the weight gradient in chunks of WG_CHUNK columns added in chunk order, db as four
                       lane-group chains per chunk combined (g0 + g1) + (g2 + g3) -- the CPU stand-in for a correct kernel when the margin M is chosen; not bit-identical to
                       the GPU (no fma)
  kink_free_images     observations none of whose relu pre-activations lies within delta of 0
"""
import numpy as np

from dense_reference import U32, _act, _act_grad, rel_err      # noqa: F401

WG_CHUNK = 512      # csrc/conv.hip: CONV_WG_CHUNK


def layer(k, cin, cout, act="identity", stride=1, pad=0):
    two = lambda v: (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))      # noqa: E731
    return {"k": two(k), "cin": int(cin), "cout": int(cout), "stride": two(stride), "pad": two(pad), "act": act}


def spec(W, H, C, layers, scale=1.0):
    return {"W": int(W), "H": int(H), "C": int(C), "scale": float(np.float32(scale)), "layers": list(layers)}


def extents(sp):
    """[(W, H, C)] entering layer 0, 1, ..., and leaving the last one"""
    out = [(sp["W"], sp["H"], sp["C"])]
    for ly in sp["layers"]:
        w, h, _ = out[-1]; (k1, k2), (s1, s2), (p1, p2) = ly["k"], ly["stride"], ly["pad"]
        out.append(((w + 2 * p1 - k1) // s1 + 1, (h + 2 * p2 - k2) // s2 + 1, ly["cout"]))
    return out


def layer_offsets(sp):
    """[(offset of W, offset of b)] of every layer in the flat parameter / gradient vector"""
    out, off = [], 0
    for ly in sp["layers"]:
        n = ly["k"][0] * ly["k"][1] * ly["cin"] * ly["cout"]
        out.append((off, off + n)); off += n + ly["cout"]
    return out


def n_params(sp):
    wo, bo = layer_offsets(sp)[-1]
    return bo + sp["layers"][-1]["cout"]


def n_features(sp):
    w, h, c = extents(sp)[-1]
    return w * h * c


def weights(params, sp, dtype):
    Ws, bs = [], []
    for ly, (wo, bo) in zip(sp["layers"], layer_offsets(sp)):
        Ws.append(np.asarray(params[wo:bo]).reshape(ly["k"] + (ly["cin"], ly["cout"]), order="F").astype(dtype)); bs.append(np.asarray(params[bo:bo + ly["cout"]]).astype(dtype))
    return Ws, bs


def glorot_params(sp, rng):
    """host stand-in for crux_conv_init_glorot: U(+-sqrt(6 / (k1 k2 cin + k1 k2 cout))) weights, zero biases"""
    p = np.zeros(n_params(sp), np.float32)
    for ly, (wo, bo) in zip(sp["layers"], layer_offsets(sp)):
        kk = ly["k"][0] * ly["k"][1]; lim = np.sqrt(6.0 / (kk * ly["cin"] + kk * ly["cout"])); p[wo:bo] = rng.uniform(-lim, lim, bo - wo).astype(np.float32)
    return p


# ---- the three products as explicit matrices -------------------------------------------------------------------------------------------------------------------------
def _patches(x, ly):
    """x [W, H, C, B] -> P [k1 k2 C, OW OH B]: row u1 + k1 (u2 + k2 ci) over the FLIPPED taps u = k - 1 - t, column ow + OW (oh + OH b);
    P[(u1, u2, ci), (ow, oh, b)] = x[ow s1 - p1 + u1, oh s2 - p2 + u2, ci, b], zero outside the image"""
    (k1, k2), (s1, s2), (p1, p2) = ly["k"], ly["stride"], ly["pad"]
    W, H, C, B = x.shape; OW, OH = (W + 2 * p1 - k1) // s1 + 1, (H + 2 * p2 - k2) // s2 + 1
    xp = np.zeros((W + 2 * p1, H + 2 * p2, C, B), x.dtype); xp[p1:p1 + W, p2:p2 + H] = x
    P = np.empty((k1, k2, C, OW, OH, B), x.dtype)
    for u1 in range(k1):
        for u2 in range(k2):
            P[u1, u2] = xp[u1:u1 + s1 * (OW - 1) + 1:s1, u2:u2 + s2 * (OH - 1) + 1:s2].transpose(2, 0, 1, 3)
    return P.reshape((k1 * k2 * C, OW * OH * B), order="F")


def _wmat(w):
    """w [k1, k2, cin, cout] -> [cout, k1 k2 cin] over the flipped taps (the rows of _patches)"""
    return np.ascontiguousarray(w[::-1, ::-1].reshape((-1, w.shape[3]), order="F").T)


def _cols(z):
    """[OW, OH, cout, B] -> [cout, OW OH B]"""
    OW, OH, co, B = z.shape
    return np.ascontiguousarray(z.transpose(2, 0, 1, 3).reshape((co, OW * OH * B), order="F"))


def _uncols(m, OW, OH, B):
    return m.reshape((m.shape[0], OW, OH, B), order="F").transpose(1, 2, 0, 3)


def _grad_patches(dz, ly, W, H):
    """gather form of the data gradient: dz [OW, OH, cout, B] -> G [k1 k2 cout, W H B], row u1 + k1 (u2 + k2 co), column iw + W (ih + H b);
    G = dz[(iw + p1 - u1) / s1, (ih + p2 - u2) / s2, co, b] where both divide and lie inside, else 0"""
    (k1, k2), (s1, s2), (p1, p2) = ly["k"], ly["stride"], ly["pad"]
    OW, OH, co, B = dz.shape
    G = np.zeros((k1, k2, co, W, H, B), dz.dtype)
    iw, ih = np.arange(W), np.arange(H)
    for u1 in range(k1):
        nx = iw + p1 - u1; okx = (nx >= 0) & (nx % s1 == 0) & (nx // s1 < OW)
        for u2 in range(k2):
            ny = ih + p2 - u2; oky = (ny >= 0) & (ny % s2 == 0) & (ny // s2 < OH)
            if okx.any() and oky.any():
                G[u1, u2][np.ix_(np.arange(co), iw[okx], ih[oky])] = dz[np.ix_(nx[okx] // s1, ny[oky] // s2)].transpose(2, 0, 1, 3)
    return G.reshape((k1 * k2 * co, W * H * B), order="F")


def _wmat_t(w):
    """w [k1, k2, cin, cout] -> [cin, k1 k2 cout] over the flipped taps (the rows of _grad_patches)"""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2).reshape((-1, w.shape[2]), order="F").T)


def trunk_reference(params, sp, x, dy, dtype=np.float64, mm=None, wg=None, rowsum=None, want_dx=True):
    """Forward and pullback of the trunk with every operand and every intermediate in `dtype`. x [W H C x B], dy [features x B] = d(loss)/d(output).
    Returns {"y", "dx", "dW": [k1, k2, cin, cout arrays], "db", "hs", "zs"}; gradients are unscaled. mm(A, B) replaces the matrix product of the forward and data passes,
    wg(A, B) that of the weight gradient (A [cout x N] times B [N x K]), rowsum(A) the sum over columns; the defaults are NumPy's."""
    dtype = np.dtype(dtype)
    mm = mm or (lambda A, B: A @ B); wg = wg or mm; rowsum = rowsum or (lambda A: A @ np.ones(A.shape[1], dtype))
    Ws, bs = weights(params, sp, dtype); ext = extents(sp); B = np.asarray(x).shape[1]
    h = (np.asarray(x).astype(dtype) * dtype.type(np.float32(sp["scale"]))).astype(dtype).reshape(ext[0] + (B,), order="F")
    hs, Ps = [h], []
    for l, ly in enumerate(sp["layers"]):
        P = _patches(hs[-1], ly); Ps.append(P)
        z = (mm(_wmat(Ws[l]), P) + bs[l][:, None]).astype(dtype)
        hs.append(np.ascontiguousarray(_uncols(_act(ly["act"], z).astype(dtype), ext[l + 1][0], ext[l + 1][1], B)))
    d = np.asarray(dy).astype(dtype).reshape(ext[-1] + (B,), order="F")
    L = len(sp["layers"]); dW, db = [None] * L, [None] * L
    for l in reversed(range(L)):
        ly = sp["layers"][l]
        d = _act_grad(ly["act"], hs[l + 1], d).astype(dtype); dm = _cols(d)
        g = wg(dm, np.ascontiguousarray(Ps[l].T)).astype(dtype)                                   # [cout, K] over the flipped taps
        dW[l] = np.ascontiguousarray(g.T.reshape(ly["k"] + (ly["cin"], ly["cout"]), order="F")[::-1, ::-1]); db[l] = rowsum(dm).astype(dtype)
        if l > 0 or want_dx:
            W_, H_, _ = ext[l]
            d = _uncols(mm(_wmat_t(Ws[l]), _grad_patches(d, ly, W_, H_)).astype(dtype), W_, H_, B)
    dx = (d * dtype.type(np.float32(sp["scale"]))).astype(dtype).reshape((-1, B), order="F") if want_dx else None
    y = hs[-1].reshape((-1, B), order="F")
    for a in [y] + dW + db + ([dx] if want_dx else []):
        assert a.dtype == dtype, (a.dtype, dtype)
    return {"y": y, "dx": dx, "dW": dW, "db": db, "hs": hs}


def flat_gradient(ref, sp, scale=1.0):
    """the reference's dW, db in the layout of crux_mlp_grads_ptr of the trunk's parameter handle"""
    g = np.zeros(n_params(sp), ref["y"].dtype)
    for l, (wo, bo) in enumerate(layer_offsets(sp)):
        g[wo:bo] = scale * ref["dW"][l].reshape(-1, order="F"); g[bo:bo + ref["db"][l].size] = scale * ref["db"][l]
    return g


# ---- the kernels' defined summation order, in float32 without fma --------------------------------------------------------------------------------------------------------
def _mfma_order(K):
    """the order one accumulator meets the reduction indices 0..K-1: blocks of 16 ascending, inside a block MFMA r = 0..3 sums lane groups g = 0..3, index 4 g + r"""
    k = np.arange(((K + 15) // 16) * 16).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1)      # [block][g][r] -> [block][r][g]
    return k[k < K]


def chain_order_f32(A, B):
    """A [M x K] @ B [K x N] in float32: one chain per output element from +0 in the MFMA order, each product rounded and then added (the kernel fuses the two)"""
    A = np.ascontiguousarray(A, np.float32); B = np.ascontiguousarray(B, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in _mfma_order(A.shape[1]):
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    return acc


def wgrad_order_f32(A, B):
    """the weight gradient A [cout x N] @ B [N x K]: the N columns in chunks of WG_CHUNK, one chain per chunk, the chunks added in chunk order"""
    A = np.ascontiguousarray(A, np.float32); B = np.ascontiguousarray(B, np.float32)
    tot = None
    for n0 in range(0, A.shape[1], WG_CHUNK):
        part = chain_order_f32(A[:, n0:n0 + WG_CHUNK], B[n0:n0 + WG_CHUNK])
        tot = part if tot is None else tot + part
    return tot


def rowsum_order_f32(A):
    """db: per chunk, lane group g sums its columns 16 j + 4 g + r ascending, the groups combine (g0 + g1) + (g2 + g3); the chunks are added in chunk order"""
    A = np.ascontiguousarray(A, np.float32)
    tot = None
    for n0 in range(0, A.shape[1], WG_CHUNK):
        blk = A[:, n0:n0 + WG_CHUNK]; acc = np.zeros((A.shape[0], 4), np.float32)
        for n in range(blk.shape[1]):
            acc[:, (n >> 2) & 3] += blk[:, n]
        part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        tot = part if tot is None else tot + part
    return tot


def emulated_reference(params, sp, x, dy, want_dx=True):
    return trunk_reference(params, sp, x, dy, np.float32, mm=chain_order_f32, wg=wgrad_order_f32, rowsum=rowsum_order_f32, want_dx=want_dx)


# ---- observations away from the relu kinks ------------------------------------------------------------------------------------------------------------------------------
def _near_kink(params, sp, x, delta, head=None):
    """per sample column: does any relu unit's float64 pre-activation lie within delta of 0 (head: (flat params, dims, acts) of a dense chain behind the trunk)"""
    Ws, bs = weights(params, sp, np.float64); ext = extents(sp); B = x.shape[1]
    h = (x.astype(np.float64) * np.float64(np.float32(sp["scale"]))).reshape(ext[0] + (B,), order="F"); bad = np.zeros(B, bool)
    for l, ly in enumerate(sp["layers"]):
        z = _wmat(Ws[l]) @ _patches(h, ly) + bs[l][:, None]
        if ly["act"] == "relu":
            bad |= (np.abs(z) < delta).reshape((-1, B), order="F").any(axis=0)
        h = _uncols(_act(ly["act"], z), ext[l + 1][0], ext[l + 1][1], B)
    if head is not None:
        import dense_reference as R
        bad |= R._near_kink(head[0], head[1], head[2], h.reshape((-1, B), order="F"), delta)
    return bad


def kink_free_images(params, sp, B, rng, delta=1e-4, max_rounds=32, draw=None, head=None):
    """observations [W H C x B] (float32, column-major) in which every sample column with a relu pre-activation inside (-delta, delta) was redrawn until none is left
    (dense_reference.kink_free_inputs for a trunk). draw(rng, shape) -> float32 array; the default is N(0, 1)."""
    draw = draw or (lambda r, shape: r.normal(0, 1, shape).astype(np.float32))
    n_in = sp["W"] * sp["H"] * sp["C"]
    x = draw(rng, (n_in, B))
    for rnd in range(max_rounds + 1):
        bad = _near_kink(params, sp, x, delta, head) if any(ly["act"] == "relu" for ly in sp["layers"]) or head is not None else np.zeros(B, bool)
        n = int(bad.sum())
        if n == 0:
            return np.asfortranarray(x)
        if rnd == max_rounds:
            break
        x[:, bad] = draw(rng, (n_in, n))
    raise RuntimeError("kink_free_images: %d of %d columns still within %g of a relu kink after %d rounds" % (n, B, delta, max_rounds))


# ---- the grid of tests/test_gpu_conv.py: (W, H, C; k, stride, pad; cout; B), chosen for the edges the kernels have ------------------------------------------------------------
def _one(W, H, C, k, stride, pad, cout, B, act="relu"):
    return (spec(W, H, C, [layer(k, C, cout, act, stride, pad)]), int(B))


ATARI = spec(80, 80, 4, [layer((8, 8), 4, 16, "relu", 4), layer((4, 4), 16, 32, "relu", 2)], scale=1.0 / 255.0)
TWO_LAYER = spec(16, 16, 2, [layer((4, 4), 2, 8, "relu", 2), layer((3, 3), 8, 12, "tanh", 1)])


def grid_cases():
    cs = [_one(9, 7, 3, (3, 2), (2, 1), 0, 5, 1), _one(9, 7, 3, (3, 2), (2, 1), 0, 5, 37),      # non-square image, K = 18, N no multiple of 16
          _one(8, 8, 1, (1, 1), 1, 0, 1, 3, "identity"),                                            # K = 1
          _one(6, 6, 2, (6, 6), 1, 0, 17, 16, "tanh"),                                              # kernel equals image, M crosses a tile
          _one(10, 10, 2, (3, 3), 1, 1, 16, 5),                                                     # padding
          _one(11, 11, 1, (2, 2), 3, 0, 4, 4, "tanh"),                                              # stride > kernel: uncovered inputs have dX exactly 0
          _one(12, 12, 4, (4, 4), 2, 0, 33, 9),                                                     # K = 64 exactly
          _one(13, 9, 5, (3, 3), 2, 0, 15, 9, "tanh"),                                              # K = 45
          (TWO_LAYER, 7), (TWO_LAYER, 64),                                                          # dX through an activation
          (ATARI, 4)]                                                                               # the deep reduction: 1 444 columns in layer 1 = three chunks of 512
    return cs


def case_id(case):
    sp, B = case
    return "%dx%dx%d_%s_B%d" % (sp["W"], sp["H"], sp["C"], "_".join("%d@%dx%ds%dx%dp%dx%d%s" % ((ly["cout"],) + ly["k"] + ly["stride"] + ly["pad"] + (ly["act"][0],)) for ly in sp["layers"]), B)


def perturbed(p, rng, sd=0.05):
    return (np.asarray(p, np.float32) + rng.normal(0, sd, np.asarray(p).size).astype(np.float32)).astype(np.float32)


def case_inputs(case, seed=3):
    """parameters (glorot weights, every parameter moved by N(0, 0.05): non-zero biases), kink-free observations and an output gradient of one grid case. The Atari case
    draws integer pixel values 0..255, which its 1/255 input scale brings to [0, 1]."""
    sp, B = case; rng = np.random.default_rng(seed)
    p = perturbed(glorot_params(sp, rng), rng)
    draw = (lambda r, shape: r.integers(0, 256, shape).astype(np.float32)) if sp["scale"] != 1.0 else None
    x = kink_free_images(p, sp, B, rng, draw=draw)
    dy = np.asfortranarray(rng.normal(0, 1, (n_features(sp), B)).astype(np.float32))
    return p, x, dy


# The margin of the trunk grid: a tensor passes iff err_gpu <= M x max(e32, u), the rule of dense_reference.py. tests/test_conv_reference.py runs the emulated kernel order
# over every grid case and measures its ratio to max(e32, u); M = 2 x the worst ratio. Chosen on the CPU, never fitted to the GPU.
# The worst ratio is 4.70 (dx of the padded case 10x10x2 -> 16@(3,3)/1 pad 1 at B = 5: e32 1.26 u, the emulated chain of 144 terms 5.90 u; next dW of the stride-3 case 4.01,
# y of the 6x6 kernel-equals-image case 2.30), so M = 2 x 4.70.
M_EMULATED_WORST = 4.70
M_EMULATED_WORST_CASE = ("10x10x2_16@3x3s1x1p1x1r_B5", "dx")
M_MARGIN = 2 * M_EMULATED_WORST


# ---- DQN over trunk + dense head: the trunk yardstick composed with dense_reference.chain_reference ------------------------------------------------------------------------
def q_reference(sp, p_trunk, dims, acts, p_head, s, dtype=np.float64):
    """value(pi, s) [n_actions x B] of the conv policy"""
    import dense_reference as R
    f = trunk_reference(p_trunk, sp, s, np.zeros((n_features(sp), np.asarray(s).shape[1])), dtype, want_dx=False)["y"]
    return R.chain_reference(p_head, dims, acts, f, np.zeros((dims[-1], f.shape[1])), dtype)["y"]


def dqn_target_reference(sp, p_trunk, dims, acts, p_head, sp_obs, r, done, gamma, dtype=np.float64):
    """y = r + gamma (1 - done) max_a Q-(sp) (rl/dqn.jl:4-6), gamma a Float32"""
    dtype = np.dtype(dtype); q = q_reference(sp, p_trunk, dims, acts, p_head, sp_obs, dtype)
    return (np.asarray(r).reshape(-1).astype(dtype) + dtype.type(np.float32(gamma)) * (1 - np.asarray(done).reshape(-1).astype(dtype)) * q.max(axis=0)).astype(dtype)


def td_reference(sp, p_trunk, dims, acts, p_head, s, a_onehot, y, w=None, dtype=np.float64):
    """train!(pi, td_loss) (utils.jl:76-87) up to the gradient: Q = sum(value .* onehot), loss = mean((Q - y)^2 w). Returns Q, loss, Qavg, the flat gradients of trunk and head
    and the norm over both."""
    import dense_reference as R
    dtype = np.dtype(dtype); B = np.asarray(s).shape[1]; a = np.asarray(a_onehot).astype(dtype)
    f = trunk_reference(p_trunk, sp, s, np.zeros((n_features(sp), B)), dtype, want_dx=False)["y"]
    z = R.chain_reference(p_head, dims, acts, f, np.zeros((dims[-1], B)), dtype)["y"]
    Q = (z * a).sum(axis=0).astype(dtype); d = (Q - np.asarray(y).reshape(-1).astype(dtype)).astype(dtype)
    ww = np.ones(B, dtype) if w is None else np.asarray(w).reshape(-1).astype(dtype)
    dz = (a * (dtype.type(2) * d * ww / dtype.type(B))[None, :]).astype(dtype)
    rh = R.chain_reference(p_head, dims, acts, f, dz, dtype)
    rt = trunk_reference(p_trunk, sp, s, rh["dx"], dtype, want_dx=False)
    gt, gh = flat_gradient(rt, sp), R.flat_gradient(rh, dims)
    return {"Q": Q, "loss": float((d * d * ww).astype(np.float64).mean()), "qavg": float(Q.astype(np.float64).mean()), "g_trunk": gt, "g_head": gh, "dabs_w": float((2 * np.abs(d) * ww).astype(np.float64).mean()),
            "grad_norm": float(np.sqrt((gt.astype(np.float64) ** 2).sum() + (gh.astype(np.float64) ** 2).sum()))}


# ---- Flux Adam's first update from zero moments ----------------------------------------------------------------------------------------------------------------------------
def adam_first_step_delta(g, eta, b1=0.9, b2=0.999, eps=1e-8):
    """p' - p in float64: m = (1 - b1) g, v = (1 - b2) g^2, -eta (m / (1 - b1)) / (sqrt(v / (1 - b2)) + eps)"""
    g = np.asarray(g, np.float64); m = (1 - b1) * g; v = (1 - b2) * g * g
    return -eta * (m / (1 - b1)) / (np.sqrt(v / (1 - b2)) + eps)


def adam_first_step_f32(p, g, eta, b1=0.9, b2=0.999, eps=1e-8):
    """the device's arithmetic (csrc/sac.hip adam_update): Float32 m and v, the update formed in Float64 and rounded once, subtracted in Float32"""
    gd = np.asarray(g, np.float32).astype(np.float64)
    mi = ((1.0 - b1) * gd).astype(np.float32); vi = (((1.0 - b2) * gd) * gd).astype(np.float32)
    d = (mi.astype(np.float64) / (1.0 - b1) / (np.sqrt(vi.astype(np.float64) / (1.0 - b2)) + eps) * eta).astype(np.float32)
    return (np.asarray(p, np.float32) - d).astype(np.float32)


def adam_small(p, eta):
    """per element: |(p' - p) - Delta64(g)| <= adam_small eta and |p' - p| <= eta (1 + adam_small). Three Float32 roundings on the way to the update (m, v -- halved by the
    square root --, the update itself: at most 2.5 u relative, taken as 4 u) and the rounding of p - d to p's spacing, at most u (|p| + eta).
    tests/test_conv_reference.py holds the float32 restatement to it."""
    return 4 * U32 + U32 * (np.abs(np.asarray(p, np.float64)) + eta) / eta


def adam_sign_ok(p, p_new, g, eta):
    """the sign of every element's update: never that of +g; and the element moves wherever the Float64 update exceeds half of p's spacing (at most u |p|, with 1 % to spare
    for the update's own roundings) -- below that p - d may round back to p"""
    p = np.asarray(p, np.float32); d = np.asarray(p_new, np.float32) - p; d64 = adam_first_step_delta(g, eta)
    must_move = np.abs(d64) > 1.01 * U32 * np.abs(p.astype(np.float64))
    return bool(np.all(np.sign(d) * np.sign(g) <= 0) and np.all(d[must_move] != 0))
