"""Host-only references of the dense engine (csrc/dense.hip, csrc/dense_fused.h): Chain(Dense...) forward and pullback in a requested precision.

Parameters are the flat vector of a network handle: per layer W (out x in, column-major: W[o + out * k]) then b; anything behind the last layer (logSigma of a
Gaussian head) is ignored. Activations are [feature][sample], as in the reference (src/policies.jl:94-96, Zygote's pullback in src/training.jl:13-25).

  chain_reference      y, dx and per layer dW, db in float64 (THE reference) or float32 through NumPy's matmul (the error scale: another summation order of the same length)
  kink_free_inputs     observations none of whose relu pre-activations lies within delta of 0, so that relu' is the same in every precision and no entry has to be excused
  gemm16_order_f32     float32 emulation of the summation order dense.hip DEFINES for its tile GEMM (k ascending; K >= 128: four quarter chains) -- the CPU stand-in for a
                       correct kernel when the margin M of the grid test is chosen; not bit-identical to the GPU (no fma)
"""
import numpy as np

U32 = 2.0 ** -24      # unit roundoff of float32


# ---- the float64 pair tests/test_gpu_sac.py has used since round 3 (moved here unchanged) -----------------------------------------------------------------
def _np_mlp(params, dims, acts, x):
    """float64 forward of Chain(Dense...) returning all activations."""
    hs, off = [x.astype(np.float64)], 0
    for l, act in enumerate(acts):
        i, o = dims[l], dims[l + 1]
        W = params[off:off + i * o].reshape((o, i), order="F").astype(np.float64); off += i * o
        b = params[off:off + o].astype(np.float64); off += o
        z = W @ hs[-1] + b[:, None]
        hs.append(np.maximum(z, 0) if act == "relu" else np.tanh(z) if act == "tanh" else z)
    return hs


def _np_backward(params, dims, acts, hs, dy):
    g, d = np.zeros_like(params, dtype=np.float64), dy.astype(np.float64)
    offs, off = [], 0
    for l in range(len(acts)):
        offs.append(off); off += dims[l] * dims[l + 1] + dims[l + 1]
    for l in reversed(range(len(acts))):
        i, o = dims[l], dims[l + 1]
        y = hs[l + 1]
        d = d * (y > 0) if acts[l] == "relu" else d * (1 - y * y) if acts[l] == "tanh" else d
        W = params[offs[l]:offs[l] + i * o].reshape((o, i), order="F").astype(np.float64)
        g[offs[l]:offs[l] + i * o] = (d @ hs[l].T).reshape(-1, order="F")
        g[offs[l] + i * o:offs[l] + i * o + o] = d.sum(axis=1)
        d = W.T @ d
    return g, d


# ---- the chain in a requested precision -------------------------------------------------------------------------------------------------------------------
def layer_offsets(dims):
    """[(offset of W, offset of b)] of every layer in the flat parameter / gradient vector."""
    out, off = [], 0
    for l in range(len(dims) - 1):
        out.append((off, off + dims[l] * dims[l + 1])); off += dims[l] * dims[l + 1] + dims[l + 1]
    return out


def n_layer_params(dims):
    return sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1))


def _weights(params, dims, dtype):
    Ws, bs = [], []
    for l, (wo, bo) in enumerate(layer_offsets(dims)):
        i, o = dims[l], dims[l + 1]
        Ws.append(np.asarray(params[wo:wo + i * o]).reshape((o, i), order="F").astype(dtype)); bs.append(np.asarray(params[bo:bo + o]).astype(dtype))
    return Ws, bs


def _act(act, z):
    return np.maximum(z, 0) if act == "relu" else np.tanh(z) if act == "tanh" else z


def _act_grad(act, y, d):
    """act'(z) .* d written in terms of the layer's OUTPUT y, as the engine does (crux_act_grad)"""
    return d * (y > 0) if act == "relu" else d * (1 - y * y) if act == "tanh" else d


def chain_reference(params, dims, acts, x, dy, dtype=np.float64, mm=None, rowsum=None):
    """Forward and pullback of Chain(Dense(dims[l], dims[l + 1], acts[l])...) with every operand and every intermediate in `dtype`.
    x [dims[0] x B], dy [dims[-1] x B] = d(loss)/d(output). Returns {"y", "dx", "dW": [...], "db": [...], "hs"}; gradients are unscaled.
    mm(A, B) / rowsum(A) replace the matrix product and the sum over samples (gemm16_order_f32 / rowsum16_order_f32); the default is NumPy's."""
    dtype = np.dtype(dtype)
    mm = mm or (lambda A, B: A @ B); rowsum = rowsum or (lambda A: A @ np.ones(A.shape[1], dtype))      # (through matmul like every other sum: NumPy's pairwise .sum() is far more accurate than any chain of the same length and would not be an error SCALE)
    Ws, bs = _weights(params, dims, dtype)
    hs = [np.ascontiguousarray(np.asarray(x).astype(dtype))]
    for l, act in enumerate(acts):
        hs.append(_act(act, (mm(Ws[l], hs[-1]) + bs[l][:, None]).astype(dtype)).astype(dtype))
    d = np.ascontiguousarray(np.asarray(dy).astype(dtype)); dW, db = [None] * len(acts), [None] * len(acts)
    for l in reversed(range(len(acts))):
        d = _act_grad(acts[l], hs[l + 1], d).astype(dtype)
        dW[l] = mm(d, np.ascontiguousarray(hs[l].T)).astype(dtype); db[l] = rowsum(d).astype(dtype)
        d = mm(np.ascontiguousarray(Ws[l].T), d).astype(dtype)
    for a in [hs[-1], d] + dW + db:
        assert a.dtype == dtype, (a.dtype, dtype)
    return {"y": hs[-1], "dx": d, "dW": dW, "db": db, "hs": hs}


def flat_gradient(ref, dims, scale=1.0):
    """the reference's dW, db in the layout of crux_mlp_grads_ptr"""
    g = np.zeros(n_layer_params(dims), ref["y"].dtype)
    for l, (wo, bo) in enumerate(layer_offsets(dims)):
        g[wo:bo] = scale * ref["dW"][l].reshape(-1, order="F"); g[bo:bo + dims[l + 1]] = scale * ref["db"][l]
    return g


def rel_err(t, t64):
    """max |T - T_f64| / max |T_f64|: the error measure of the engine grid"""
    t64 = np.asarray(t64, np.float64)
    return float(np.abs(np.asarray(t, np.float64) - t64).max() / max(np.abs(t64).max(), np.finfo(np.float64).tiny))


# ---- observations away from the relu kinks ------------------------------------------------------------------------------------------------------------------
def _near_kink(params, dims, acts, x, delta):
    """per sample column: does any relu unit's float64 pre-activation lie within delta of 0"""
    Ws, bs = _weights(params, dims, np.float64)
    h, bad = x.astype(np.float64), np.zeros(x.shape[1], bool)
    for l, act in enumerate(acts):
        z = Ws[l] @ h + bs[l][:, None]
        if act == "relu":
            bad |= (np.abs(z) < delta).any(axis=0)
        h = _act(act, z)
    return bad


def kink_free_inputs(params, dims, acts, B, rng, delta=1e-4, max_rounds=32, stats=None):
    """N(0, 1) observations [dims[0] x B] (float32, column-major) in which every sample column with a relu pre-activation inside (-delta, delta) was redrawn until none is
    left: relu' then agrees between float64, float32 and the k-ordered MFMA sums (delta = 1e-4 is about ten times the worst-case float32 error of a 256-long chain of
    O(1) terms, 256 u ~ 1.5e-5). Raises after max_rounds rounds. stats (a dict) receives the rounds and the columns redrawn."""
    x = rng.normal(0, 1, (dims[0], B)).astype(np.float32)
    redrawn = 0
    for rnd in range(max_rounds + 1):
        bad = _near_kink(params, dims, acts, x, delta)
        n = int(bad.sum())
        if n == 0:
            if stats is not None:
                stats["rounds"], stats["redrawn"] = rnd, redrawn
            return np.asfortranarray(x)
        if rnd == max_rounds:
            break
        x[:, bad] = rng.normal(0, 1, (dims[0], n)).astype(np.float32); redrawn += n
    raise RuntimeError("kink_free_inputs: %d of %d columns still within %g of a relu kink after %d rounds (dims %s)" % (n, B, delta, max_rounds, dims))


# ---- the engine's defined summation order, in float32 without fma -------------------------------------------------------------------------------------------
def _quarters(K, split):
    """[(kbeg, kend)] of the chains the reduction over K is defined in (dense.hip, Gemm16: kper = ceil16(ceil(K / 4)) whenever the split-K form applies)"""
    if split is None:
        split = K >= 128
    if not split:
        return [(0, K)]
    kper = (((K + 3) >> 2) + 15) & ~15
    return [(min(q * kper, K), min((q + 1) * kper, K)) for q in range(4)]


def gemm16_order_f32(A, B, split=None):
    """A [M x K] @ B [K x N] in float32 in the order the tile GEMM defines: every output element is a chain over k ascending from +0, each product rounded to float32 and
    then added (the kernel's v_mfma chain fuses the two: this is the no-fma restatement); for K >= 128 four quarter chains, combined ((q0 + q1) + q2) + q3 (a quarter that
    starts past K contributes +0). split=False gives one chain over the whole of K (what K < 128 takes)."""
    A = np.ascontiguousarray(A, np.float32); B = np.ascontiguousarray(B, np.float32)
    M, K = A.shape; K2, N = B.shape; assert K == K2
    tot = None
    for kb, ke in _quarters(K, split):
        acc = np.zeros((M, N), np.float32)
        for k in range(kb, ke):
            acc += A[:, k:k + 1] * B[k:k + 1, :]
        tot = acc if tot is None else tot + acc
    return tot


def rowsum16_order_f32(A, split=None):
    """sum over the columns of A [M x K] the way db rides along in the weight-gradient tiles: lane group g sums k = 16 j + 4 g + r ascending, the quarters are combined per
    lane group ((q0 + q1) + q2) + q3, then the four lane groups as (g0 + g1) + (g2 + g3)."""
    A = np.ascontiguousarray(A, np.float32); M, K = A.shape
    grp = (np.arange(K) >> 2) & 3
    tot = None
    for kb, ke in _quarters(K, split):
        acc = np.zeros((M, 4), np.float32)
        for k in range(kb, ke):
            acc[:, grp[k]] += A[:, k]
        tot = acc if tot is None else tot + acc
    return (tot[:, 0] + tot[:, 1]) + (tot[:, 2] + tot[:, 3])


# ---- the shape grid of tests/test_gpu_dense_grid.py (explicit lists: every edge is named in a test id) -------------------------------------------------------
FUSED_WIDTHS = [(128, 128), (192, 192), (256, 256), (192, 128), (128, 256)]      # df_fwd12_ok / df_bwd_ok: widths in {128, 192, 256}
FUSED_B = [127, 128, 129, 200, 255, 256, 257]                                    # the fused pullback's batch window 128 <= B <= 256, ragged inside, and its two borders
RELU3, TANH3 = ["relu", "relu", "identity"], ["tanh", "tanh", "identity"]


def _case(dims, acts, B):
    return (list(dims), list(acts), int(B))


def case_id(case):
    dims, acts, B = case
    return "%s_%s_B%d" % ("-".join(str(d) for d in dims), "".join(a[0] for a in acts), B)


def fused_cases():
    """every fused width pair at every B of the pullback's window; input and output widths rotate through the values that select other kernel combinations:
    inputs 1, 3, 16 (one input tile: the fused pullback), 17, 32 (u1: Fwd12Op's second input tile; no fused pullback), outputs 1, 4 (fused3) and 2, 6, 17 (not)"""
    ins, outs = [3, 16, 17, 32, 1, 8, 16], [1, 4, 2, 6, 17, 4, 1]
    out = []
    for w, (h1, h2) in enumerate(FUSED_WIDTHS):
        for b, B in enumerate(FUSED_B):
            k = (w + b) % len(ins)
            acts = RELU3 if (w + b) % 3 else TANH3
            out.append(_case([ins[k], h1, h2, outs[(w + 2 * b) % len(outs)]], acts, B))
    return out


def grid_cases():
    cs = fused_cases()
    # fused shapes whose output layer is not identity: no fused3, and the k_act_grad launch in front of the pullback
    cs += [_case([8, 256, 256, 4], ["relu", "relu", "tanh"], B) for B in (128, 200, 256)] + [_case([4, 192, 192, 1], ["tanh", "relu", "tanh"], B) for B in (129, 255)]
    # input widths at the borders of "one input tile" (df_bwd_ok: <= 16) and of the fused forward (df_fwd12_ok: <= 32; u1 = in0 > 16): four kernel combinations
    for in0 in (1, 3, 16, 17, 32, 33):
        cs += [_case([in0, 256, 256, 4], RELU3, 200), _case([in0, 192, 192, 1], TANH3, 256), _case([in0, 128, 128, 2], RELU3, 1000)]
    # widths outside the fused family: per-layer launches only; 130 / 50 / 7 / 48 / 33 take the dword operand path (vec_ok needs K % 4 == 0 and stride % 4 == 0)
    for (h1, h2), in0, out_, acts in [((256, 64), 8, 4, RELU3), ((64, 256), 17, 6, TANH3), ((64, 64), 4, 2, RELU3), ((48, 48), 3, 1, TANH3), ((160, 96), 16, 3, RELU3),
                                      ((320, 320), 8, 4, RELU3), ((130, 50), 33, 6, TANH3)]:
        for B in (1, 17, 130, 257, 1000):
            cs.append(_case([in0, h1, h2, out_], acts, B))
    for B in (1, 15, 16, 17, 127, 128, 129, 512, 4000):
        cs.append(_case([5, 7, 3], ["relu", "identity"], B))               # width (7,)
    for B in (1, 15, 16, 17, 128, 130, 5003):
        cs.append(_case([5, 3], ["identity"], B))                           # one layer
    cs += [_case([5, 3], ["tanh"], 200)]
    for B in (17, 129, 256, 1000):
        cs.append(_case([8, 256, 256, 256, 4], ["relu", "tanh", "relu", "identity"], B))      # four layers: Fwd12Op, then two per-layer launches
    # the weight gradient's K = B under split-K: ragged fourth quarters, and quarters that start past K
    for B in (130, 512, 1000, 4000, 4097, 5003):
        cs += [_case([17, 64, 64, 6], TANH3, B), _case([3, 64, 64, 1], RELU3, B)]
    for B in (1, 15, 16, 17):
        cs += [_case([8, 256, 256, 4], RELU3, B), _case([17, 192, 128, 6], TANH3, B)]
    for B in (512, 1000, 4000, 4097, 5003):
        cs += [_case([8, 192, 192, 4], RELU3, B)]
    # a 256-wide layer at B = 4112 has 16 x 257 = 4112 tiles: past launch_gemm's split-K limit (4096), where one wave walks the four quarters of K = 256 (these launches took
    # ONE chain until the switch-form test at this B showed them to differ from Fwd12Op)
    cs += [_case([17, 256, 256, 6], TANH3, B) for B in (4000, 4096, 4112)] + [_case([8, 256, 256, 4], RELU3, B) for B in (4096, 4112)]
    cs += [_case([17, 64, 64, 6], TANH3, 65536)]
    seen, out = set(), []
    for c in cs:
        if case_id(c) not in seen:
            seen.add(case_id(c)); out.append(c)
    return out


def is_fused_forward(dims):
    return len(dims) >= 3 and dims[0] <= 32 and dims[1] in (128, 192, 256) and dims[2] >= 16 and dims[2] % 16 == 0


def is_fused_backward(dims, B):
    return len(dims) >= 3 and dims[0] <= 16 and dims[1] >= 32 and dims[1] % 32 == 0 and dims[2] in (128, 192, 256) and 128 <= B <= 256


def perturbed_params(p, rng):
    """glorot weights with zero biases -> every parameter moved by N(0, 0.05): non-zero biases"""
    return (np.asarray(p, np.float32) + rng.normal(0, 0.05, np.asarray(p).size).astype(np.float32)).astype(np.float32)


def glorot_params(dims, rng):
    """host stand-in for a handle's initial parameters (CPU tests): glorot-uniform weights, zero biases"""
    p = np.zeros(n_layer_params(dims), np.float32)
    for l, (wo, bo) in enumerate(layer_offsets(dims)):
        lim = np.sqrt(6.0 / (dims[l] + dims[l + 1])); p[wo:bo] = rng.uniform(-lim, lim, bo - wo).astype(np.float32)
    return p


# The margin of the engine grid: a tensor passes iff err_gpu <= M x max(e32, u). M starts at 4 (two float32 summation orders of one length have errors of one distribution,
# and the fma contraction of the MFMA chain gets the rest); test_dense_reference.py runs the emulated engine order over every grid member with B <= 1000 and measures
# its ratio to max(e32, u). The worst ratio is 5.55 (db of layer 0, 33-128-128-2 at B = 1000: the reference's sgemv sums 1000 terms in several interleaved accumulators,
# the engine's sixteen chains of 62 terms meet partial sums of growing size; y 2.51, dx 2.37, dW 2.84), so M = 2 x 5.55. Chosen on the CPU, never fitted to the GPU.
M_EMULATED_WORST = 5.55
M_MARGIN = 2 * M_EMULATED_WORST
