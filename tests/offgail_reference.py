"""Float64 restatement of OffPolicyGAIL's discriminator loss and reward (src/model_free/il/off_policy_gail.jl:64-125) with torch autograd, of the row draws of its
minibatches (include/crux_rng.h) and of AdRIL's callback (src/model_free/il/AdRIL.jl:39-50) on a host ring: the yardstick of tests/test_gpu_offgail.py.

Draws: row j of source k in discriminator epoch `counter` is id = (Philox(seed, counter Bd + j, 16 + k, SAMPLE).v[0] * len_k) >> 32, which is what uniform_sample!
draws for the same (key, stream, counter) (csrc/per.hip, k_uniform_ids).
"""
import numpy as np
import torch

import iq_reference as IR

RNG_SAMPLE = 5
STREAM0 = 16
_M = np.uint64(0xFFFFFFFF)
mlp_params, mlp, adam_first_step, flat_grad = IR.mlp_params, IR.mlp, IR.adam_first_step, IR.flat_grad
EPS = np.float32(1e-5)
TERM_BOUND = float(np.log(1.0 + 1e-5) - np.log(1e-5))      # |log(p + 1e-5) - log(1 - p + 1e-5)| <= this for p in [0, 1]: 11.5129...


def philox_counters(seed, counters, stream, purpose):
    """Philox4x32-10 of crux_rng.h for an array of 64-bit counters and one stream: (4, n) uint32."""
    ctr = np.asarray(counters, np.uint64).reshape(-1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1 = ctr & _M, ctr >> np.uint64(32)
    c2 = np.full(ctr.shape, stream, np.uint64); c3 = np.full(ctr.shape, purpose, np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M, p1 >> np.uint64(32), p1 & _M
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M; k1 = (k1 + np.uint64(0xBB67AE85)) & _M
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def sample_ids(seed, stream, counter, Bd, n):
    """0-based rows uniform_sample!(target, source; B=Bd) draws from a source of length n with (key, stream, counter)"""
    x = philox_counters(seed, np.uint64(counter) * np.uint64(Bd) + np.arange(Bd, dtype=np.uint64), stream, RNG_SAMPLE)
    return ((x[0].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def gather(sources, Bd, seed, counter):
    """X = hcat over the sources of vcat(s, a)[:, ids_k]: sources are dicts of host columns (s [od x n], a [ad x n], bool one-hot or float)"""
    cols = []
    for k, src in enumerate(sources):
        ids = sample_ids(seed, STREAM0 + k, counter, Bd, src["s"].shape[1])
        cols.append(np.concatenate([src["s"][:, ids].astype(np.float32), src["a"][:, ids].astype(np.float32)], axis=0))
    return np.concatenate(cols, axis=1)


def labels(K, Bd):
    """the class of every column of hcat(D_demo_batch, D_batch, D_ndas_batch...): its source (:87-93)"""
    return np.repeat(np.arange(K), Bd)


def ce_loss(layers, acts, X, K, Bd):
    """Flux.Losses.logitcrossentropy(D(x), y) = mean_j (logsumexp z_j - z_j[label_j]) in float64, with the graph"""
    z = mlp(layers, acts, torch.as_tensor(np.asarray(X, np.float64)))
    lab = torch.as_tensor(labels(K, Bd))
    return (torch.logsumexp(z, 0) - z[lab, torch.arange(z.shape[1])]).mean()


def ce_seed(z, K, Bd):
    """dL/dz in closed form: (softmax(z) - onehot(label)) / N"""
    z = np.asarray(z, np.float64); N = z.shape[1]
    p = np.exp(z - z.max(0)); p /= p.sum(0)
    p[labels(K, Bd), np.arange(N)] -= 1.0
    return p / N


def weights(K):
    """w = [1f0, 0f0, λ_nda * ones(N_nda)...], λ_nda = Float32(-1 / N_nda) (:35, :122)"""
    return np.array([1.0, 0.0] + ([float(np.float32(-1.0 / (K - 2)))] * (K - 2) if K > 2 else []))


def reward(z, dtype=np.float64):
    """sum((log.(softmax(z) .+ 1f-5) .- log.(1f0 .- softmax(z) .+ 1f-5)) .* w, dims=1) (:121-124) in `dtype`, operand order as written"""
    z = np.asarray(z, dtype); K = z.shape[0]; one, eps = dtype(1), dtype(EPS)
    e = np.exp(z - z.max(0)); p = (e / e.sum(0)).astype(dtype)
    t = (np.log(p + eps) - np.log((one - p) + eps)) * weights(K).astype(dtype)[:, None]
    acc = t[0]
    for k in range(1, K):
        acc = (acc + t[k]).astype(dtype)
    return acc


# ---- AdRIL on a host ring, callback THEN push, as the reference runs it (sampler.jl:150-152) ---------------------------------------------------------------------
class HostRing:
    """the :i and :r columns of an ExperienceBuffer of `capacity` (experience_buffer.jl:232-259: ring push, elements, next_ind)"""

    def __init__(self, capacity):
        self.capacity, self.elements, self.next_ind = int(capacity), 0, 0
        self.i, self.r = np.zeros(capacity, np.int64), np.zeros(capacity, np.float32)

    def __len__(self):
        return self.elements

    def push(self, i, r):
        for a, b in zip(i, r):
            self.i[self.next_ind], self.r[self.next_ind] = a, b
            self.next_ind = (self.next_ind + 1) % self.capacity; self.elements = min(self.elements + 1, self.capacity)


def adril_callback(D_i, D_r, ring, buffer_init, dN):
    """AdRIL_callback(𝒟; 𝒮) (AdRIL.jl:39-50), line by line. Raises ValueError where Int(...) raises InexactError; leaves ring and D untouched then
    except for D[:r] .= 0, which the reference has already done (the block is never pushed: the error unwinds steps!)."""
    D_r[...] = 0                                                                  # :40
    if len(ring) > 0:                                                             # :42
        n = len(ring)
        max_i = max(int(D_i.max()), int(ring.i[:n].max()))                        # :43
        q = (max_i - buffer_init) / dN                                            # :44 Float64 quotient
        if q != int(q):
            raise ValueError("InexactError: Int(%r)" % q)
        k = int(q) - 1
        old = ring.i[:n] <= max_i - dN                                            # :45
        with np.errstate(divide="ignore"):
            val = np.float32(np.float64(-1.0) / np.float64(k)) if k != 0 else np.float32(-np.inf)      # -1/k: Float64, stored into a Float32 column; k == 0: -Inf
        ring.r[:n][old] = val                                                     # :47
        ring.r[:n][~old] = 0                                                      # :48


def adril_steps(ring, new_i, buffer_init, dN):
    """one steps! of the reference: the fresh block (its :i values given, rewards arbitrary), cb(data), then push!(buffer, data)"""
    D_i = np.asarray(new_i, np.int64); D_r = np.full(D_i.shape, 7.0, np.float32)      # whatever the environment paid: the callback zeroes it
    adril_callback(D_i, D_r, ring, buffer_init, dN)
    ring.push(D_i, D_r)
