"""Plain numpy restatement of prioritized replay (src/experience_buffer.jl:290-349): the yardstick of tests/test_gpu_per_tree.py, checked on the CPU by
tests/test_per_reference.py. Nothing here shares code with csrc/per.hip / csrc/per_tree.h:

  pairwise_cumsum   Base.cumsum of a Float32 vector (accumulate_pairwise!), the oracle's orc_pairwise_cumsum_f32 (pinned by test_oracle_golden.py)
  search            the sequential searchsortedfirst of :335-340, one binary search per stratum run in lock step (NOT np.searchsorted: the Float32 cumsum can be
                    locally non-monotone, and then only the probe sequence defines the answer)
  weights           the importance weights of :343-347 in Float64
  Model             priorities / max_priority / min_priority / elements / next_ind of a buffer that follows update_priorities! and push! through the oracle
  leaves            the leaves of the summation tree (the halving recursion on N - 1), to name a differing element's leaf and root path

Draws: u_j = u53(Philox(seed, i B + j, stream, SAMPLE)) (include/crux_rng.h), Philox4x32-10 vectorised over the counter.
"""
import ctypes as C

import numpy as np

import oracle as O
from crux_jl_amd import _lib as L

RNG_SAMPLE = 5
ONE_BELOW = 1.0 - 2.0 ** -53          # the largest Float64 draw below 1
_M = np.uint64(0xFFFFFFFF)


def pairwise_cumsum(pr):
    pr = np.ascontiguousarray(pr, np.float32); out = np.empty(pr.size, np.float32)
    O.lib().orc_pairwise_cumsum_f32(O.vpz(pr), pr.size, O.vpz(out))
    return out


def philox(seed, counter, stream, purpose):
    """Philox4x32-10 of crux_rng.h for an array of 64-bit counters: (4, n) uint32."""
    counter = np.asarray(counter, np.uint64).reshape(-1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    c0, c1 = counter & _M, counter >> np.uint64(32)
    c2 = np.full(counter.shape, stream, np.uint64); c3 = np.full(counter.shape, purpose, np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M, p1 >> np.uint64(32), p1 & _M
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M; k1 = (k1 + np.uint64(0xBB67AE85)) & _M
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def sample_rands(seed, i, B, stream=0):
    """the B Float64 uniforms prioritized_sample! draws with Philox counter i when no rands are injected"""
    x = philox(seed, np.uint64(i) * np.uint64(B) + np.arange(B, dtype=np.uint64), stream, RNG_SAMPLE)
    v = ((x[0].astype(np.uint64) << np.uint64(32)) | x[1].astype(np.uint64)) >> np.uint64(11)
    return v.astype(np.float64) * 1.1102230246251565e-16


def injected_rands(B, rng, flip=False):
    """B uniforms with the two edges in them: 0.0 in the first stratum (key 0: the first element) and 1 - 2^-53 in the last (the key passes the total whenever
    B * Float32(ptot / B) > ptot: the clamp). flip: the other way round (B = 1 holds one edge at a time)."""
    r = rng.random(B); r[0] = 0.0; r[-1] = ONE_BELOW if (B > 1 or flip) else 0.0
    return r[::-1].copy() if flip else r


def clamp_B(ptot, Bmax=1000):
    """the smallest B >= 2 whose stratum width rounds up, B * Float32(ptot / B) > ptot: with u = 1 - 2^-53 the last stratum's key (B + u - 1 = B in Float64) then
    passes the total and the search runs off the end"""
    ptot = np.float32(ptot)
    for B in range(2, Bmax + 1):
        if np.float64(B) * np.float64(ptot / np.float32(B)) > np.float64(ptot):
            return B
    raise AssertionError("no B <= %d rounds Float32(%r / B) up" % (Bmax, ptot))


def search(cumsum, B, rands, clamp=True):
    """ids[j] = searchsortedfirst(cumsum, (j + rands[j] - 1) * (ptot / B)) for j = 1..B (0-based result). The stratum width is Float32 / Int in Float32, the key
    Float64, every probe Float64(cumsum[mid]) < key. clamp: an index past the end becomes N - 1 (the reference would index out of bounds there)."""
    c = np.ascontiguousarray(cumsum, np.float32); N = c.size; B = int(B)
    u = np.asarray(rands, np.float64).reshape(-1); assert u.size == B and N >= 1
    dp = np.float64(np.float32(c[N - 1]) / np.float32(B))
    key = (np.arange(1, B + 1, dtype=np.float64) + u - 1.0) * dp
    lo = np.zeros(B, np.int64); hi = np.full(B, N, np.int64)
    while True:
        act = lo < hi
        if not act.any():
            break
        mid = lo + ((hi - lo) >> 1)
        lt = c[np.minimum(mid, N - 1)].astype(np.float64) < key
        lo = np.where(act & lt, mid + 1, lo); hi = np.where(act & ~lt, mid, hi)
    return np.minimum(lo, N - 1) if clamp else lo


def weights(pr, ids, ptot, min_priority, N, beta):
    """(N priorities[ids] / ptot)^beta / (N min_priority / ptot)^-beta ... in Float64 (:343-347: pmin = min_priority / ptot, max_w = (pmin N)^-beta)"""
    pr = np.asarray(pr, np.float64); ptot, beta = np.float64(ptot), np.float64(beta)
    max_w = (np.float64(min_priority) / ptot * N) ** (-beta)
    return (N * pr[np.asarray(ids, np.int64)] / ptot) ** beta / max_w


def leaves(N):
    """[(first element, length, level)] of accumulate_pairwise!'s leaves over elements 1 .. N - 1 (0-based; element 0 is the seed outside the tree), in memory order"""
    out = []

    def rec(i1, n, lvl):
        if n < 128:
            out.append((i1, n, lvl)); return
        n2 = n >> 1; rec(i1, n2, lvl + 1); rec(i1 + n2, n - n2, lvl + 1)
    if N >= 2:
        rec(1, N - 1, 0)
    return out


def locate(N, e):
    """(leaf number, first element, length, level, heap number) of element e >= 1"""
    i1, n, lvl, heap = 1, N - 1, 0, 1
    while n >= 128:
        n2 = n >> 1
        if e >= i1 + n2:
            i1, n, heap = i1 + n2, n - n2, 2 * heap + 1
        else:
            n, heap = n2, 2 * heap
        lvl += 1
    k = [s for s, _, _ in leaves(N)].index(i1)
    return k, i1, n, lvl, heap


class Model:
    """the priority state of a prioritized ExperienceBuffer of `capacity` rows, kept by the oracle's update_priorities! / push! (an O.OBuffer with the
    narrowest columns: the rows themselves are not under test)"""

    def __init__(self, capacity, alpha=0.6):
        self.cap = int(capacity)
        self.ob = O.OBuffer(1, 1, L.ACTION_CONTINUOUS, self.cap, ["weight"], prioritized=True, alpha=np.float32(alpha))

    def update(self, ids0, v):
        """update_priorities!(b, ids0 + 1, v): v Float64 or Float32 (the dtype is significant), sequential, the last write of a repeated id wins"""
        I = np.ascontiguousarray(ids0, np.int64); v = np.ascontiguousarray(v)
        is64 = v.dtype == np.float64
        if not is64:
            v = v.astype(np.float32)
        O.chk(O.lib().orc_per_update(self.ob.h, O.vpz(I), O.vpz(v), 1 if is64 else 0, I.size))

    def push(self, n):
        """push! of n rows: they land at next_ind .. next_ind + n - 1 (mod capacity) with (max_priority + eps)^alpha, max_priority read once before"""
        z = np.zeros((1, n), np.float32)
        return self.ob.push({"s": z, "a": z, "sp": z, "r": z, "done": np.zeros((1, n), bool)}) - 1

    def _get(self):
        pr = np.empty(self.cap, np.float32); mx, mn = C.c_float(), C.c_float()
        O.chk(O.lib().orc_per_get(self.ob.h, O.vpz(pr), C.byref(mx), C.byref(mn), None))
        return pr, mx.value, mn.value

    @property
    def priorities(self):
        return self._get()[0]

    @property
    def max_priority(self):
        return self._get()[1]

    @property
    def min_priority(self):
        return self._get()[2]

    @property
    def elements(self):
        return len(self.ob)

    @property
    def next_ind(self):
        return int(O.lib().orc_buffer_next_ind(self.ob.h))

    def sample(self, B, rands=None, beta=0.5, i=1, seed=0):
        """orc_per_sample into a scratch target: (ids, the source's :weight column afterwards) -- the CPU test's check of search / weights"""
        to = O.OBuffer(1, 1, L.ACTION_CONTINUOUS, B, ["weight"])
        r = None if rands is None else np.ascontiguousarray(rands, np.float64)
        O.chk(O.lib().orc_per_sample(to.h, self.ob.h, B, O.vpz(r), beta, i, seed))
        ids = np.empty(B, np.int64); O.chk(O.lib().orc_buffer_indices(to.h, O.vpz(ids), B))
        return ids, self.ob.col("weight")[0].copy()
