"""The prioritized buffer's INCREMENTAL pairwise-cumsum tree (csrc/per.hip, csrc/per_tree.h, PerUpdateOp) against a model that shares nothing with it
(tests/per_reference.py, checked on the CPU by tests/test_per_reference.py).

One driver (Tree) applies a seeded sequence of mutations to a prioritized crux.ExperienceBuffer and to the model, and after EVERY mutation asserts the invariant:
  (1) priorities bit-identical to the model at every row (so untouched rows are unchanged), max_priority / min_priority equal. A row the mutation wrote may differ
      from the host's pow by one Float32 ulp; that is printed as a finding (profiles/per_tree_tests.txt) and never extends to rows the mutation did not write;
  (2) buf.cumsum() -- materialised from run[] and the node totals -- == accumulate_pairwise! of the priorities READ BACK FROM THE GPU, bit for bit. Independent of (1);
  (3) every few mutations and after the last: prioritized_sample_ with injected draws (0.0 and 1 - 2^-53 among them) and with Philox draws, B in {1, 3, 5, 128, 1000} and
      the B that reaches the clamp: ids == per_reference.search over the reference cumsum, gathered rows == the source's rows, weights within 4e-7 max(1, max w).
Every mutation kind is counted and the counts are asserted at the end of each case. Nothing is skipped or filtered, with one exception that the API sets: steps! rejects
a block of more transitions than the ring holds, so a rollout of n steps exists only where n <= N (asserted to be rejected otherwise)."""
import collections
import time

import numpy as np
import pytest

import crux_jl_amd as crux
from crux_jl_amd import _lib as L
import oracle as O
import parity
import per_reference as R

pytestmark = pytest.mark.gpu

OD, AD = 8, 4
SMALL_N = [2, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097]
LARGE_N = [65_536, 100_003, 1_000_000]
B_GRID = [1, 3, 5, 128, 1000]
UPDATE_N = [2, 64, 128, 256, 257, 1024, 1025, 4096, 4097]      # LeafRefreshOp grids, both TreeTouchOp branches (n <= / > 1024 threads), the 4096-id limit of crux_per_touched
PUSH_N = [1, 4, 32, 33, 256, 257, 5000]


def _explain(N, c, ref, what):
    """which element, leaf and level of the root path a cumsum difference starts at"""
    d = np.flatnonzero(c.view(np.uint32) != ref.view(np.uint32)); i = int(d[0])
    if i == 0:
        return "%s: cumsum[0] (the seed element outside the tree) differs" % what
    k, i1, n, lvl, heap = R.locate(N, i)
    a1, an, al, where = 1, N - 1, 0, None
    while where is None:                                       # the shallowest node whose span starts at i: its LEFT sibling's total is what the prefix of i picked up
        if a1 == i and al > 0:
            where = "the span of a level-%d node starts there: the total of its left sibling (level %d of the root paths) is stale" % (al, al)
        elif an < 128:
            where = "inside the leaf: its running sums are stale"
        else:
            n2 = an >> 1
            a1, an = (a1 + n2, an - n2) if i >= a1 + n2 else (a1, n2)
            al += 1
    return "%s: N = %d, %d elements differ, first %d, last %d; first is in leaf %d (elements %d..%d, level %d, heap node %d); %s; got %r want %r" % (
        what, N, d.size, i, int(d[-1]), k, i1, i1 + n - 1, lvl, heap, where, c[i], ref[i])


class Tree:
    def __init__(self, N, seed, od=OD, ad=AD, discrete=True):
        self.N, self.od, self.ad, self.discrete = N, od, ad, discrete
        self.rng = np.random.default_rng(seed)
        S = crux.ContinuousSpace(od); A = crux.DiscreteSpace(ad) if discrete else crux.ContinuousSpace(ad)
        self.buf = crux.ExperienceBuffer(S, A, N, prioritized=True)
        self.tg = crux.ExperienceBuffer(S, A, 1000, ["weight"])
        self.model = R.Model(N)
        self.counts = collections.Counter(); self.expected = set()
        self.loose = np.zeros(0, np.int64); self.pow_findings = []
        self.i_sample = 0; self.i_roll = 0; self.clamped = self.first = self.samples = 0
        self.t0 = time.time()

    # ---- mutations -----------------------------------------------------------------------------------------------------------------
    def data(self, n):
        rng = self.rng
        if self.discrete:
            a = np.zeros((self.ad, n), bool); a[rng.integers(0, self.ad, n), np.arange(n)] = True
        else:
            a = rng.standard_normal((self.ad, n)).astype(np.float32)
        return {"s": rng.standard_normal((self.od, n)).astype(np.float32), "a": a, "sp": rng.standard_normal((self.od, n)).astype(np.float32),
                "r": rng.standard_normal((1, n)).astype(np.float32), "done": rng.random((1, n)) < 0.05}

    def values(self, n, f64):
        v = np.abs(self.rng.standard_normal(n)) * self.rng.choice([1e-3, 1.0, 30.0], n) + 1e-4
        return v if f64 else v.astype(np.float32)

    def push(self, n, kind):
        I = self.buf.push_(self.data(n)) - 1; Im = self.model.push(n)
        assert np.array_equal(I, Im), kind
        self.invariant(kind, I)

    def update(self, ids0, v, kind):
        ids0 = np.asarray(ids0, np.int64)
        self.buf.update_priorities_(ids0 + 1, v); self.model.update(ids0, v)
        self.invariant(kind, ids0)

    def steps(self, sampler, n, kind):
        first = self.buf.next_ind - 1; self.i_roll += n
        crux.steps_(sampler, self.buf, Nsteps=n, explore=True, i=self.i_roll)
        I = (first + np.arange(n)) % self.N
        assert np.array_equal(self.model.push(n), I), kind          # the model takes the rows the GPU wrote: only the priority bookkeeping is under test here
        self.invariant(kind, I)

    def stir(self, n):
        """fresh priorities for the rows the next push of n rows will overwrite: pushes all carry (max_priority + eps)^alpha, so a row that a push one lap earlier
        wrote already holds the value the next one stores, and a leaf re-summed from the STALE row would still come out right"""
        rows = (self.buf.next_ind - 1 + np.arange(min(n, self.N))) % self.N
        self.update(rows, self.values(rows.size, False), "update_rows_ahead")

    def align(self, row):
        """move next_ind to `row` with a push of its own (a mutation like any other)"""
        m = (row - (self.buf.next_ind - 1)) % self.N
        if m:
            self.push(m, "push_align")

    # ---- the invariant -------------------------------------------------------------------------------------------------------------
    def invariant(self, kind, touched, count=True):
        what = "mutation %d (%s, %d ids)" % (sum(self.counts.values()) + 1, kind, len(touched))
        if count:
            self.counts[kind] += 1
        buf, m = self.buf, self.model
        n = len(buf); assert n == m.elements and buf.next_ind - 1 == m.next_ind, what
        pp = buf.priority_params(); pg, pm = pp["priorities"], m.priorities
        bad = np.flatnonzero(pg.view(np.uint32) != pm.view(np.uint32))
        if bad.size:                                            # (1): only rows this mutation wrote (or rows found off by an ulp before and not rewritten since) may differ, by one ulp
            fresh = np.setdiff1d(bad, self.loose)
            assert np.isin(fresh, touched).all(), "%s: rows it did not write changed: %s" % (what, np.setdiff1d(fresh, touched)[:8])
            ulp = np.abs(pg.view(np.int32)[bad].astype(np.int64) - pm.view(np.int32)[bad].astype(np.int64))
            assert ulp.max() <= 1, "%s: priorities differ from the model by more than one ulp at rows %s: %r vs %r" % (what, bad[ulp > 1][:8], pg[bad[ulp > 1][:8]], pm[bad[ulp > 1][:8]])
            for r in fresh:
                self.pow_findings.append((what, int(r), float(pg[r]), float(pm[r])))
        self.loose = bad
        assert pp["max_priority"] == m.max_priority and pp["min_priority"] == m.min_priority, what
        c = buf.cumsum(); ref = R.pairwise_cumsum(pg[:n])       # (2)
        assert c.shape == ref.shape and np.array_equal(c.view(np.uint32), ref.view(np.uint32)), _explain(n, c, ref, what)
        return pp, ref

    def sample(self, B, rands, pp, ref):
        n = len(self.buf); pr = pp["priorities"][:n]
        self.i_sample += 1; i = self.i_sample; self.samples += 1
        self.tg.clear_()
        ids = crux.prioritized_sample_(self.tg, self.buf, B=B, i=i, rands=rands) - 1
        u = rands if rands is not None else R.sample_rands(crux.api.SAMPLE_SEED, i, B)
        raw = R.search(ref, B, u, clamp=False); want = np.minimum(raw, n - 1)
        self.clamped += int((raw >= n).sum()); self.first += int((want == 0).sum())
        what = "sample %d (N = %d, B = %d, %s draws)" % (self.samples, n, B, "Philox" if rands is None else "injected")
        assert np.array_equal(ids, want), "%s: ids differ at strata %s" % (what, np.flatnonzero(ids != want)[:8])
        rows = {k: self.buf[k][:, ids] for k in self.buf.keys()} if n <= 4097 else self.buf.minibatch(ids + 1)
        for k in self.tg.keys():
            if k != "weight":
                assert np.array_equal(self.tg[k], rows[k]), "%s: column %s" % (what, k)
        w = R.weights(pr, want, ref[n - 1], pp["min_priority"], n, 0.5); tol = 4e-7 * max(1.0, w.max())
        assert np.abs(self.tg["weight"][0] - w).max() <= tol and np.abs(rows["weight"][0] - w).max() <= tol, what

    def sample_round(self):
        pp, ref = self.invariant("sample", (), count=False)
        n = len(self.buf); flip = bool(self.samples & 1)
        for B in B_GRID + [R.clamp_B(ref[n - 1])]:
            self.sample(B, R.injected_rands(B, self.rng, flip=flip), pp, ref)
            self.sample(B, None, pp, ref)
        self.invariant("sample", (), count=False)              # sampling changes no priority and leaves the tree as it was

    def finish(self, name, extra=()):
        self.sample_round()
        self.expected |= set(extra)
        missing = [k for k in sorted(self.expected) if self.counts[k] == 0]
        assert not missing and self.samples > 0 and self.first > 0 and self.clamped > 0, (missing, self.samples, self.first, self.clamped)
        print("\n[per-tree] %s N=%d: %d mutations %s; %d samples (%d clamped strata, %d first-element hits); pow-ulp findings %d %s; %.2f s" % (
            name, self.N, sum(self.counts.values()), dict(sorted(self.counts.items())), self.samples, self.clamped, self.first, len(self.pow_findings), self.pow_findings[:3],
            time.time() - self.t0))


# ---- mutation lists ------------------------------------------------------------------------------------------------------------------
def _fill(t, n=None):
    n = t.N if n is None else n
    t.push(n, "push_fill")
    t.update(np.arange(n), t.values(n, True), "update_all")


def _edge_rows(N):
    """row 0 (the seed outside the tree), row 1, row N - 1, the first and the last element of the first, a middle and the last leaf"""
    lv = R.leaves(N); rows = [0, 1, N - 1]
    for i1, n, _ in (lv[0], lv[len(lv) // 2], lv[-1]):
        rows += [i1, i1 + n - 1]
    return [r for r in rows if 0 <= r < N]


def _single_updates(t):
    for j, r in enumerate(_edge_rows(t.N)):
        t.update([r], t.values(1, j % 2 == 0), "update_single")
    t.expected.add("update_single")


def _sized_updates(t):
    N = t.N
    for n in UPDATE_N:
        for f64, sort in ((False, True), (True, False)):
            ids = t.rng.choice(N, n, replace=n > N)               # more ids than rows: they repeat, with different values -- the last write wins
            t.update(np.sort(ids) if sort else ids, t.values(n, f64), "update_n")
    i1, n, _ = R.leaves(N)[len(R.leaves(N)) // 2]
    t.update(i1 + t.rng.permutation(n)[:max(1, min(n, 64))], t.values(max(1, min(n, 64)), False), "update_one_leaf")
    t.expected |= {"update_n", "update_one_leaf"}


def _duplicate_updates(t):
    N = t.N; rows = t.rng.choice(N, min(N, 40), replace=False)
    for sort in (True, False):
        ids = rows[t.rng.integers(0, rows.size, 300)]
        t.update(np.sort(ids) if sort else ids, t.values(300, not sort), "dup_small_sorted" if sort else "dup_small_unsorted")
    rows = t.rng.choice(N, min(N, 64), replace=False)
    for f64 in (False, True):
        t.update(rows[t.rng.integers(0, rows.size, 2048)], t.values(2048, f64), "dup_large")       # 2048 ids over <= 64 rows, all values different
    t.expected |= {"dup_small_sorted", "dup_small_unsorted", "dup_large"}


def _placed(t, n, do):
    """run do() three times: so that the n rows end exactly at the ring end, wrap across it, and start at row 0"""
    N = t.N
    for row in ((N - n) % N, (N - max(1, n // 2)) % N, 0):
        t.align(row); t.stir(n); do()


def _host_pushes(t, sizes=PUSH_N):
    for n in sizes:
        _placed(t, n, lambda: t.push(n, "push_full_ring"))
    t.expected |= {"push_full_ring", "push_align", "update_rows_ahead"}


def _sampler(n_envs, dims, seed=11):
    q = crux.DiscreteNetwork(parity.chain(dims, ["relu"] * (len(dims) - 2) + ["identity"]), list(range(1, AD + 1)), seed=seed)
    mdp = crux.SynthMDP(OD, AD, discrete=True, n_envs=n_envs, seed=seed)
    pe = crux.EpsGreedyPolicy(crux.LinearDecaySchedule(1.0, 0.1, 100), list(range(AD)))
    return crux.Sampler(mdp, crux.PolicyParams(q, pi_explore=pe), max_steps=20)


def _rollouts(t, monkeypatch):
    """steps! into the prioritized ring: the only way to the fused push bodies"""
    N = t.N
    res1, res2, gen1 = _sampler(1, [8, 256, 256, 4]), _sampler(2, [8, 256, 256, 4]), _sampler(1, [8, 32, 4])
    cases = [(res1, [1, 2, 4, 31, 32], "rollout_res_small"),          # push_touch_small at the end of k_rollout_res (one step: k_push_touch_small behind the generic rollout)
             (res1, [33, 256], "rollout_res_block"),                  # push_touch_block, touch = 1
             (res2, [2, 4, 32], "rollout_fused_small"),               # two environments: k_push_touch_small through crux_per_push_fused
             (res2, [34, 256], "rollout_fused_block"),                # k_push_touch
             (gen1, [4, 33], "rollout_fused_generic")]                # a network outside the resident kernel
    for smp, sizes, kind in cases:
        for n in sizes:
            if n > N:
                with pytest.raises(crux.CruxError):                   # steps!: a block larger than the ring is refused, there is nothing to check
                    crux.steps_(smp, t.buf, Nsteps=n, explore=True)
                continue
            t.expected.add(kind)
            _placed(t, n, lambda: t.steps(smp, n, kind))
    monkeypatch.setenv("CRUX_PUSH_FUSED", "0")                         # the separate launches: ring ids, snapshot, PerUpdateOp, LeafRefreshOp, TreeTouchOp
    for n in (4, 33, 300):
        if n <= N:
            t.expected.add("rollout_separate")
            _placed(t, n, lambda: t.steps(res1, n, "rollout_separate"))
    monkeypatch.delenv("CRUX_PUSH_FUSED")
    return res1


def _interleaved(t, smp):
    N = t.N
    for rep in range(3):
        t.update(t.rng.choice(N, min(N, 7), replace=False), t.values(min(N, 7), False), "inter_update"); t.sample_round()
        t.stir(1 + rep * 3); t.push(1 + rep * 3, "inter_push")
        t.update([int(t.rng.integers(0, N))], t.values(1, True), "inter_update"); t.sample_round()
        if N >= 4:
            t.stir(4); t.steps(smp, 4, "inter_rollout"); t.expected.add("inter_rollout")
        t.update(t.rng.choice(N, min(N, 128), replace=False), t.values(min(N, 128), False), "inter_update")
    t.expected |= {"inter_update", "inter_push"}


ALL_KINDS = {"push_fill", "update_all", "update_single", "update_n", "update_one_leaf", "dup_small_sorted", "dup_small_unsorted", "dup_large", "push_full_ring", "push_align", "update_rows_ahead",
             "rollout_res_small", "rollout_res_block", "rollout_fused_small", "rollout_fused_block", "rollout_fused_generic", "rollout_separate", "inter_update", "inter_push",
             "inter_rollout"}


@pytest.mark.parametrize("N", SMALL_N)
def test_incremental_tree_follows_the_model_through_the_whole_mutation_list(gpu_ctx, monkeypatch, N):
    t = Tree(N, seed=N)
    _fill(t); t.expected |= {"push_fill", "update_all"}
    t.sample_round()
    _single_updates(t); t.sample_round()
    _sized_updates(t); t.sample_round()
    _duplicate_updates(t); t.sample_round()
    _host_pushes(t); t.sample_round()
    smp = _rollouts(t, monkeypatch); t.sample_round()
    _interleaved(t, smp)
    if N >= 300:
        assert t.expected == ALL_KINDS, ALL_KINDS - t.expected        # from 300 rows on no rollout size is refused: the whole list ran
    t.finish("whole list")


@pytest.mark.parametrize("N", SMALL_N)
def test_ring_that_fills_changes_the_tree_with_every_push(gpu_ctx, N):
    """pushes while the ring fills (the tree's N and topology change), an update at and beyond len(buf), the push that exactly fills the ring, and -- a second ring -- the push
    that crosses from filling to full and wraps"""
    for cross in (False, True):
        t = Tree(N, seed=2 * N + cross)
        a = max(1, N // 3)
        t.push(a, "push_filling"); t.update(np.arange(a), t.values(a, True), "update_filling"); t.sample_round()
        if N >= 4:
            t.push(a, "push_filling"); t.sample_round()
        n = len(t.buf)
        if n < N:                                                    # ids at or beyond len(buf) on a part-filled ring: outside the current tree (in_tree = false -> rebuild)
            ids = np.unique(np.concatenate([[n, N - 1], t.rng.integers(0, N, 5)]))
            t.update(ids, t.values(ids.size, False), "update_beyond_len"); t.expected.add("update_beyond_len")
            t.update([0], t.values(1, False), "update_filling")
        if cross:
            t.push(N - n + max(1, N // 4), "push_cross_and_wrap"); t.expected.add("push_cross_and_wrap")
            assert len(t.buf) == N and t.buf.next_ind - 1 == max(1, N // 4) % N
        else:
            t.push(N - n, "push_fills_exactly"); t.expected.add("push_fills_exactly")
            assert len(t.buf) == N and t.buf.next_ind == 1
        t.update([0, N - 1], t.values(2, False), "update_after_fill")
        t.push(min(N, 4), "push_after_fill")
        t.update(t.rng.choice(N, min(N, 64), replace=False), t.values(min(N, 64), True), "update_after_fill")
        t.finish("filling ring, %s" % ("crossing" if cross else "exact"), {"push_filling", "update_filling", "update_after_fill", "push_after_fill"})


@pytest.mark.parametrize("N", LARGE_N)
def test_incremental_tree_at_large_sizes(gpu_ctx, N):
    """the reduced list: single ids at the edges, one 128-id update, pushes of 4 and 256 rows with a wrap, one round of samples"""
    t = Tree(N, seed=N)
    _fill(t)
    _single_updates(t)
    t.update(t.rng.choice(N, 128, replace=False), t.values(128, False), "update_n")
    for n in (4, 256):
        t.align(N - n // 2); t.stir(n); t.push(n, "push_full_ring")
    t.finish("reduced list", {"push_fill", "update_all", "update_n", "push_full_ring", "push_align", "update_rows_ahead"})


def test_three_million_rows_take_the_global_memory_tree_pass(gpu_ctx):
    """N = 3 000 001: 16 levels (still <= CRUX_PER_PMAX), node totals past the LDS-resident pass (k_tree): a 128-id update on the rebuilt tree, invariant (2)"""
    N = 3_000_001; rng = np.random.default_rng(N); t0 = time.time()
    b = crux.ExperienceBuffer(crux.ContinuousSpace(1), crux.DiscreteSpace(2), N, prioritized=True)
    a = np.zeros((2, N), bool); a[0] = True; z = np.zeros((1, N), np.float32)
    b.push_({"s": z, "a": a, "sp": z, "r": z, "done": np.zeros((1, N), bool)})
    b.update_priorities_(np.arange(1, N + 1), (np.abs(rng.standard_normal(N)) + 1e-3).astype(np.float32))
    for rep in range(2):
        c = b.cumsum(); ref = R.pairwise_cumsum(b.priority_params()["priorities"])
        assert np.array_equal(c.view(np.uint32), ref.view(np.uint32)), _explain(N, c, ref, "3 M rows, %s" % ("rebuild" if rep == 0 else "128-id update"))
        if rep == 0:
            ids = np.concatenate([[0, 1, N - 1], rng.choice(N, 125, replace=False)])
            b.update_priorities_(ids + 1, (np.abs(rng.standard_normal(128)) + 1e-3).astype(np.float32))
    print("\n[per-tree] 3 000 001 rows: rebuild + 128-id update, %.2f s" % (time.time() - t0))


@pytest.mark.parametrize("N", [256, 4096])          # leaves on two levels (lengths 64 and 127 mixed)
def test_two_hundred_mixed_small_mutations_on_a_two_level_tree(gpu_ctx, N):
    assert len({l for _, _, l in R.leaves(N)}) == 2
    t = Tree(N, seed=7 * N); _fill(t)
    smp = _sampler(1, [8, 256, 256, 4])
    for j in range(240):
        k = int(t.rng.integers(0, 6))
        if k == 0:
            t.update([int(t.rng.integers(0, N))], t.values(1, bool(j & 1)), "mix_update_single")
        elif k == 1:
            n = int(t.rng.integers(2, 65)); t.update(t.rng.choice(N, n, replace=False), t.values(n, bool(j & 1)), "mix_update_small")
        elif k == 2:
            n = int(t.rng.integers(1, 33)); t.stir(n); t.push(n, "mix_push")
        elif k == 3:
            n = int(t.rng.integers(1, 33)); t.stir(n); t.steps(smp, n, "mix_rollout_small")
        elif k == 4:
            n = int(t.rng.integers(33, 100)); t.stir(n); t.steps(smp, n, "mix_rollout_block")
        else:
            n = int(t.rng.integers(2, 200)); t.update(t.rng.integers(0, N, n), t.values(n, False), "mix_update_repeats")
        if j % 30 == 29:
            t.sample_round()
    assert sum(t.counts.values()) >= 200
    t.finish("mixed", {"mix_update_single", "mix_update_small", "mix_push", "mix_rollout_small", "mix_rollout_block", "mix_update_repeats", "update_rows_ahead"})


@pytest.mark.parametrize("N", [4096, 20_000])       # leaves on two levels / on one level
def test_chained_dqn_epochs_leave_a_tree_that_sums_its_priorities(gpu_ctx, N):
    """crux_dqn_epochs, 4 epochs on a full ring (LeafTouchOp: leaves and root paths as one op behind a ticket). The priorities come from the GPU's td errors, so there is no
    model for (1); (2) needs none -- the check the chained-against-separate comparison (test_gpu_round2.py) cannot make."""
    rng = np.random.default_rng(N); B = 128; t0 = time.time()
    S, A = crux.ContinuousSpace(OD), crux.DiscreteSpace(AD)
    buf = crux.ExperienceBuffer(S, A, N, prioritized=True); D = crux.buffer_like(buf, capacity=B)
    a = np.zeros((AD, N), bool); a[rng.integers(0, AD, N), np.arange(N)] = True
    buf.push_({"s": rng.normal(0, 1, (OD, N)).astype(np.float32), "a": a, "sp": rng.normal(0, 1, (OD, N)).astype(np.float32), "r": rng.normal(0, 1, (1, N)).astype(np.float32),
               "done": rng.random((1, N)) < 0.02, "episode_end": np.zeros((1, N), bool)})
    buf.update_priorities_(np.arange(1, N + 1), (np.abs(rng.normal(0, 1, N)) + 1e-3).astype(np.float32))
    q = crux.DiscreteNetwork(parity.chain([8, 256, 256, 4], ["relu", "relu", "identity"]), [1, 2, 3, 4], seed=5)
    qm = crux.clone_policy(q); q.attach_optimizer(crux.Adam(np.float32(1e-3)))
    before = buf.priority_params()["priorities"].copy()
    for call in range(3):
        infos = np.zeros((4, L.INFO_N), np.float32)
        q.ctx.check(q.ctx.lib.crux_dqn_epochs(q.h, qm.h, buf.h, D.h, 0.99, 1, 0.6, 40 + 4 * call, 4, O.vpz(infos)))
        pr = buf.priority_params()["priorities"]; c = buf.cumsum(); ref = R.pairwise_cumsum(pr[:N])
        assert np.array_equal(c.view(np.uint32), ref.view(np.uint32)), _explain(N, c, ref, "chained epochs, call %d" % call)
    assert (pr != before).sum() >= B                                  # the epochs did rewrite priorities
    print("\n[per-tree] chained epochs N=%d: 3 calls of 4 epochs, %d priorities rewritten, %.2f s" % (N, int((pr != before).sum()), time.time() - t0))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_rows_wider_than_one_wave_are_gathered_whole(gpu_ctx, monkeypatch, fused):
    """obs_dim 40 and 6 continuous actions: a row of more than 64 four-byte elements (the second loop of PerSampleGatherOp), CRUX_PER_FUSED_GATHER on and off"""
    monkeypatch.setenv("CRUX_PER_FUSED_GATHER", fused)
    t = Tree(1000, seed=40 + int(fused), od=40, ad=6, discrete=False)
    _fill(t); t.sample_round()
    t.update(t.rng.choice(1000, 128, replace=False), t.values(128, False), "update_n"); t.sample_round()
    t.stir(37); t.push(37, "push_full_ring")
    t.finish("wide rows, fused gather %s" % fused, {"push_fill", "update_all", "update_n", "push_full_ring", "update_rows_ahead"})
