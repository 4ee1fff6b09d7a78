"""The case table of tests/rollout_res_cases.py, checked without a GPU: every call with T >= 2 meets the dispatch condition of k_rollout_res and no call with T = 1 does, no
row under comparison is overwritten, the oracle's trajectory of every case CONTAINS the events the case is named for, and the discrete decisions of every case survive
1e-5 relative noise on every parameter. Nothing here runs a kernel: the oracle alone.

The decision margin is a condition on the chosen seeds, not a measurement: the fused-multiply-add forward of the kernels and the unfused oracle differ at the 1e-6 level (the
suite asserts 1e-5 for a forward pass), so a trajectory whose :a (discrete), :done, :episode_end and :t columns are the same under three independent draws of 1e-5 parameter
noise cannot be flipped by that difference. A case that misses gets other seeds (rollout_res_cases.SEED_OVERRIDES)."""
import numpy as np
import pytest

import rollout_res_cases as RC

ALL = RC.CASES + RC.EVAL_CASES
IDS = [c.name for c in ALL]
RNG_ACTION = 1      # include/crux_rng.h: CRUX_RNG_ACTION


def test_the_table_holds_what_it_must():
    names = [c.name for c in RC.CASES]
    assert len(set(names)) == len(names)
    by = {}
    for c in RC.CASES:
        by.setdefault((c.env, c.head, tuple(c.acts)), set()).add(c.H)
    for key in [(RC.SYNTH, h, tuple(RC.RELU3)) for h in ("eps_greedy", "categorical", "softq", "greedy", "always_stochastic")] + \
               [(RC.PEND, "gaussian", tuple(RC.RELU3)), (RC.PEND, "squashed", tuple(RC.RELU3)), (RC.PEND, "noise", tuple(RC.RELU3)), (RC.PEND, "noise", tuple(RC.TANH_OUT)),
                (RC.PEND, "gaussian", tuple(RC.TANH_HID))]:
        assert by.get(key) == {128, 256}, key
    assert {c.E for c in RC.CASES} == {1, 3}
    seqs = {tuple(t for t, _ in c.calls) for c in RC.CASES}
    assert seqs >= {(2,), (3,), (4, 4, 4), (33,), (1, 3, 1, 4)}
    assert {t for s in seqs for t in s} <= {1, 2, 3, 4, 33}
    for H in (128, 256):
        here = [c for c in RC.CASES if c.H == H]
        assert any("wrap_inside_env0" in c.events for c in here) and any("wrap_between_envs" in c.events for c in here)
        for resets in (False, True):      # max_steps = 5 with and without reset_at_end on the launches that hold the ends
            assert any(c.max_steps == 5 and all(r == resets for _, r in c.calls[1:]) for c in here), (H, resets)
    for env in (RC.SYNTH, RC.PEND):
        here = [c for c in RC.CASES if c.env == env]
        assert any((c.mu, c.sigma) == (0.01, 0.5) for c in here) and any(set(c.extras) >= {"t", "i", "weight", "cost"} for c in here)
        for H in (128, 256):
            assert any(c.seam and c.H == H and "logprob" in c.extras for c in here), (env, H)      # the explore seam: one discrete and one Gaussian case per width
    pr = [c for c in RC.CASES if c.prioritized]
    assert len(pr) == 1 and (pr[0].E, pr[0].env, pr[0].H, [t for t, _ in pr[0].calls]) == (1, RC.SYNTH, 256, [4, 33]) and pr[0].fill >= pr[0].cap
    for c in RC.CASES:
        if c.head in ("eps_greedy", "categorical", "gaussian") and not c.prioritized:      # (the prioritized ring is C3's: no :logprob column, the Float64 log is skipped)
            assert "logprob" in c.extras, c
        assert sum(t for t, _ in c.calls) <= 100      # rollout steps run serially
    for c in RC.EVAL_CASES:
        assert (c.E, c.calls, c.max_steps, c.explore) == (3, [(12, True)], 12, False)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_long_call_takes_the_resident_kernel_and_no_row_is_overwritten(case):
    for T, _ in case.calls:
        assert RC.takes_res(case, T) == (T >= 2), (case, T)
    assert any(T >= 2 for T, _ in case.calls)
    assert case.n_rows <= case.cap
    rows = case.rows()
    assert rows["j"].size == case.n_rows == np.unique(rows["j"]).size and rows["ctr"].max() < 100
    if case.prioritized:
        assert case.fill >= case.cap      # a full ring: the pushes update the tree in place


def _last_of_call(rows):
    return rows["t"] == rows["T"] - 1


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_the_oracles_trajectory_holds_the_events_the_case_is_named_for(case):
    ref = RC.oracle_run(case, extras=sorted(set(case.extras) | {"t"}))
    rows, cols = case.rows(), ref.cols
    j = rows["j"]
    ee, done, tt = cols["episode_end"][0, j], cols["done"][0, j], cols["t"][0, j]
    assert np.isfinite(cols["s"]).all() and np.isfinite(cols["sp"]).all() and np.isfinite(cols["r"]).all()
    by_max = ee & ~done & (tt == case.max_steps)
    if "max_steps_end" in case.events:
        assert by_max.sum() >= 2 * case.E and (by_max & ~_last_of_call(rows)).any(), case      # several ends INSIDE a launch
    if "end_on_last_step" in case.events:
        assert (by_max & _last_of_call(rows)).any(), case
        k = int(np.flatnonzero(by_max & _last_of_call(rows))[0]); c = int(rows["call"][k])
        if case.calls[c][1]:      # under reset_at_end the end on the last step is ONE end: the reset finds the episode already closed
            n_ends = int(ee[rows["call"] == c].sum())
            assert ref.per_call[c][1] == n_ends, (case, ref.per_call[c], n_ends)
    if any(r for _, r in case.calls):
        c = [k for k, (_, r) in enumerate(case.calls) if r][-1]
        assert ee[(rows["call"] == c) & _last_of_call(rows)].all(), case                          # every environment's last row of a reset launch ends an episode
    e0 = rows["e"] == 0
    inside = [c for c in range(len(case.calls)) if (np.diff(j[e0 & (rows["call"] == c)]) < 0).any()]
    if "wrap_inside_env0" in case.events:
        assert inside, case
    if "wrap_between_envs" in case.events:
        assert not inside and any(j[(rows["call"] == c) & (rows["e"] == e) & _last_of_call(rows)][0] == case.cap - 1 and j[(rows["call"] == c) & (rows["e"] == e + 1) & (rows["t"] == 0)][0] == 0
                                  for c in range(len(case.calls)) for e in range(case.E - 1)), case
    z = ref.policy.forward(cols["s"][:, j])
    if case.disc:
        ai = np.argmax(cols["a"][:, j], axis=0); assert (cols["a"][:, j].sum(axis=0) == 1).all()
    if case.head == "eps_greedy":
        s0, s1, n = case.eps
        eps = np.maximum(s1, s0 - rows["gi"] * ((s0 - s1) / n))
        u = np.array([RC.philox_u64(case.env_seed, c, e, RNG_ACTION) for c, e in zip(rows["ctr"], rows["e"])])
        rand = u < eps
        assert rand.any() and (~rand).any() and eps[0] > 0.5 and eps[-1] == s1, (case, eps)      # mostly random at the start, mostly greedy at the end
        assert np.array_equal(ai[~rand], np.argmax(z, axis=0)[~rand])
        if "logprob" in case.extras:
            assert np.allclose(cols["logprob"][0, j], np.log(eps / case.ad + 1.0 - eps), atol=1e-6)
    if case.head in ("categorical", "softq", "always_stochastic") and case.n_rows >= 9:
        assert np.unique(ai).size >= 2, case                                                        # the draws decide, not one dominant logit
    if case.head == "always_stochastic":
        assert np.isnan(cols["logprob"][0, j]).all()
    if case.head in ("greedy", "deterministic"):
        a = cols["a"][:, j]
        assert np.array_equal(ai, np.argmax(z, axis=0)) if case.disc else float(np.abs(a - z).max()) < 1e-6
    if case.head == "noise":
        a = cols["a"][0, j]; lo, hi = np.float32(RC.NOISE["a_min"]), np.float32(RC.NOISE["a_max"])
        at_bound = (a == lo) | (a == hi); n0 = (a - z[0])[~at_bound]
        eps_bound = np.abs(np.abs(n0) - RC.NOISE["eps_max"]) < 1e-5
        assert at_bound.any() and not at_bound.all() and eps_bound.any() and not eps_bound.all(), (case, int(at_bound.sum()), int(eps_bound.sum()))
        assert a.min() >= lo and a.max() <= hi and float(np.abs(n0).max()) < RC.NOISE["eps_max"] + 1e-5
    if case.head == "squashed":
        assert float(np.abs(cols["a"]).max()) <= RC.ASCALE
    if case.head in ("gaussian", "squashed", "categorical", "softq"):
        assert np.isfinite(cols["logprob"][0, j]).all()
    bias = case.params()      # every bias is far from Glorot's zero
    off = 0
    for l in range(3):
        off += case.dims[l] * case.dims[l + 1]; b = bias[off:off + case.dims[l + 1]]; off += case.dims[l + 1]
        assert (b != 0).all(), (case, l)
        if b.size > 4:
            assert float(np.abs(b).mean()) > 0.02, (case, l)
        else:      # the output biases one by one (a condition on the seed): 200 times the bound the GPU module puts on a continuous action, 20 times the one on :logprob
            assert float(np.abs(b).min()) > 0.002, (case, b)
    if case.prioritized:
        pr, mx, mn = ref.priorities
        assert np.unique(pr).size > case.cap - case.n_rows and mx > mn > 0


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_discrete_decisions_survive_parameter_noise_of_1e_5(case):
    extras = sorted(set(case.extras) | {"t"})
    base = RC.oracle_run(case, extras=extras)
    keys = ["done", "episode_end", "t"] + (["a"] if case.disc else [])
    for n in range(3):
        other = RC.oracle_run(case, jitter_seed=7000 + 10 * n + case.H, extras=extras)
        assert not np.array_equal(other.policy.params, base.policy.params)
        for k in keys:
            assert np.array_equal(base.cols[k], other.cols[k]), (case, n, k)
        assert [p[1:] for p in base.per_call] == [p[1:] for p in other.per_call]
        assert np.array_equal(base.state[1], other.state[1]) and np.array_equal(base.state[2], other.state[2])
