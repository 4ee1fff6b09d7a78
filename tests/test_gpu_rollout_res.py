"""The register-resident wide rollout kernel k_rollout_res<H> (csrc/env.hip; H = 128 and 256, the rollouts of the off-policy configurations C3 / C4 and every evaluation episode
of their policies) on the cases of tests/rollout_res_cases.py: every head it serves, tanh hidden and output layers, E = 1 and 3, T = 2, 3, 4 and 33, T = 1 calls (the generic
kernel) alternating with it on one sampler, ring wraps inside and between the environments' rows, episode ends by max_steps inside a launch and on its last step with and
without reset_at_end, whitened observations, the optional columns, a full prioritized ring -- all with NON-ZERO biases (N(0, 0.05) on every parameter).

  a  route identity: the whole call sequence under the default switches and under CRUX_FORCE_GENERIC=1 (k_rollout_wide / k_rollout), bit for bit in every buffer column, the sampler
     state, the per-call sums and next_ind; the prioritized case also in priorities, max / min priority and cumsum() after every call. The kernel's header promises the generic
     kernels' bits; a difference is a bug of k_rollout_res, never a tolerance.
  b  against the oracle, with the bounds of test_rollout_matches_oracle; the measured maxima are printed (ROLLOUT_RES lines; profiles/rollout_res_tests.txt).
  c  crux.policy_explore on the rollout's own :s column and draw counters returns its :a and :logprob columns bit for bit (k_explore_generic<256> against k_rollout_res).
  d  crux.episodes_ with a greedy policy of the resident shapes against orc_first_episode_metrics.
tests/test_rollout_res_cases.py shows on the CPU that every case contains the events it is named for and that its discrete decisions survive 1e-5 parameter noise, so an exact
comparison of :a, :done, :episode_end and :t with the unfused oracle is not a matter of seed luck.

With CRUX_FORCE_GENERIC=1 set for the whole run (a) skips and (b) - (d) pin the generic kernels at these shapes.

Measured on an MI355X (profiles/rollout_res_tests.txt): (a), (c) and (d) hold bit for bit on every case; (b) worst continuous :a 7.2e-07, :s / :sp / :r 1.1e-06, :logprob 4.8e-07,
sampler state 1.6e-07, sum_r 2.9e-08 relative, every exact column exact. No kernel change was needed. Scratch builds with b2 dropped from layer 2, or with eight lanes of layer 3
read twice, fail 57 of the 58 tests each (all of (a), (b) and (c) at both widths; a greedy evaluation at H = 256 keeps its argmax)."""
import os

import numpy as np
import pytest

import crux_jl_amd as crux
import oracle as O
import rollout_res_cases as RC

pytestmark = pytest.mark.gpu
IDS = [c.name for c in RC.CASES]
SEAM = [c for c in RC.CASES if c.seam]
EXACT = ("done", "episode_end", "t", "i")


def _gpu_run(case):
    """the case's call sequence from a fresh policy, sampler and buffer"""
    g = case.gpu_policy(); smp = case.gpu_sampler(g); buf = case.gpu_buffer()
    i, per_call, per = case.i0, [], []
    for T, reset in case.calls:
        info = crux.steps_(smp, buf, Nsteps=case.E * T, explore=case.explore, i=i, reset=reset)
        per_call.append((info["sum_r"], info["n_episode_end"], buf.next_ind)); i += case.E * T
        if case.prioritized:
            pp = buf.priority_params(); per.append((pp["priorities"], np.float32(pp["max_priority"]), np.float32(pp["min_priority"]), buf.cumsum()))
    run = RC.Run({k: buf[k] for k in buf.keys()}, smp.state(), per_call)
    run.per, run.policy, run.n = per, g, len(buf)
    return run


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint64) if x.dtype == np.float64 else x


def _same_bits(a, b):
    a, b = _bits(np.asarray(a)), _bits(np.asarray(b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("case", RC.CASES, ids=IDS)
def test_resident_rollout_has_the_generic_kernels_bits(gpu_ctx, monkeypatch, case):
    if os.environ.get("CRUX_FORCE_GENERIC"):
        pytest.skip("the whole run is on the generic kernels: nothing to compare")
    res = _gpu_run(case)
    monkeypatch.setenv("CRUX_FORCE_GENERIC", "1")
    gen = _gpu_run(case)
    monkeypatch.delenv("CRUX_FORCE_GENERIC")
    assert res.n == gen.n == min(case.cap, case.fill + case.n_rows) and sorted(res.cols) == sorted(gen.cols)
    rows = case.rows()
    for k in res.cols:
        if not _same_bits(res.cols[k], gen.cols[k]):
            bad = np.flatnonzero((_bits(res.cols[k]) != _bits(gen.cols[k])).any(axis=0))
            hit = np.isin(rows["j"], bad)
            raise AssertionError("%s: column :%s differs in %d rows, first ring row %d (call, env, step) = %s: %r vs %r" % (
                case, k, bad.size, bad[0], list(zip(rows["call"][hit], rows["e"][hit], rows["t"][hit]))[:4], res.cols[k][:, bad[0]], gen.cols[k][:, bad[0]]))
    for k, (a, b) in enumerate(zip(res.state, gen.state)):
        assert _same_bits(a, b), "%s: %s differs: %r vs %r" % (case, ("the Float64 state", "ep_len", "n_resets")[k], a, b)
    assert [(np.float64(s).view(np.uint64), n, ni) for s, n, ni in res.per_call] == [(np.float64(s).view(np.uint64), n, ni) for s, n, ni in gen.per_call], (res.per_call, gen.per_call)
    for c, (a, b) in enumerate(zip(res.per, gen.per)):
        for what, x, y in zip(("priorities", "max_priority", "min_priority", "cumsum"), a, b):
            assert _same_bits(x, y), "%s: %s differs after call %d at %s" % (case, what, c, np.flatnonzero(_bits(np.atleast_1d(x)) != _bits(np.atleast_1d(y)))[:8])
    assert len(res.per) == (len(case.calls) if case.prioritized else 0)


def _against_oracle(case, run, ref, say):
    """the bounds of test_rollout_matches_oracle on every column, the sampler state and the per-call sums; returns the measured maxima"""
    assert sorted(run.cols) == sorted(ref.cols), (sorted(run.cols), sorted(ref.cols))
    worst = {}
    for k in run.cols:
        a, b = run.cols[k], ref.cols[k]
        assert a.shape == b.shape, (case, k)
        if a.dtype == np.float32:
            assert np.array_equal(np.isnan(a), np.isnan(b)), (case, k, "NaN pattern")
            worst[k] = float(np.abs(np.nan_to_num(a) - np.nan_to_num(b)).max())
        else:
            worst[k] = int((a != b).sum())
    worst["state"] = float(np.abs(run.state[0] - ref.state[0]).max())
    worst["sum_r"] = max(abs(g[0] - o[0]) / max(1.0, abs(o[0])) for g, o in zip(run.per_call, ref.per_call))
    say("ROLLOUT_RES %s: %s" % (case, " ".join("%s %.3g" % (k, worst[k]) for k in sorted(worst))))
    for k in worst:
        if k in EXACT or (k == "a" and case.disc):
            assert worst[k] == 0, (case, k, worst)
        elif k == "a":
            assert worst[k] < 1e-5, (case, k, worst)
        elif k in ("s", "sp", "r", "logprob", "weight", "cost"):
            assert worst[k] < 1e-4, (case, k, worst)
    assert worst["state"] < 1e-6 and np.array_equal(run.state[1], ref.state[1]) and np.array_equal(run.state[2], ref.state[2]), (case, worst, run.state, ref.state)
    assert worst["sum_r"] < 1e-5 and [p[1:] for p in run.per_call] == [p[1:] for p in ref.per_call], (case, run.per_call, ref.per_call)
    return worst


@pytest.mark.parametrize("case", RC.CASES, ids=IDS)
def test_resident_rollout_matches_the_oracle(gpu_ctx, case):
    run, ref = _gpu_run(case), RC.oracle_reference(case)
    _against_oracle(case, run, ref, print)
    if case.prioritized:      # push!: the new rows carry (max_priority + eps)^alpha (experience_buffer.jl:254); the pow of the device and of libm may differ in the last bit
        pr, mx, mn = ref.priorities
        gp, gmx, gmn, _ = run.per[-1]
        assert float(np.abs(gp - pr).max()) <= 4e-7 * float(pr.max()) and abs(gmx - mx) <= 4e-7 * mx and abs(gmn - mn) <= 4e-7 * mx


@pytest.mark.parametrize("case", SEAM, ids=[c.name for c in SEAM])
def test_policy_explore_reproduces_the_resident_rollouts_action_and_logprob_columns(gpu_ctx, case):
    """the seam the caller-stepped environments rest on (test_gpu_host_env.py has it for the 64-wide table): crux_policy_explore promises the bits of the rollout kernel that
    serves the policy shape -- for these shapes k_explore_generic<256> on one side and k_rollout_res on the other"""
    run, rows = _gpu_run(case), case.rows()
    S, A, LP = run.cols["s"], run.cols["a"], run.cols["logprob"]
    assert np.isfinite(LP[0, rows["j"]]).all()
    for c in range(len(case.calls)):
        for t in range(case.calls[c][0]):
            sel = np.flatnonzero((rows["call"] == c) & (rows["t"] == t))
            assert np.array_equal(rows["e"][sel], np.arange(case.E))
            j = rows["j"][sel]
            a, lp = crux.policy_explore(run.policy, case.cfg(False, rows["gi"][sel[0]]), S[:, j], case.env_seed, rows["ctr"][sel])
            assert _same_bits(a, A[:, j]), "%s call %d step %d: actions differ: %r vs %r" % (case, c, t, a, A[:, j])
            assert _same_bits(lp, LP[0, j]), "%s call %d step %d: logprob differs: %r vs %r" % (case, c, t, lp, LP[0, j])


@pytest.mark.parametrize("case", RC.EVAL_CASES, ids=[c.name for c in RC.EVAL_CASES])
def test_batched_evaluation_of_a_resident_shape_matches_the_oracle(gpu_ctx, case):
    """episodes! (src/sampler.jl:175-200) as crux.episodes_ launches it: E = Neps fresh environments, T = max_steps, reset at the end -- one k_rollout_res launch"""
    Neps, T, seed = case.E, case.max_steps, case.env_seed + 0x45564C
    g = case.gpu_policy()
    data, m = crux.episodes_(case.gpu_sampler(g, n_envs=1), Neps=Neps)
    o, ob = case.oracle_policy(), case.oracle_buffer()
    oe = O.OEnv(case.env, Neps, T, 0.99, seed, so=case.od, sa=case.ad)
    sr, ne = oe.rollout(o, case.cfg(True, 0), ob, T)
    und, dis, ln, ok = np.empty(Neps, np.float32), np.empty(Neps, np.float32), np.empty(Neps, np.int64), np.empty(Neps, np.uint8)
    O.chk(O.lib().orc_first_episode_metrics(ob.h, Neps, T, np.float32(0.99), O.vpz(und), O.vpz(dis), O.vpz(ln), O.vpz(ok)))
    print("ROLLOUT_RES %s: undiscounted %.3g discounted %.3g" % (case, float(np.abs(m["undiscounted"] - und).max()), float(np.abs(m["discounted"] - dis).max())))
    assert np.array_equal(m["length"], ln) and np.array_equal(m["complete"], ok.astype(bool)) and ok.all() and (ln == T).all()
    assert np.abs(m["undiscounted"] - und).max() < 1e-4 * max(1, np.abs(und).max()) and np.abs(m["discounted"] - dis).max() < 1e-4 * max(1, np.abs(dis).max())
    for k in ("a", "done", "episode_end"):
        assert np.array_equal(data[k], ob[k]) if case.disc or k != "a" else float(np.abs(data[k] - ob[k]).max()) < 1e-5, (case, k)
    for k in ("s", "sp", "r"):
        assert float(np.abs(data[k] - ob[k]).max()) < 1e-4, (case, k)
