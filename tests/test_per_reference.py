"""CPU checks of the prioritized-replay yardstick (tests/per_reference.py): its search and weights against the oracle's prioritized_sample! on the N grid of
tests/test_gpu_per_tree.py, with injected and with Philox draws, and proof that the injected draws reach the clamp past the last element and the first element."""
import numpy as np
import pytest

import oracle as O
import per_reference as R

N_GRID = [2, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097, 65_536, 100_003, 1_000_000]
B_GRID = [1, 3, 5, 128, 1000]
SEED = 0x5EED5A3F


def _filled(N, seed):
    """a full ring of N rows whose priorities went through push!, a Float64 update of every row and a Float32 update of a few"""
    rng = np.random.default_rng(seed); m = R.Model(N)
    m.push(N)
    m.update(np.arange(N), np.abs(rng.standard_normal(N)) + 1e-3)
    k = min(N, 50); m.update(rng.choice(N, k, replace=False), (np.abs(rng.standard_normal(k)) + 1e-3).astype(np.float32))
    return m, rng


def _check(m, B, rands, i):
    """search / weights against orc_per_sample; returns (clamped strata, first-element hits)"""
    N = m.elements; pr = m.priorities[:N]; c = R.pairwise_cumsum(pr)
    ids_o, w_o = m.sample(B, rands, 0.5, i, SEED)
    u = rands if rands is not None else R.sample_rands(SEED, i, B)
    raw = R.search(c, B, u, clamp=False); ids = np.minimum(raw, N - 1)
    assert np.array_equal(ids, R.search(c, B, u)) and np.array_equal(ids, ids_o), (N, B)
    w = R.weights(pr, ids, c[N - 1], m.min_priority, N, 0.5)
    assert np.abs(w - w_o[ids]).max() <= 4e-7 * max(1.0, w.max()), (N, B)
    return int((raw >= N).sum()), int((ids == 0).sum())


def test_philox_draws_are_the_oracles():
    for ctr in (0, 1, 7 * 1000 + 999, 2 ** 40 + 3):
        out = np.zeros(4, np.uint32); O.lib().orc_philox(SEED, ctr, 0, R.RNG_SAMPLE, O.vpz(out))
        assert np.array_equal(R.philox(SEED, [ctr], 0, R.RNG_SAMPLE)[:, 0], out)
    u = R.sample_rands(SEED, 3, 1000)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.05


def test_leaves_tile_the_vector_and_sit_on_at_most_two_levels():
    two_level = []
    for N in N_GRID + [3_000_001]:
        lv = R.leaves(N)
        assert lv[0][0] == 1 and lv[-1][0] + lv[-1][1] == N and all(a[0] + a[1] == b[0] for a, b in zip(lv, lv[1:]))
        assert all(1 <= n < 128 for _, n, _ in lv) and len({l for _, _, l in lv}) <= 2
        if len({l for _, _, l in lv}) == 2:
            two_level.append(N)
        for e in {1, N - 1, lv[len(lv) // 2][0]}:
            k, i1, n, lvl, heap = R.locate(N, e)
            assert lv[k] == (i1, n, lvl) and i1 <= e < i1 + n and heap >> lvl == 1
    assert 4096 in two_level and 256 in two_level and 1_000_000 not in two_level


@pytest.mark.parametrize("N", N_GRID)
def test_search_and_weights_reproduce_the_oracle(N):
    m, rng = _filled(N, N); clamped = first = 0
    Bc = R.clamp_B(R.pairwise_cumsum(m.priorities[:N])[N - 1])      # (chosen from the reference alone)
    for B in B_GRID + [Bc]:
        r = R.injected_rands(B, rng)
        for i, rands in enumerate([r, None, R.injected_rands(B, rng, flip=True)]):
            c_, f_ = _check(m, B, rands, i + 1); clamped += c_; first += f_
    assert first >= 1 and clamped >= 1, (first, clamped)       # u = 0 in stratum 1 lands on element 1; u = 1 - 2^-53 in the last stratum passes the total at B = Bc


def test_a_locally_non_monotone_cumsum_is_searched_by_probe_sequence():
    """large prefix + tiny leaf sums: c[i] = s + s_ rounds differently across a leaf boundary; np.searchsorted is not a valid restatement there"""
    N = 4096; m = R.Model(N); m.push(N); rng = np.random.default_rng(9)
    v = np.full(N, 1e-7); v[:200] = 3e4 * (1 + rng.random(200))
    m.update(np.arange(N), v)
    for B in (128, 1000):
        _check(m, B, rng.random(B), 5)
