"""No GPU: known answers for the float64 yardstick of NDA-GAIL-JS (tests/nda_gail_reference.py), so that what tests/test_gpu_nda_gail.py compares the device against is
itself pinned. At ar = 1/2 the reward is r = (logsigmoid(z) - logsigmoid(z) + z) / 2 = z / 2 whatever z is, and with Dnda = D the hinge max(0, r - r) vanishes."""
import numpy as np
import torch

import nda_gail_reference as R

DIMS, ACTS = [5, 16, 16, 1], ["relu", "tanh", "identity"]


def _params(seed, dims=DIMS):
    rng = np.random.default_rng(seed); p = []
    for i, o in zip(dims[:-1], dims[1:]):
        p += [rng.normal(0, 0.5, i * o), rng.normal(0, 0.1, o)]
    return np.concatenate(p)


def _data(seed, n, od=3, ad=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (ad, n)), rng.normal(0, 1, (od, n))


def test_reward_is_half_the_output_at_alpha_one_half():
    z = np.concatenate([np.linspace(-30, 30, 61), [-745.0, 1e-9, 700.0]])
    assert np.array_equal(R.reward(z, 0.5), 0.5 * R.logsigmoid(z) - 0.5 * (R.logsigmoid(z) - z))
    assert np.abs(R.reward(z, 0.5) - z / 2).max() <= 1e-13 * np.abs(z).max()
    # away from one half the two logs weigh in: r -> ar z for z -> -inf, r -> (1 - ar) z for z -> +inf
    ar = float(np.float32(0.3))      # the Float32 the reference holds
    assert abs(R.reward(-40.0, 0.3) - ar * -40.0) < 1e-12 and abs(R.reward(40.0, 0.3) - (1 - ar) * 40.0) < 1e-12


def test_hinge_is_zero_when_dnda_is_d_and_one_sided_otherwise():
    a, s = _data(1, 50); p = _params(2)
    z = R.d_out(p, DIMS, ACTS, a, s)
    for ar in (0.5, 0.3):
        r = R.reward(z, ar)
        assert np.array_equal(R.hinge_cost(r, r), np.zeros(50))
        zn = R.d_out(_params(3), DIMS, ACTS, a, s); rn = R.reward(zn, ar); c = R.hinge_cost(r, rn)
        assert np.array_equal(c > 0, rn > r) and np.allclose(c[c > 0], (rn - r)[c > 0], rtol=0, atol=0) and 0 < (c > 0).sum() < 50
    assert np.allclose(R.hinge_cost(R.reward(z, 0.5), R.reward(zn, 0.5)), np.maximum(0, (zn - z) / 2), rtol=0, atol=1e-13)


def test_loss_value_and_gradient_against_finite_differences():
    (ae, se), (ap, sp) = _data(4, 13), _data(5, 9); p = _params(6)
    loss, g = R.d_step(p, DIMS, ACTS, ae, se, ap, sp)
    ze, zp = R.d_out(p, DIMS, ACTS, ae, se), R.d_out(p, DIMS, ACTS, ap, sp)
    assert abs(loss - (np.mean(np.logaddexp(0, -ze)) + np.mean(np.logaddexp(0, zp)))) < 1e-12      # -log sigmoid(z_E) and -log(1 - sigmoid(z_pi))
    f = lambda q: R.gail_d_loss(R.mlp_params(q, DIMS), ACTS, ae, se, ap, sp).item()
    rng = np.random.default_rng(7); h = 1e-6
    for i in rng.choice(p.size, 40, replace=False):
        e = np.zeros(p.size); e[i] = h
        fd = (f(p + e) - f(p - e)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (i, fd, g[i])      # relu kinks are measure zero for these draws
    assert np.abs(g).max() > 1e-3


def test_partition_plan_on_hand_written_cases():
    P = R.partition_plan
    # expert shorter: 5 rows against 9 at batch 4 -> two pairs, the second ragged on the expert side only
    assert P(5, 9, 4, 1) == [(0, 0, 4, 0, 4), (0, 4, 1, 4, 4)]
    # policy shorter
    assert P(9, 5, 4, 1) == [(0, 0, 4, 0, 4), (0, 4, 4, 4, 1)]
    # equal lengths, a multiple of the batch: no ragged pair
    assert P(8, 8, 4, 2) == [(0, 0, 4, 0, 4), (0, 4, 4, 4, 4), (1, 0, 4, 0, 4), (1, 4, 4, 4, 4)]
    # ragged on both sides in the last pair
    assert P(6, 7, 4, 1) == [(0, 0, 4, 0, 4), (0, 4, 2, 4, 3)]
    # the shapes of the device tests: 3 B + 9 against 2 B + 5 -> three pairs, the last (B, 5)
    assert [(ne, np_) for _e, _oe, ne, _op, np_ in P(3 * 64 + 9, 2 * 64 + 5, 64, 1)] == [(64, 64), (64, 64), (64, 5)]
    # max_batches cutting mid-epoch: 3 pairs per epoch, 5 steps -> the second epoch ends after its second pair
    plan = P(12, 12, 4, 3, max_batches=5)
    assert [(e, oe) for e, oe, *_ in plan] == [(0, 0), (0, 4), (0, 8), (1, 0), (1, 4)]
    assert len(P(12, 12, 4, 3, max_batches=6)) == 6 and len(P(12, 12, 4, 3)) == 9
    # a batch wider than both buffers: one pair of everything
    assert P(3, 5, 128, 2) == [(0, 0, 3, 0, 5), (1, 0, 3, 0, 5)]


def test_gae_returns_and_whiten_known_answers():
    ee = np.array([0, 0, 1, 0, 1, 0, 0], bool)
    assert R.episodes(ee) == [(0, 2), (3, 4), (5, 6)] and R.episodes(np.zeros(3, bool)) == [(0, 2)]
    r = np.arange(1.0, 8.0); done = np.array([0, 0, 1, 0, 0, 0, 0], float); z = np.zeros(7)
    adv, ret = R.gae_returns(r, done, ee, z, z, 1.0, 0.5)
    assert np.array_equal(ret, [1 + 0.5 * (2 + 0.5 * 3), 2 + 0.5 * 3, 3, 4 + 0.5 * 5, 5, 6 + 0.5 * 7, 7]) and np.array_equal(adv, ret)      # lambda = 1, V = 0: A is the return
    Vs, Vsp = np.full(7, 2.0), np.full(7, 4.0)
    adv0, _ = R.gae_returns(r, done, ee, Vs, Vsp, 0.0, 0.5)
    assert np.array_equal(adv0, r + (1 - done) * 0.5 * 4.0 - 2.0)                                                                             # lambda = 0: the one-step TD error
    w = R.whiten(np.array([1.0, 2.0, 3.0, 6.0]))
    assert abs(w.mean()) < 1e-15 and abs(w.std(ddof=1) - 1) < 1e-15 and abs(w[3] - 3.0 / np.sqrt(14.0 / 3.0)) < 1e-15
