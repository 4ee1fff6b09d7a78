"""Host-only checks of tests/offgail_reference.py, the float64 yardstick of tests/test_gpu_offgail.py: the closed-form seed of the labelled cross-entropy against
autograd, the label layout, the derived bound of the reward, the draw restatement against the scalar Philox of tests/cql_reference.py, and AdRIL's callback
(src/model_free/il/AdRIL.jl:39-50) in the reference's callback-then-push order, worked by hand.
"""
import numpy as np
import pytest
import torch

import cql_reference as CR
import offgail_reference as R


def _net(dims, seed):
    rng = np.random.default_rng(seed); flat = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o)); flat += [rng.uniform(-lim, lim, i * o), np.zeros(o)]
    return np.concatenate(flat)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_seed_is_softmax_minus_onehot_over_n(K, act):
    Bd, dims = 9, [5, 16, K]; acts = [act, "identity"]
    X = np.random.default_rng(K).normal(0, 1, (5, K * Bd))
    layers = R.mlp_params(_net(dims, 1), dims)
    x = torch.as_tensor(X)
    z = R.mlp(layers, acts, x); z.retain_grad()
    lab = torch.as_tensor(R.labels(K, Bd))
    loss = (torch.logsumexp(z, 0) - z[lab, torch.arange(K * Bd)]).mean()
    loss.backward()
    assert np.abs(z.grad.numpy() - R.ce_seed(z.detach().numpy(), K, Bd)).max() < 1e-15
    assert abs(float(loss.detach()) - float(R.ce_loss(R.mlp_params(_net(dims, 1), dims), acts, X, K, Bd).detach())) < 1e-15
    assert abs(float(loss.detach()) - float(torch.nn.functional.cross_entropy(z.detach().T, lab))) < 1e-12


@pytest.mark.parametrize("K", [2, 3, 4])
def test_label_layout(K):
    """hcat(demo, policy, ndas...): column j belongs to source j // Bd; a head that is certain of that layout has loss ~ 0, any other layout does not"""
    Bd = 7; lab = R.labels(K, Bd)
    assert lab.tolist() == [k for k in range(K) for _ in range(Bd)]
    z = np.full((K, K * Bd), -30.0); z[lab, np.arange(K * Bd)] = 30.0
    lse = np.log(np.exp(z).sum(0))
    assert np.abs(lse - z[lab, np.arange(K * Bd)]).max() < 1e-12
    assert np.abs(R.ce_seed(z, K, Bd)).max() < 1e-12
    assert np.abs(R.ce_seed(np.roll(z, Bd, axis=1), K, Bd)).max() > 0.5 / (K * Bd)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_reward_bounds_and_weights(K):
    """every term lies in +-(log(1 + 1e-5) - log(1e-5)) = +-11.5129, so |r| <= 11.5129 sum|w|"""
    assert abs(R.TERM_BOUND - 11.5129) < 1e-4
    w = R.weights(K)
    assert w[0] == 1 and w[1] == 0 and np.allclose(w[2:], -1.0 / max(K - 2, 1)) and len(w) == K
    rng = np.random.default_rng(K)
    for spread in (1.0, 6.0, 40.0, 200.0):
        z = rng.normal(0, spread, (K, 500))
        for dt in (np.float64, np.float32):
            r = R.reward(z, dt)
            assert np.all(np.isfinite(r)) and np.abs(r).max() <= R.TERM_BOUND * np.abs(w).sum() * (1 + 1e-6)
    # a column the discriminator is sure is a demonstration earns the upper bound; one it is sure is the policy's earns the lower
    z = np.full((K, 2), -100.0); z[0, 0] = 100.0; z[1, 1] = 100.0
    r = R.reward(z)
    assert r[0] > 11.5 and r[1] < -11.5 + (11.6 if K > 2 else 0)


def test_draws_restate_uniform_sample():
    seed, Bd, n = 0x5EED5A3F, 50, 37
    for stream, counter in ((16, 0), (17, 3), (18, 12345678901)):
        ids = R.sample_ids(seed, stream, counter, Bd, n)
        assert ids.min() >= 0 and ids.max() < n
        for j in (0, 1, Bd - 1):
            x = CR.philox(seed, counter * Bd + j, [stream], R.RNG_SAMPLE)
            assert ids[j] == (int(x[0, 0]) * n) >> 32
    # a source shorter than the batch is sampled with replacement over its length
    assert len(set(R.sample_ids(seed, 16, 1, 128, 5).tolist())) <= 5


def test_adril_five_iterations_by_hand():
    """dN = 50, buffer_init = 0: iteration t pushes rows i = 50 (t - 1) + 1 .. 50 t; before its push the old rows are paid -, -1, -1/2, -1/3, -1/4"""
    ring, dN = R.HostRing(1000), 50
    want_old = [None, -1.0, -0.5, np.float32(-1.0 / 3.0), -0.25]
    for t in range(5):
        R.adril_steps(ring, np.arange(50 * t + 1, 50 * t + 51), 0, dN)
        n = len(ring); assert n == 50 * (t + 1)
        assert np.all(ring.r[n - 50:n] == 0)
        if t == 0:
            continue
        assert np.all(ring.r[:n - 50] == np.float32(want_old[t])), (t, np.unique(ring.r[:n - 50]))


def test_adril_wrapping_ring_keeps_new_rows_at_zero():
    ring, dN = R.HostRing(120), 50
    for t in range(5):
        R.adril_steps(ring, np.arange(50 * t + 1, 50 * t + 51), 0, dN)
    assert len(ring) == 120 and ring.next_ind == 250 % 120
    mx = ring.i.max(); assert mx == 250
    fresh = ring.i > mx - dN
    assert fresh.sum() == 50 and np.all(ring.r[fresh] == 0) and np.all(ring.r[~fresh] == np.float32(-0.25))


def test_adril_non_divisible_raises_and_leaves_the_ring():
    ring = R.HostRing(100)
    R.adril_steps(ring, np.arange(1, 51), 0, 50)
    i0, r0 = ring.i.copy(), ring.r.copy()
    with pytest.raises(ValueError, match="InexactError"):
        R.adril_steps(ring, np.arange(51, 78), 0, 50)                # max_i = 77
    assert np.array_equal(ring.i, i0) and np.array_equal(ring.r, r0) and len(ring) == 50


def test_adril_k_zero_gives_minus_infinity():
    """max_i - buffer_init == dN: k = 0, -1/k = -Inf on every old row (reachable with buffer_init > 0)"""
    ring = R.HostRing(100)
    R.adril_steps(ring, np.arange(101, 121), 100, 50)               # empty buffer: only the zeroing
    assert np.all(ring.r[:20] == 0)
    R.adril_steps(ring, np.arange(121, 151), 100, 50)               # max_i = 150: k = 0; old rows i <= 100: none
    assert np.all(ring.r[:50] == 0)
    ring.i[:5] = 100                                                # rows old enough
    R.adril_steps(ring, np.arange(141, 151), 100, 50)
    assert np.all(np.isneginf(ring.r[:5])) and np.all(ring.r[5:60] == 0)
