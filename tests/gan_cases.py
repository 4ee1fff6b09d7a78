"""The fixed inputs of tests/test_gpu_gan_losses.py, from numpy alone, so that tests/test_gan_reference.py can assert on the yardstick (tests/gan_reference.py) the
conditions the GPU tests rely on, without a device.

A case: a discriminator (ad + od)-16-16-1 with relu or tanh hidden layers and pools of 300 expert and 300 policy rows; a step of (n_ex, n_pi) reads the first n_ex and
n_pi rows of the pools. The last layer is rescaled and its bias moved so that D's output over both pools has mean 0 and standard deviation 2 (it spans about +-3 and
beyond) with the expert pool's mean above the policy pool's: both sides of the hinge's kinks z = 1 (expert) and z = -1 (policy) are then populated.
"""
import numpy as np

import sn_reference as SR

POOL = 300
SIZES = [(1, 1), (3, 300), (255, 257), (256, 256), (300, 3)]      # the split inside the first trip of the head's 256-stride loop, inside the second, on the boundary
WGP_SIZES = [1, 255, 257]
HEAD_KINDS = ["LS", "Hinge", "W"]
# name: (od, ad, discrete action, hidden activation, rng seed)
# the seeds were fixed through the yardstick alone (tests/test_gan_reference.py asserts what they were chosen for: no column on a kink, both sides of each kink
# populated, few entries under the exclusion rule, and no exactly-zero gradient entry that is a cancellation between columns rather than a dead unit -- under the
# Wasserstein kinds a relu unit that is on in every column of a step is one, which is why suitable seeds are rare: about one in a hundred for the relu cases)
CASES = {"cont-relu": (3, 2, False, "relu", 61), "cont-tanh": (3, 2, False, "tanh", 11), "disc-relu": (4, 2, True, "relu", 197)}
LAM, GP_SEED, GP_COUNTER = 10.0, 0x6A11, 3
EXCLUDE = 1e-3      # entries whose float64 gradient is non-zero but within this share of the gradient's scale of zero are not compared after the Adam step


def rows(rng, od, ad, n, disc, shift=0.0):
    a = np.eye(ad, dtype=bool)[:, rng.integers(0, ad, n)] if disc else rng.uniform(-1, 1, (ad, n)).astype(np.float32)
    return {"s": (rng.normal(0, 1, (od, n)) + shift).astype(np.float32), "a": a, "sp": (rng.normal(0, 1, (od, n)) + shift).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool)}


def x_of(r, n=None):
    """vcat(a, s) of the first n rows, float32 (one-hot actions as 0/1)"""
    n = r["s"].shape[1] if n is None else n
    return np.vstack([r["a"][:, :n].astype(np.float32), r["s"][:, :n]])


def case(name, seed=None):
    od, ad, disc, act, seed0 = CASES[name]; seed = seed0 if seed is None else seed
    rng = np.random.default_rng(seed)
    dims, acts = (ad + od, 16, 16, 1), (act, act, "identity")
    p = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o)); p += [rng.uniform(-lim, lim, i * o), rng.normal(0, 0.3, o)]      # biases of both signs: few relu units are on in every column
    ex, pi = rows(rng, od, ad, POOL, disc, 0.5), rows(rng, od, ad, POOL, disc)
    Ws, bs = SR.unflatten(np.concatenate(p), dims)
    z, _ = SR.forward(SR.flatten(Ws, bs), dims, acts, (0, 0, 0), [], np.concatenate([x_of(ex), x_of(pi)], 1))
    k = (2.0 if z[0, :POOL].mean() >= z[0, POOL:].mean() else -2.0) / z.std(); Ws[-1] = Ws[-1] * k; bs[-1] = (bs[-1] - z.mean()) * k      # the expert pool on the upper side
    return {"name": name, "od": od, "ad": ad, "disc": disc, "dims": dims, "acts": acts, "p": SR.flatten(Ws, bs).astype(np.float32), "ex": ex, "pi": pi}


def skipped(g):
    """the mask of the exclusion rule and its share"""
    g = np.asarray(g, np.float64); m = (g != 0) & (np.abs(g) <= EXCLUDE * np.abs(g).max())
    return m, float(m.mean())
