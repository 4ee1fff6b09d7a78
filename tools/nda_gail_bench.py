"""NDA-GAIL's GAIL_callback: the round (crux_nda_gail_round, one host synchronisation) against the composition of the entries that existed before it -- the host loop of
crux_buffer_shuffle + crux_gail_d_step for both discriminators, crux_gail_reward for both, the hinge on the host, and the six advantage calls. Both at the shape of
examples/nda_gail_pendulum.py and at the HalfCheetah shape (17 obs / 6 act, discriminators 23-256-256-1). Warm-up, then timed repeats between two stream
synchronisations (tools/per_bench.py). Writes profiles/nda_gail_bench.txt."""
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import crux_jl_amd as crux
from crux_jl_amd import _lib as L

ctx = crux.default_context()
EXTRAS = ["return", "advantage", "logprob", "cost", "cost_advantage", "cost_return"]
LAM, GAMMA, AR = 0.95, 0.99, 0.5


def chain(dims):
    return crux.Chain(*[crux.Dense(i, o, "relu" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))])


def rows(rng, od, ad, n, T):
    ee = np.zeros((1, n), bool); ee[0, T - 1::T] = True
    return {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": ee.copy(), "episode_end": ee}


def buf(od, ad, d, extras=()):
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), d["s"].shape[1], list(extras)); b.push_(d); return b


def timed(fn, warm=3, n=20):
    for _ in range(warm):
        fn()
    ctx.sync(); t0 = time.perf_counter()
    for _ in range(n):
        fn()
    ctx.sync(); return (time.perf_counter() - t0) / n * 1e3


def bench(name, od, ad, hidden, n_demo, dN, T, B, epochs):
    rng = np.random.default_rng(0); vp = lambda a: a.ctypes.data_as(L.vp)
    mk = lambda dims, seed: crux.ContinuousNetwork(chain(dims), seed=seed)
    D, N = mk([od + ad] + hidden + [1], 3), mk([od + ad] + hidden + [1], 4); V, Vc = mk([od, 64, 64, 1], 2), mk([od, 64, 64, 1], 5)
    for q in (D, N):
        q.attach_optimizer(crux.Adam(np.float32(3e-4)))
    demo, nda = buf(od, ad, rows(rng, od, ad, n_demo, T)), buf(od, ad, rows(rng, od, ad, n_demo, T))
    bd = rows(rng, od, ad, dN, T); batch, cD, cN = buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS)
    k = [0]; rD, rN, o3, m = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32), np.zeros(1, np.float32)
    lib = ctx.lib

    def round_():
        ctx.check(lib.crux_nda_gail_round(D.h, N.h, demo.h, nda.h, batch.h, cD.h, cN.h, V.h, Vc.h, B, epochs, 0, 11, k[0], B, epochs, 0, 12, k[0], AR, LAM, GAMMA, vp(rD), vp(rN), vp(o3)))
        k[0] += epochs

    def parts():      # the entries of the parent commit
        for net, ex, seed in ((D, demo, 11), (N, nda, 12)):
            pol = crux.copy_buffer(batch)
            nb = min(-(-len(ex) // B), -(-len(pol) // B))
            for e in range(epochs):
                crux.shuffle_device_(ex, seed, 2 * (k[0] + e)); crux.shuffle_device_(pol, seed, 2 * (k[0] + e) + 1)
                for q in range(nb):
                    ctx.check(lib.crux_gail_d_step(net.h, ex.h, q * B, min(B, len(ex) - q * B), pol.h, q * B, min(B, len(pol) - q * B), vp(rD)))
        k[0] += epochs
        ctx.check(lib.crux_gail_reward(N.h, batch.h, AR, 1.0, vp(m))); rn = batch["r"]
        ctx.check(lib.crux_gail_reward(D.h, batch.h, AR, 1.0, vp(m))); batch["cost"] = np.maximum(0, rn - batch["r"])
        ctx.check(lib.crux_fill_gae(batch.h, V.h, LAM, GAMMA)); ctx.check(lib.crux_fill_returns(batch.h, GAMMA))
        ctx.check(lib.crux_fill_gae_keys(batch.h, Vc.h, LAM, GAMMA, L.COL["cost"], L.COL["cost_advantage"])); ctx.check(lib.crux_fill_returns_keys(batch.h, GAMMA, L.COL["cost"], L.COL["cost_return"]))
        ctx.check(lib.crux_whiten(batch.h, L.COL["advantage"])); ctx.check(lib.crux_whiten(batch.h, L.COL["cost_advantage"]))
    tp, tr = timed(parts), timed(round_)
    steps = 2 * epochs * min(-(-n_demo // B), -(-dN // B))
    return "%-12s %d obs / %d act, D %s, %d demo rows, dN %d, batch %d, %d epochs (%d discriminator steps): parts %.3f ms  round %.3f ms  ratio %.2f" % (
        name, od, ad, "-".join(map(str, [od + ad] + hidden + [1])), n_demo, dN, B, epochs, steps, tp, tr, tp / tr)


if __name__ == "__main__":
    lines = [bench("pendulum", 3, 1, [64, 64], 512, 1024, 16, 256, 4), bench("halfcheetah", 17, 6, [256, 256], 4096, 4096, 1000, 256, 4)]
    out = "\n".join(["NDA-GAIL GAIL_callback per iteration: the composition of the earlier entries (parts) against crux_nda_gail_round (round); mean of 20 after 3 warm-up calls"] + lines)
    print(out)
    os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
    with open(os.path.join(R, "profiles", "nda_gail_bench.txt"), "w") as f:
        f.write(out + "\n")
