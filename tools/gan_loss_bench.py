"""The discriminator losses of the GAIL family (src/extras/gans.jl): what a step and a round cost per loss kind.

  step   us per crux_gail_d_step_gan for BCE, LS, hinge, W and WGP at D 4-64-64-1 (Pendulum) and 23-256-256-1 (HalfCheetah) with 256 + 256 columns, and
         crux_advil_d_step over 256 rows (the same 768 columns as the WGP step, plus the actor's forward pass) beside it
  round  ms per crux_nda_gail_round_gan with the hinge against crux_nda_gail_round (BCE) at the shape of examples/nda_gail_pendulum.py

Expected, to confirm or refute: LS, hinge and W cost what BCE costs (the same launches, only the head differs); a WGP step is of the order of crux_advil_d_step.
Every step ends in its own host synchronisation, so a host clock around a window of calls times them. The kinds alternate window by window inside one process
(ROUNDS rounds of one window per kind, after a warm-up window of every kind), so drift of a shared host lands on all of them; reported: the median window and the
spread (min .. max) over the rounds. Writes profiles/gan_loss_bench.txt."""
import os
import sys
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import crux_jl_amd as crux
from crux_jl_amd import _lib as L

ctx = crux.default_context()
EXTRAS = ["return", "advantage", "logprob", "cost", "cost_advantage", "cost_return"]
KINDS = {"BCE": 0, "LS": 1, "Hinge": 2, "W": 3, "WGP": 4}
ROUNDS = 7
vp = lambda a: a.ctypes.data_as(L.vp)


def chain(dims):
    return crux.Chain(*[crux.Dense(i, o, "relu" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))])


def rows(rng, od, ad, n, T=16):
    ee = np.zeros((1, n), bool); ee[0, T - 1::T] = True
    return {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": ee.copy(), "episode_end": ee}


def buf(od, ad, d, extras=()):
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), d["s"].shape[1], list(extras)); b.push_(d); return b


def alternate(fns, calls):
    """{name: (median, min, max)} of the per-call time in seconds: a warm-up window of every fn, then ROUNDS rounds of one window of `calls` calls per fn"""
    t = {k: [] for k in fns}
    for r in range(ROUNDS + 1):
        for k, fn in fns.items():
            ctx.sync(); t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            ctx.sync(); dt = (time.perf_counter() - t0) / calls
            if r:
                t[k].append(dt)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def step_bench(od, ad, hidden, B=256, calls=400):
    rng = np.random.default_rng(0); sd = od + ad; dims = [sd] + hidden + [1]
    ex, pi = buf(od, ad, rows(rng, od, ad, B)), buf(od, ad, rows(rng, od, ad, B))
    nets = {}
    for k in list(KINDS) + ["AdVIL"]:      # a handle per kind: every kind trains from the same start and keeps its own Adam state
        nets[k] = crux.ContinuousNetwork(chain(dims), seed=3); nets[k].attach_optimizer(crux.Adam(np.float32(1e-5)))
    actor = crux.ContinuousNetwork(chain([od, 64, 64, ad]), seed=4)
    info, adv, ctr = np.zeros(L.INFO_N, np.float32), np.zeros(4, np.float32), [0]

    def mk(k):
        def f():
            ctx.check(ctx.lib.crux_gail_d_step_gan(nets[k].h, ex.h, 0, B, pi.h, 0, B, KINDS[k], 10.0, 5, ctr[0], vp(info))); ctr[0] += 1
        return f

    def advil():
        ctx.check(ctx.lib.crux_advil_d_step(actor.h, nets["AdVIL"].h, ex.h, 10.0, 1.0, 5, ctr[0], vp(info), vp(adv))); ctr[0] += 1
    fns = {k: mk(k) for k in KINDS}; fns["AdVIL"] = advil
    res = alternate(fns, calls)
    head = "step  D %s, %d + %d columns, %d calls per window, %d rounds" % ("-".join(map(str, dims)), B, B, calls, ROUNDS)
    return [head] + ["  %-6s %8.1f us  (%.1f .. %.1f)%s" % (k, m * 1e6, lo * 1e6, hi * 1e6, "   %.2f x BCE" % (m / res["BCE"][0]) if k != "BCE" else "") for k, (m, lo, hi) in res.items()]


def round_bench(calls=20):
    """examples/nda_gail_pendulum.py: 3 obs / 1 act, D 4-64-64-1, 512 demonstration rows, dN 1024, 4 epochs of minibatches of 256"""
    od, ad, hidden, n_demo, dN, B, epochs = 3, 1, [64, 64], 512, 1024, 256, 4
    rng = np.random.default_rng(0); mkn = lambda dims, seed: crux.ContinuousNetwork(chain(dims), seed=seed)
    V, Vc = mkn([od, 64, 64, 1], 2), mkn([od, 64, 64, 1], 5)
    demo, nda = buf(od, ad, rows(rng, od, ad, n_demo)), buf(od, ad, rows(rng, od, ad, n_demo))
    bd = rows(rng, od, ad, dN); batch, cD, cN = buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS)
    rD, rN, o3, k = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32), [0]
    pairs = {}
    for name in ("BCE", "Hinge"):
        D, N = mkn([od + ad] + hidden + [1], 3), mkn([od + ad] + hidden + [1], 4)
        for q in (D, N):
            q.attach_optimizer(crux.Adam(np.float32(1e-5)))
        pairs[name] = (D, N)

    def bce():
        D, N = pairs["BCE"]
        ctx.check(ctx.lib.crux_nda_gail_round(D.h, N.h, demo.h, nda.h, batch.h, cD.h, cN.h, V.h, Vc.h, B, epochs, 0, 11, k[0], B, epochs, 0, 12, k[0], 0.5, 0.95, 0.99, vp(rD), vp(rN), vp(o3))); k[0] += epochs

    def hinge():
        D, N = pairs["Hinge"]
        ctx.check(ctx.lib.crux_nda_gail_round_gan(D.h, N.h, demo.h, nda.h, batch.h, cD.h, cN.h, V.h, Vc.h, B, epochs, 0, 11, k[0], B, epochs, 0, 12, k[0], 0.5, 0.95, 0.99, KINDS["Hinge"],
                                                  vp(rD), vp(rN), vp(o3))); k[0] += epochs
    res = alternate({"BCE": bce, "Hinge": hinge}, calls)
    head = "round pendulum: D 4-64-64-1, %d demo rows, dN %d, batch %d, %d epochs (%d discriminator steps), %d calls per window, %d rounds" % (
        n_demo, dN, B, epochs, 2 * epochs * min(-(-n_demo // B), -(-dN // B)), calls, ROUNDS)
    return [head] + ["  %-6s %8.3f ms  (%.3f .. %.3f)%s" % (n, m * 1e3, lo * 1e3, hi * 1e3, "   %.2f x BCE" % (m / res["BCE"][0]) if n != "BCE" else "") for n, (m, lo, hi) in res.items()]


if __name__ == "__main__":
    lines = ["GAIL discriminator losses: per-call host time, every call ending in its own synchronisation; median window (min .. max over the rounds), kinds alternating"]
    lines += step_bench(3, 1, [64, 64]) + step_bench(17, 6, [256, 256]) + round_bench()
    out = "\n".join(lines)
    print(out)
    os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
    with open(os.path.join(R, "profiles", "gan_loss_bench.txt"), "w") as f:
        f.write(out + "\n")
