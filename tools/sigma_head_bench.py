"""Two-headed Gaussian actors in SAC: us per crux_sac_actor_step and per chained value_training epoch (crux_sac_epochs, 8 epochs per list: rand!, target, temperature,
critics, actor, polyak), each for a constant-logSigma GaussianPolicy actor and for the two-headed SquashedGaussianPolicy actor (logSigma a second Dense(h, ad) head on the same
trunk, ascale 2) on one build, at 3-256-256 / ad 1 and 17-256-256 / ad 6, B = 256. Device-synchronised host timing after warm-up; medians of 5 windows.
No ratio is fixed in advance: the two-headed step pays one wider output layer and the heavier head, and saves the logSigma row-sum launch. The constant-logSigma epoch at
3-256-256 / ad 1 takes the tile plan (exec.hip: SacRun::epoch_tiles), which two-headed actors never do: that line compares plans as well as heads."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402


def chain(dims, acts):
    return crux.Chain(*[crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(acts))])


def actor(od, ad, h, two):
    if not two:
        return crux.GaussianPolicy(chain([od, h, h, ad], ["relu", "relu", "identity"]), np.full(ad, -0.5, np.float32), seed=1)
    base = [crux.Dense(od, h, "relu"), crux.Dense(h, h, "relu")]
    return crux.SquashedGaussianPolicy(crux.Chain(*base, crux.Dense(h, ad)), crux.Chain(*base, crux.Dense(h, ad)), 2.0, seed=1)


def median_us(f, k, windows=5):
    ctx = crux.default_context()
    for i in range(5):
        f(i)
    out = []
    for w in range(windows):
        ctx.sync(); t0 = time.perf_counter()
        for i in range(k):
            f(w * k + i)
        ctx.sync(); out.append(1e6 * (time.perf_counter() - t0) / k)
    return float(np.median(out)), float(min(out)), float(max(out))


def run(od, ad, two, B=256, h=256, reps=200):
    ctx = crux.default_context(); rng = np.random.default_rng(0); n = 8 * B
    A = actor(od, ad, h, two); At = crux.clone_policy(A)
    qs = [crux.ContinuousNetwork(chain([od + ad, h, h, 1], ["relu", "relu", "identity"]), seed=s) for s in (2, 3, 2, 3)]
    la = crux.ParamVector([np.float32(np.log(0.2))], ctx=ctx)
    for net in [A] + qs[:2] + [la]:
        net.attach_optimizer(crux.Adam(np.float32(3e-4)))
    buf = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), n, ctx=ctx); D = crux.buffer_like(buf, capacity=B)
    buf.push_({"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
               "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool)})
    crux.uniform_sample_(D, buf, B, i=1)
    raw = np.zeros(crux._lib.INFO_N, np.float32); rp = raw.ctypes.data_as(C.c_void_p)
    step = lambda i: ctx.check(ctx.lib.crux_sac_actor_step(A.h, qs[0].h, qs[1].h, la.h, D.h, 7, 100 + i, rp))      # noqa: E731
    E = 8; rows = [np.zeros((E, crux._lib.INFO_N), np.float32) for _ in range(3)]; vp = [r.ctypes.data_as(C.c_void_p) for r in rows]
    epochs = lambda i: ctx.check(ctx.lib.crux_sac_epochs(A.h, qs[0].h, qs[1].h, At.h, qs[2].h, qs[3].h, la.h, buf.h, D.h, 0.99, -float(ad), 0.005, 0, 0, E, 1, 1,      # noqa: E731
                                                         1000 + E * i, 7, 3 * (1000 + E * i), *vp))
    t_s, t_e = median_us(step, reps), median_us(epochs, reps // 8)
    r = {"shape": "%d-%d-%d/ad %d" % (od, h, h, ad), "actor": "two-headed squashed (ascale 2)" if two else "constant-logSigma Gaussian", "B": B, "actor_outputs": 2 * ad if two else ad,
         "actor_step_us": round(t_s[0], 1), "actor_step_us_min_max": [round(t_s[1], 1), round(t_s[2], 1)],
         "chained_epoch_us": round(t_e[0] / E, 1), "chained_epoch_us_min_max": [round(t_e[1] / E, 1), round(t_e[2] / E, 1)]}
    print(json.dumps(r)); sys.stdout.flush()
    return r


if __name__ == "__main__":
    for od, ad in ((3, 1), (17, 6)):
        for two in (False, True):
            run(od, ad, two)
