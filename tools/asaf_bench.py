"""ASAF's device calls at two shapes: the example's (squashed 2 -> 64 -> 64 -> 1, tanh, B = 256 rollout rows per step, the 512 committed Pendulum demonstrations) and the
HalfCheetah shape (Gaussian 17 -> 64 -> 64 -> 6, tanh, B = 256, the 256 committed HalfCheetah demonstrations). Per shape: us per crux_asaf_actor_step through the step
entry (each call ends in its own host synchronisation), us per step inside crux_asaf_batch_train (one synchronisation per call of epochs x minibatches steps; the epoch
shuffles are inside), us per freeze pass over the rollout buffer and over the demonstrations, and next to the step the same step with the frozen network forwarded every
time (step + both freeze passes over the step's own columns): what the precomputation of gG and gE saves. One process; after a warm-up every figure is the median over
timed blocks of device-synchronised host time per call, with the fastest and slowest block beside it. One JSON line per shape. There is no threshold on these times:
the calls have no earlier form to compare with."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402

WARMUP, BLOCKS, PER_BLOCK = 20, 9, 40
GOLD = os.path.join(ROOT, "tests", "golden")


def chain(dims, act):
    acts = [act] * (len(dims) - 2) + ["identity"]
    return crux.Chain(*[crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(acts))])


def timed(ctx, fn, per_block=PER_BLOCK, div=1):
    for i in range(WARMUP if div == 1 else 3):
        fn(i)
    us = []
    for b in range(BLOCKS):
        ctx.sync(); t0 = time.perf_counter()
        for i in range(per_block):
            fn(WARMUP + b * per_block + i)
        ctx.sync(); us.append(1e6 * (time.perf_counter() - t0) / (per_block * div))
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def run(name, fixture, dims, ascale, B=256, roll=2048, act="tanh"):
    ctx = crux.default_context(); rng = np.random.default_rng(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    od, ad = dims[0], dims[-1]
    d = dict(np.load(os.path.join(GOLD, fixture)))
    S, A = crux.ContinuousSpace(od, mu=d["s"].mean(1).astype(np.float32), sigma=d["s"].std(1).astype(np.float32)), crux.ContinuousSpace(ad)
    ls = np.full(ad, -0.5, np.float32)
    pi = crux.SquashedGaussianPolicy(chain(dims, act), ls, ascale, seed=1) if ascale > 0 else crux.GaussianPolicy(chain(dims, act), ls, seed=1)
    pi.attach_optimizer(crux.Adam(np.float32(1e-5)))
    demo = crux.ExperienceBuffer(S, A, d["s"].shape[1], ctx=ctx); demo.push_({k: d[k] for k in ("s", "a", "sp", "r", "done")}); crux.normalize_(demo, S, A)
    lim = 0.9 * ascale if ascale > 0 else 1.0
    buf = crux.ExperienceBuffer(S, A, roll, ["logprob"], ctx=ctx)
    buf.push_({"s": rng.normal(0, 1, (od, roll)).astype(np.float32), "a": rng.uniform(-lim, lim, (ad, roll)).astype(np.float32), "sp": rng.normal(0, 1, (od, roll)).astype(np.float32),
               "r": np.zeros((1, roll), np.float32), "done": np.zeros((1, roll), bool)})
    NE = len(demo); gE = crux.il_on_policy._DeviceVec(ctx, NE); tmpG, tmpE = crux.il_on_policy._DeviceVec(ctx, roll), crux.il_on_policy._DeviceVec(ctx, NE)
    gG = buf.column_ptr("logprob")
    crux.asaf_freeze_(pi, buf, gG); crux.asaf_freeze_(pi, demo, gE.p)
    info, out = np.zeros(crux._lib.INFO_N, np.float32), np.zeros(3, np.float32)
    lib = ctx.lib
    r = {"shape": name, "policy": "-".join(map(str, dims)), "head": "squashed" if ascale > 0 else "gaussian", "act": act, "B": B, "N_E": NE, "rollout_rows": roll,
         "warmup": WARMUP, "blocks": BLOCKS, "calls_per_block": PER_BLOCK}
    step = lambda i: ctx.check(lib.crux_asaf_actor_step(pi.h, buf.h, (i % (roll // B)) * B, B, gG, demo.h, gE.p, 1.0, vp(info), vp(out)))      # noqa: E731
    r["actor_step"] = timed(ctx, step)
    r["loss"], r["entropy"] = float(info[0]), float(out[0])

    def step_refreeze(i):      # the frozen network forwarded every step over the step's own B + N_E columns, as the reference's loss does
        off = (i % (roll // B)) * B
        ctx.check(lib.crux_asaf_freeze(pi.h, buf.h, off, B, tmpG.p)); ctx.check(lib.crux_asaf_freeze(pi.h, demo.h, 0, NE, tmpE.p))
        ctx.check(lib.crux_asaf_actor_step(pi.h, buf.h, off, B, gG, demo.h, gE.p, 1.0, vp(info), vp(out)))
    r["actor_step_with_frozen_forward"] = timed(ctx, step_refreeze)
    r["freeze_rollout"] = timed(ctx, lambda i: ctx.check(lib.crux_asaf_freeze(pi.h, buf.h, 0, roll, gG)))
    r["freeze_demo"] = timed(ctx, lambda i: ctx.check(lib.crux_asaf_freeze(pi.h, demo.h, 0, NE, gE.p)))
    epochs = 10; nsteps = epochs * (roll // B); rows = np.zeros((epochs, crux.il_on_policy.ASAF_ROW), np.float32)
    chain_call = lambda i: ctx.check(lib.crux_asaf_batch_train(pi.h, buf.h, demo.h, gE.p, B, epochs, 0, 0, i * epochs, 1.0, vp(info), vp(rows)))      # noqa: E731
    r["chain_steps_per_call"] = nsteps
    r["actor_step_in_chain"] = timed(ctx, chain_call, per_block=4, div=nsteps)
    print(json.dumps(r)); sys.stdout.flush()
    return r


if __name__ == "__main__":
    run("pendulum example", "pendulum_transitions.npz", [2, 64, 64, 1], 2.0)
    run("half cheetah", "half_cheetah_mujoco_transitions.npz", [17, 64, 64, 6], 0.0)
