"""AdVIL's device calls at the HalfCheetah shape (actor 17 -> 64 -> 64 -> 6, D 23 -> 256 -> 256 -> 1, tanh), B = 128 and B = 4000: us per crux_advil_d_step, per
crux_advil_actor_step and per crux_orthogonal_reg (the actor's, value + gradient), and next to them crux_iq_step with the gradient penalty at the same width
(Q 23 -> 256 -> 256 -> 6 over B rows, B / 2 penalty columns). One process; after a warm-up every figure is the median over timed blocks of device-synchronised
host time per call, with the fastest and slowest block beside it. Every call ends in its own host synchronisation (the info read), so a figure includes one round
trip. One JSON line per batch size. There is no threshold on these times: the calls have no earlier form to compare with."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402

WARMUP, BLOCKS, PER_BLOCK = 20, 9, 40


def chain(dims, act):
    acts = [act] * (len(dims) - 2) + ["identity"]
    return crux.Chain(*[crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(acts))])


def timed(ctx, fn):
    for i in range(WARMUP):
        fn(i)
    us = []
    for b in range(BLOCKS):
        ctx.sync(); t0 = time.perf_counter()
        for i in range(PER_BLOCK):
            fn(WARMUP + b * PER_BLOCK + i)
        ctx.sync(); us.append(1e6 * (time.perf_counter() - t0) / PER_BLOCK)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def run(B, od=17, ad=6, act="tanh"):
    ctx = crux.default_context(); rng = np.random.default_rng(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731
    A = crux.ContinuousNetwork(chain([od, 64, 64, ad], act), seed=1); D = crux.ContinuousNetwork(chain([od + ad, 256, 256, 1], act), seed=2)
    A.attach_optimizer(crux.Adam(np.float32(1e-5))); D.attach_optimizer(crux.Adam(np.float32(1e-5)))
    data = {"s": rng.normal(0, 1, (od, B)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, B)).astype(np.float32), "sp": rng.normal(0, 1, (od, B)).astype(np.float32),
            "r": np.zeros((1, B), np.float32), "done": np.zeros((1, B), bool)}
    mb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), B, ctx=ctx); mb.push_(data)
    info, adv, val = np.zeros(crux._lib.INFO_N, np.float32), np.zeros(4, np.float32), np.zeros(1, np.float32)
    r = {"B": B, "actor": "%d-64-64-%d" % (od, ad), "D": "%d-256-256-1" % (od + ad), "act": act, "warmup": WARMUP, "blocks": BLOCKS, "calls_per_block": PER_BLOCK}
    r["advil_d_step"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_advil_d_step(A.h, D.h, mb.h, 10.0, 0.4, 0, 8 * i + 5, vp(info), vp(adv))))
    r["d_loss"], r["grad_pen"] = float(info[0]), float(adv[2])
    r["advil_actor_step"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_advil_actor_step(A.h, D.h, mb.h, 0.2, 1e-4, vp(info), vp(adv))))
    r["actor_loss"], r["bc_mse"] = float(info[0]), float(adv[1])
    r["advil_actor_step_no_reg"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_advil_actor_step(A.h, D.h, mb.h, 0.2, 0.0, vp(info), vp(adv))))
    r["orthogonal_reg_actor"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_orthogonal_reg(A.h, 1e-4, 1, vp(val))))
    r["orthogonal_reg_D"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_orthogonal_reg(D.h, 1e-4, 1, vp(val))))
    # crux_iq_step with gp at the same width: a DiscreteNetwork over the 23-wide columns, B rows (half of them demo rows), B / 2 penalty columns
    nA = 6
    Q = crux.DiscreteNetwork(chain([od + ad, 256, 256, nA], act), list(range(1, nA + 1)), seed=3); Q.attach_optimizer(crux.Adam(np.float32(1e-5)))
    qd = {"s": rng.normal(0, 1, (od + ad, B)).astype(np.float32), "a": np.eye(nA, dtype=bool)[rng.integers(0, nA, B)].T.copy(),
          "sp": rng.normal(0, 1, (od + ad, B)).astype(np.float32), "r": np.zeros((1, B), np.float32), "done": rng.random((1, B)) < 0.05}
    qb = crux.ExperienceBuffer(crux.ContinuousSpace(od + ad), crux.DiscreteSpace(nA), B, ctx=ctx); qb.push_(qd)
    iq = np.zeros(6, np.float32)
    r["iq_step_gp"] = timed(ctx, lambda i: ctx.check(ctx.lib.crux_iq_step(Q.h, qb.h, B // 2, 0.9, 1, 0.5, 1, 10.0, 0, i, vp(info), vp(iq))))
    print(json.dumps(r)); sys.stdout.flush()
    return r


if __name__ == "__main__":
    for B in (128, 4000):
        run(B)
