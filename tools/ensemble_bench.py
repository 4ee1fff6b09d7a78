"""us per crux_ensemble_step (the member-grouped step of csrc/ensemble.hip) against the composition the per-handle entries offer for the same members and minibatch:
per member crux_mlp_forward_cached, a head, crux_mlp_backward, crux_adam_apply. The baseline's head is free: every member is seeded with one fixed output
gradient uploaded before the clock starts, and it forms no loss, no norm and reads nothing back -- all of which favours the baseline.

    python tools/ensemble_bench.py > profiles/ensemble_bench.txt

Per shape: 20 warm-up steps, then 7 repeats of 200 steps each, timed on the host around a final crux_sync (both sides synchronise once per step or per call as their
entries do); the median repeat and the spread (min .. max) are reported, with the launches per step counted from the entry's structure."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux  # noqa: E402
from crux_jl_amd import _lib as L  # noqa: E402

SHAPES = [((8, 64, 64, 2), 128), ((17, 256, 256, 12), 256)]
M, WARM, REPS, STEPS = 5, 20, 7, 200


def members(ctx, dims):
    nets = [crux.ContinuousNetwork(crux.Chain(*[crux.Dense(dims[l], dims[l + 1], "relu" if l + 2 < len(dims) else "identity") for l in range(len(dims) - 1)]), ctx=ctx, seed=1, stream=m) for m in range(M)]
    for n in nets:
        n.attach_optimizer(crux.Adam(np.float32(1e-4)))
    return nets


def timed(fn, ctx):
    for _ in range(WARM):
        fn()
    ctx.sync(); out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        ctx.sync(); out.append((time.perf_counter() - t0) / STEPS * 1e6)
    return np.median(out), min(out), max(out)


def main():
    ctx = crux.default_context(); lib = ctx.lib; rng = np.random.default_rng(0)
    print("ensemble step, M = %d members, %d warm-up + %d x %d steps, us per step: median (min .. max)" % (M, WARM, REPS, STEPS))
    for dims, B in SHAPES:
        nd = dims[-1] // 2; Lyr = len(dims) - 1
        x = np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32)); y = np.asfortranarray(rng.normal(0, 1, (nd, B)).astype(np.float32))
        dy = np.asfortranarray((rng.normal(0, 1, (dims[-1], B)) / (nd * B * M)).astype(np.float32))
        dx, dyy, ddy = ctx.alloc(x.nbytes), ctx.alloc(y.nbytes), ctx.alloc(dy.nbytes); ctx.h2d(dx, x); ctx.h2d(dyy, y); ctx.h2d(ddy, dy)
        grouped, single = members(ctx, dims), members(ctx, dims)
        arr = (C.c_void_p * M)(*[n.h.value for n in grouped]); info = np.zeros(L.INFO_N + 2 * M, np.float32); ip = info.ctypes.data_as(C.c_void_p)

        def step_grouped():
            ctx.check(lib.crux_ensemble_step(arr, M, L.ENS["gauss"], dx, dyy, None, B, ip))

        def step_single():
            for n in single:
                ctx.check(lib.crux_mlp_forward_cached(n.h, dx, B, None)); ctx.check(lib.crux_mlp_backward(n.h, dx, B, ddy, 1.0, 1, None)); ctx.check(lib.crux_adam_apply(n.h, 1.0))
        g, s = timed(step_grouped, ctx), timed(step_single, ctx)
        lg = Lyr + 1 + (2 * Lyr - 1) + 2
        name = "-".join(map(str, dims))
        print("%-14s B %3d  grouped %8.1f (%.1f .. %.1f)  launches %3d (+ 1 memset, 1 read-back)" % (name, B, g[0], g[1], g[2], lg))
        print("%-14s B %3d  per-handle %6.1f (%.1f .. %.1f)  launches: M x (forward + pullback + Adam), no head, no norm, no read-back" % (name, B, s[0], s[1], s[2]))
        print("%-14s ratio per-handle / grouped %.2f" % (name, s[0] / g[0]))
        for p in (dx, dyy, ddy):
            ctx.free(p)


if __name__ == "__main__":
    main()
