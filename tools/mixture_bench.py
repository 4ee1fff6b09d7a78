"""us per crux_mixture_step (the grouped step of csrc/mixture.hip) against the same step run component by component through the per-handle entries: per component
crux_mlp_forward_cached, crux_mlp_backward, crux_adam_apply, and the same three for the weight network. The baseline's head is free: every handle is seeded with one fixed
output gradient uploaded before the clock starts, and it forms no density, no logSigma gradient, no loss, no norm and reads nothing back -- all of which favours the
baseline.

    python tools/mixture_bench.py > profiles/mixture_bench.txt

Per shape: 20 warm-up steps of either side, then 7 repeats of 200 steps each, the two sides alternating within a repeat, timed on the host around a final crux_sync (the
grouped entry synchronises once per step, as it does for its callers); the median repeat and the spread (min .. max) are reported, with the launches per step counted from
the entry's structure. A measurement path that finds no GPU fails."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux  # noqa: E402
from crux_jl_amd import _lib as L  # noqa: E402

# (component dims, weight-network dims, K, B): the reference's DeepGMM, and a locomotion-sized policy
SHAPES = [((2, 32, 1), (2, 32, 2), 2, 256), ((17, 256, 256, 6), (17, 64, 5), 5, 256)]
WARM, REPS, STEPS = 20, 7, 200


def chain(dims):
    return crux.Chain(*[crux.Dense(dims[l], dims[l + 1], "relu" if l + 2 < len(dims) else "identity") for l in range(len(dims) - 1)])


def handles(ctx, dims, wdims, K):
    nets = [crux.GaussianPolicy(chain(dims), np.zeros(dims[-1], np.float32), ctx=ctx, seed=1, stream=k) for k in range(K)]
    w = crux.ContinuousNetwork(chain(wdims), ctx=ctx, seed=1, stream=K)
    for n in nets + [w]:
        n.attach_optimizer(crux.Adam(np.float32(1e-4)))
    return nets, w


def window(fn, ctx):
    t0 = time.perf_counter()
    for _ in range(STEPS):
        fn()
    ctx.sync(); return (time.perf_counter() - t0) / STEPS * 1e6


def main():
    ctx = crux.default_context(); lib = ctx.lib; rng = np.random.default_rng(0)
    print("mixture step, %d warm-up + %d x %d steps per side (alternating), us per step: median (min .. max)" % (WARM, REPS, STEPS))
    for dims, wdims, K, B in SHAPES:
        nd = dims[-1]; Lc, Lw = len(dims) - 1, len(wdims) - 1
        s = np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32)); a = np.asfortranarray(rng.normal(0, 1, (nd, B)).astype(np.float32))
        dy = np.asfortranarray((rng.normal(0, 1, (nd, B)) / B).astype(np.float32)); dz = np.asfortranarray((rng.normal(0, 1, (K, B)) / B).astype(np.float32))
        ds, da, ddy, ddz = (ctx.alloc(v.nbytes) for v in (s, a, dy, dz))
        for p, v in ((ds, s), (da, a), (ddy, dy), (ddz, dz)):
            ctx.h2d(p, v)
        (gn, gw), (sn, sw) = handles(ctx, dims, wdims, K), handles(ctx, dims, wdims, K)
        arr = (C.c_void_p * K)(*[n.h.value for n in gn]); info = np.zeros(L.INFO_N + K, np.float32); ip = info.ctypes.data_as(C.c_void_p)

        def step_grouped():
            ctx.check(lib.crux_mixture_step(arr, K, gw.h, ds, da, None, B, ip))

        def step_single():
            for n, seed in [(n, ddy) for n in sn] + [(sw, ddz)]:
                ctx.check(lib.crux_mlp_forward_cached(n.h, ds, B, None)); ctx.check(lib.crux_mlp_backward(n.h, ds, B, seed, 1.0, 1, None)); ctx.check(lib.crux_adam_apply(n.h, 1.0))
        for _ in range(WARM):
            step_grouped(); step_single()
        ctx.sync(); g, o = [], []
        for _ in range(REPS):
            g.append(window(step_grouped, ctx)); o.append(window(step_single, ctx))
        assert np.isfinite(info[:2]).all(), info
        lg = Lc + Lw + 2 + (2 * Lc - 1) + (2 * Lw - 1) + 2
        name = "-".join(map(str, dims)); tag = "%-13s K %d B %3d" % (name, K, B)
        print("%s  grouped    %8.1f (%.1f .. %.1f)  launches %3d at most (+ 1 memset, 1 read-back); weight network %s" % (tag, np.median(g), min(g), max(g), lg, "-".join(map(str, wdims))))
        print("%s  per-handle %8.1f (%.1f .. %.1f)  launches: (K + 1) x (forward + pullback + Adam), no head, no norm, no read-back" % (tag, np.median(o), min(o), max(o)))
        print("%s  ratio per-handle / grouped %.2f" % (tag, np.median(o) / np.median(g)))
        for p in (ds, da, ddy, ddz):
            ctx.free(p)


if __name__ == "__main__":
    main()
