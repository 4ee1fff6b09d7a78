"""Times of OffPolicyGAIL's callback and AdRIL's relabel on the device (csrc/gail_off.hip), written to profiles/offgail_bench.txt.

  python tools/offgail_bench.py                  us per crux_offgail_round against the same round composed call by call (uniform_sample! of every source into a
                                                 staging buffer + crux_offgail_d_step per epoch, then crux_offgail_reward); us per crux_adril_relabel at 1 000 and
                                                 1 M rows against the host round trip it replaces (buf["i"], buf["r"] read, buf["r"] written)
  python tools/offgail_bench.py --rounds-only N  N rounds at the Pendulum shape and nothing else: the program to put after `rocprofv3 --kernel-trace --stats --`
                                                 for the launches per round (kernel calls of the trace / N, after subtracting the set-up's)

Wall-clock times around a synchronising call, median of `--repeats` blocks of `--iters` calls after a warm-up block; one process, one stream.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crux_jl_amd as crux  # noqa: E402
import parity  # noqa: E402

SEED = 0x5EED5A3F


def rows(od, ad, n, seed):
    rng = np.random.default_rng(seed)
    return {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.normal(0, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": np.zeros((1, n), bool)}


def buffer(ctx, d, extras=()):
    b = crux.ExperienceBuffer(crux.ContinuousSpace(d["s"].shape[0]), crux.ContinuousSpace(d["a"].shape[0]), d["s"].shape[1], list(extras), ctx=ctx)
    b.push_(d); return b


def timed(fn, iters, repeats):
    for _ in range(iters):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return float(np.median(out)), float(min(out)), float(max(out))


def setup(ctx, od, ad, K, Bd=128, B=256):
    srcs = [buffer(ctx, rows(od, ad, n, 10 + k)) for k, n in enumerate([4096, 100000, 4096][:K])]
    batch = buffer(ctx, rows(od, ad, B, 20))
    D = crux.ContinuousNetwork(parity.chain([od + ad, 256, 256, K], ["relu", "relu", "identity"]), seed=1, stream=0)
    D.attach_optimizer(crux.Adam(np.float32(3e-4)))
    stages = [crux.buffer_like(s, capacity=Bd) for s in srcs]
    return D, srcs, batch, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200); ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--rounds-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offgail_bench.txt"))
    a = ap.parse_args()
    ctx = crux.default_context()
    Bd, E, B = 128, 5, 256
    if a.rounds_only:
        D, srcs, batch, _ = setup(ctx, 3, 1, 2)
        for n in range(a.rounds_only):
            crux.offgail_round_(D, srcs, Bd, E, batch, SEED, n * E)
        return
    lines = ["off-policy GAIL / AdRIL on the device (tools/offgail_bench.py): us per call, median [min, max] of %d blocks of %d calls" % (a.repeats, a.iters)]
    for name, od, ad, K in (("Pendulum 3+1 -> 256 -> 256 -> 2", 3, 1, 2), ("HalfCheetah-sized 17+6 -> 256 -> 256 -> 3", 17, 6, 3)):
        D, srcs, batch, stages = setup(ctx, od, ad, K)
        ctr = [0]

        def fused():
            crux.offgail_round_(D, srcs, Bd, E, batch, SEED, ctr[0]); ctr[0] += E

        def composed():      # what the existing entry points need for the same round: every epoch gathers ALL columns of every source, then one step; then the reward
            for e in range(E):
                for st, s in zip(stages, srcs):
                    crux.uniform_sample_(st, s, B=Bd, i=ctr[0] + e)
                crux.offgail_d_step_(D, srcs, Bd, SEED, ctr[0] + e)
            crux.offgail_reward_(D, batch, K); ctr[0] += E
        f, c = timed(fused, a.iters, a.repeats), timed(composed, max(a.iters // 4, 10), a.repeats)
        lines.append("%s, Bd = %d, d_epochs = %d, B = %d:" % (name, Bd, E, B))
        lines.append("  crux_offgail_round (one synchronisation)                         %8.1f [%.1f, %.1f]" % f)
        lines.append("  composed: %d x (%d uniform_sample! + d_step) + reward (%d synchronisations) %8.1f [%.1f, %.1f]" % ((E, K, E + 1) + c))
    for n in (1000, 1 << 20):
        d = rows(3, 1, n, 30); d["i"] = np.arange(1, n + 1, dtype=np.int64).reshape(1, n)
        ring = buffer(ctx, d, ["i"]); dN = 50 if n == 1000 else 1 << 14

        def dev():
            crux.adril_relabel_(ring, dN, 0, dN)

        def host():
            i, r = ring["i"], ring["r"]
            mx = int(i.max()); k = (mx - 0) // dN - 1
            r[...] = np.where(i <= mx - dN, np.float32(-1.0 / k), np.float32(0)); ring["r"] = r
        dv, hs = timed(dev, a.iters if n == 1000 else 50, a.repeats), timed(host, 50 if n == 1000 else 5, a.repeats)
        lines.append("AdRIL relabel, ring of %d rows: crux_adril_relabel %8.1f [%.1f, %.1f]   host round trip (read i, r; write r) %10.1f [%.1f, %.1f]" % ((n,) + dv + hs))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
