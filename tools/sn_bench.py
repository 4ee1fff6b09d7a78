"""What spectral normalisation of the discriminator costs on the device (csrc/spectral.hip), written to profiles/sn_bench.txt.

  python tools/sn_bench.py                  us per crux_offgail_d_step (K = 2, Bd = 128: 256 columns) and ms per 16-step crux_nda_gail_round, each with a plain
                                            and with a DenseSN discriminator, at the example shape (D 4-64-64-out) and the HalfCheetah shape (D 23-256-256-out)
  python tools/sn_bench.py --plain-only      the two plain crux_offgail_d_step timings alone, printed and not written: run from a checkout of the parent commit as well
                                            (copy this file there), in the same session, for the A/B of the plain step
  python tools/sn_bench.py --round-only N   N off-policy rounds (5 steps + reward) with the DenseSN discriminator and nothing else: the program to put after
                                            `rocprofv3 --kernel-trace --` for the launch list of one round

Fresh process, wall-clock around synchronising calls, a warm-up block, then the median [min, max] of `--repeats` blocks of `--iters` calls; one stream.
By launch count the SN step adds one k_sn_power launch per forward pass and one k_sn_grad launch per backward pass to a step of about ten launches.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402
from crux_jl_amd import _lib as L  # noqa: E402

SEED = 0x5EED5A3F
EXTRAS = ["return", "advantage", "logprob", "cost", "cost_advantage", "cost_return"]


def rows(rng, od, ad, n, T=64):
    ee = np.zeros((1, n), bool); ee[0, T - 1::T] = True
    return {"s": rng.normal(0, 1, (od, n)).astype(np.float32), "a": rng.uniform(-1, 1, (ad, n)).astype(np.float32), "sp": rng.normal(0, 1, (od, n)).astype(np.float32),
            "r": rng.normal(0, 1, (1, n)).astype(np.float32), "done": ee.copy(), "episode_end": ee}


def buf(od, ad, d, extras=()):
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), d["s"].shape[1], list(extras)); b.push_(d); return b


def disc(dims, sn, seed):
    lay = crux.DenseSN if sn else crux.Dense
    D = crux.ContinuousNetwork(crux.Chain(*[lay(i, o, "relu" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]), seed=seed)
    D.attach_optimizer(crux.Adam(np.float32(3e-4))); return D


def timed(fn, iters, repeats):
    for _ in range(iters):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append((time.perf_counter() - t0) / iters)
    return float(np.median(out)), float(min(out)), float(max(out))


def off_step(od, ad, hidden, sn, iters, repeats, Bd=128):
    rng = np.random.default_rng(0)
    srcs = [buf(od, ad, rows(rng, od, ad, n)) for n in (4096, 100000)]
    D = disc([od + ad] + hidden + [2], sn, 1); k = [0]

    def step():
        crux.offgail_d_step_(D, srcs, Bd, SEED, k[0]); k[0] += 1
    return tuple(1e6 * t for t in timed(step, iters, repeats))


def nda_round(od, ad, hidden, sn, iters, repeats, n_demo, dN, B=256, epochs=4):
    ctx = crux.default_context(); lib = ctx.lib; rng = np.random.default_rng(0); vp = lambda a: a.ctypes.data_as(L.vp)      # noqa: E731
    D, N = disc([od + ad] + hidden + [1], sn, 3), disc([od + ad] + hidden + [1], sn, 4)
    V, Vc = disc([od, 64, 64, 1], False, 2), disc([od, 64, 64, 1], False, 5)
    demo, nda = buf(od, ad, rows(rng, od, ad, n_demo)), buf(od, ad, rows(rng, od, ad, n_demo))
    bd = rows(rng, od, ad, dN); batch, cD, cN = buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS), buf(od, ad, bd, EXTRAS)
    k = [0]; rD, rN, o3 = np.zeros(L.INFO_N, np.float32), np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)

    def round_():
        ctx.check(lib.crux_nda_gail_round(D.h, N.h, demo.h, nda.h, batch.h, cD.h, cN.h, V.h, Vc.h, B, epochs, 0, 11, k[0], B, epochs, 0, 12, k[0], 0.5, 0.95, 0.99, vp(rD), vp(rN), vp(o3)))
        k[0] += epochs
    return tuple(1e3 * t for t in timed(round_, iters, repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100); ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--round-only", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sn_bench.txt"))
    a = ap.parse_args()
    if a.round_only:
        rng = np.random.default_rng(0)
        srcs = [buf(3, 1, rows(rng, 3, 1, n)) for n in (4096, 100000)]; batch = buf(3, 1, rows(rng, 3, 1, 256)); D = disc([4, 64, 64, 2], True, 1)
        for n in range(a.round_only):
            crux.offgail_round_(D, srcs, 128, 5, batch, SEED, 5 * n)
        return
    if a.plain_only:
        for name, od, ad, hidden in (("example      D 4-64-64", 3, 1, [64, 64]), ("halfcheetah  D 23-256-256", 17, 6, [256, 256])):
            print("%s-2, crux_offgail_d_step, 2 x 128 columns: plain %7.1f us [%.1f, %.1f]" % ((name,) + off_step(od, ad, hidden, False, a.iters, a.repeats)))
        return
    lines = ["DenseSN against plain Dense discriminators (tools/sn_bench.py): median [min, max] of %d blocks of %d calls after a warm-up block" % (a.repeats, a.iters)]
    for name, od, ad, hidden, n_demo, dN in (("example      D 4-64-64", 3, 1, [64, 64], 512, 1024), ("halfcheetah  D 23-256-256", 17, 6, [256, 256], 512, 1024)):
        p, s = off_step(od, ad, hidden, False, a.iters, a.repeats), off_step(od, ad, hidden, True, a.iters, a.repeats)
        lines.append("%s-2, crux_offgail_d_step, 2 x 128 columns: plain %7.1f us [%.1f, %.1f]   SN %7.1f us [%.1f, %.1f]   SN / plain %.2f" % ((name,) + p + s + (s[0] / p[0],)))
        it = max(a.iters // 5, 5)
        p, s = nda_round(od, ad, hidden, False, it, a.repeats, n_demo, dN), nda_round(od, ad, hidden, True, it, a.repeats, n_demo, dN)
        lines.append("%s-1, crux_nda_gail_round, batch 256, 16 steps:     plain %7.3f ms [%.3f, %.3f]   SN %7.3f ms [%.3f, %.3f]   SN / plain %.2f" % ((name,) + p + s + (s[0] / p[0],)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
