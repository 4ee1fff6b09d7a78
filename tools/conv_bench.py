"""The convolutional trunk and crux_conv_td_step beside the same work in torch-ROCm eager (f32 conv2d + linear + Adam) on the same card; writes profiles/conv_bench.txt with --save.

Shapes: the Atari trunk 80x80x4 -> 16@(8,8)/4 relu -> 32@(4,4)/2 relu (2048 features) for the trunk's own passes: forward alone, backward alone and both (host clock around
synchronised windows; kernel-by-kernel times are a profiler's job and are not taken here). The default mode times the whole DQN step on the stand-in
80x80x4 -> 16@(8,8)/4 -> 16@(4,4)/2 -> flatten -> 1024-256-6 that profiles/conv_bench.txt was measured on (a head crux_mlp_create takes); the true 2048-256-6 head of
examples/rl/atari.jl is --atari's (below). B = 32 and 128.
The torch side runs in a child process of its own (torch brings its own HIP runtime; with the library's already initialised in the process it found no device), after the
library's side, on the same card; every figure is the median of `reps` windows of `n` steps after a warm-up of the same shape. If the child fails the line says "not measured".

--atari: the TRUE network and optimiser of examples/rl/atari.jl -- 80x80x4 -> 16@(8,8)/4 -> 32@(4,4)/2 -> flatten -> Dense(2048, 256, relu) -> Dense(256, 6) (the head is a wide
handle, crux_mlp_create_wide) with Optimiser(ClipValue(1), Adam(1e-3)) and with plain Adam(1e-3), B = 32 -- beside torch-ROCm eager with clip_grad_value_ before Adam.step.
The head's forward (crux_mlp_forward_cached) and backward (crux_mlp_backward) are timed alone on the trunk's features; the update has no entry of its own, so its line is the
whole step minus the four passes (derived, and says so). Writes profiles/conv_atari_bench.txt with --save."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)


def chain(c2, head):
    return crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((8, 8), 4, 16, "relu", stride=4), crux.Conv((4, 4), 16, c2, "relu", stride=2), crux.flatten,
                      crux.Dense(64 * c2, head, "relu"), crux.Dense(head, 6), input=(80, 80, 4))


def median_window(fn, sync, n, reps):
    fn(); sync(); out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync(); out.append(1e6 * (time.perf_counter() - t0) / n)
    return float(np.median(out)), float(min(out)), float(max(out))


def torch_side(c2, B, x_host, with_head):
    import torch
    dev = torch.device("cuda")
    conv1, conv2 = torch.nn.Conv2d(4, 16, 8, 4), torch.nn.Conv2d(16, c2, 4, 2)
    mods = [conv1, torch.nn.ReLU(), conv2, torch.nn.ReLU(), torch.nn.Flatten()] + ([torch.nn.Linear(64 * c2, 256), torch.nn.ReLU(), torch.nn.Linear(256, 6)] if with_head else [])
    net = torch.nn.Sequential(*mods).to(dev); opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    x = torch.tensor(x_host.T.reshape(B, 4, 80, 80).copy(), device=dev); y = torch.zeros(B, device=dev); a = torch.zeros(B, dtype=torch.long, device=dev)
    dy = torch.ones(B, 64 * c2, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        q = net(x * (1.0 / 255.0)).gather(1, a[:, None])[:, 0]
        loss = ((q - y) ** 2).mean(); loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), float("inf"))      # the gradient norm the device step also forms
        opt.step(); return loss

    def passes():
        opt.zero_grad(set_to_none=True); net(x * (1.0 / 255.0)).backward(dy)
    return (step if with_head else passes), torch.cuda.synchronize


def torch_atari_step(B, x_host, clip):
    import torch
    dev = torch.device("cuda")
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 16, 8, 4), torch.nn.ReLU(), torch.nn.Conv2d(16, 32, 4, 2), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(2048, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 6)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    x = torch.tensor(x_host.T.reshape(B, 4, 80, 80).copy(), device=dev); y = torch.zeros(B, device=dev); a = torch.zeros(B, dtype=torch.long, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        q = net(x * (1.0 / 255.0)).gather(1, a[:, None])[:, 0]
        loss = ((q - y) ** 2).mean(); loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), float("inf"))      # the gradient norm the device step also forms
        if clip:
            torch.nn.utils.clip_grad_value_(net.parameters(), 1.0)
        opt.step(); return loss
    return step, torch.cuda.synchronize


def torch_child(a):
    """the torch figures of both shapes and batch sizes as one JSON line"""
    rng = np.random.default_rng(0); out = {}
    if a.atari:
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, 32)).astype(np.float32))
        for clip in (0, 1):
            out["atari_clip%d" % clip] = median_window(*torch_atari_step(32, x, clip), a.n, a.reps)
        print(json.dumps(out)); return
    for B in (32, 128):
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32))
        out["trunk%d" % B] = median_window(*torch_side(32, B, x, False), a.n, a.reps); out["step%d" % B] = median_window(*torch_side(16, B, x, True), a.n, a.reps)
    print(json.dumps(out))


def atari(a, crux, L):
    """atari.jl's network and optimiser, literally, at B = 32: the step with the clamp on and off, and its pieces"""
    ctx = crux.default_context(); rng = np.random.default_rng(0); B = 32; lines = []
    x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32))
    buf = crux.ExperienceBuffer(crux.ContinuousSpace((80, 80, 4)), crux.DiscreteSpace(6), B, ctx=ctx)
    buf.push_({"s": x, "sp": x, "a": np.asfortranarray(np.eye(6, dtype=bool)[:, rng.integers(0, 6, B)]), "r": np.zeros((1, B), np.float32), "done": np.zeros((1, B), bool), "episode_end": np.zeros((1, B), bool)})
    d_t = ctx.alloc(4 * B); ctx.h2d(d_t, np.zeros(B, np.float32)); raw = np.zeros(L.INFO_N, np.float32); ours = {}
    for clip in (0, 1):
        pi = crux.DiscreteNetwork(chain(32, 256), list(range(6)), seed=2, ctx=ctx)
        pi.attach_optimizer(crux.Optimiser(crux.ClipValue(1.0), crux.Adam(np.float32(1e-3))) if clip else crux.Adam(np.float32(1e-3)))
        sync_step = lambda: ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_t, 0, raw.ctypes.data_as(C.c_void_p)))      # noqa: E731
        enq_step = lambda: ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_t, 0, None))                                  # noqa: E731
        ours[clip] = (median_window(sync_step, ctx.sync, a.n, a.reps), median_window(enq_step, ctx.sync, a.n, a.reps))
    # the pieces, on the last policy: trunk passes, then the head's passes on the trunk's features
    t = pi.trunk; F = t.spec.out_features
    d_x, d_f, d_df, d_q = ctx.alloc(x.nbytes), ctx.alloc(4 * F * B), ctx.alloc(4 * F * B), ctx.alloc(4 * 6 * B)
    ctx.h2d(d_x, x); ctx.h2d(d_q, np.ones((6, B), np.float32)); ctx.check(ctx.lib.crux_conv_forward(t.h, t.p.h, d_x, B, d_f)); ctx.h2d(d_df, np.ones((F, B), np.float32))
    tfw = lambda: ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, None))                      # noqa: E731
    tbw = lambda: ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_df, 1.0, 1, None))               # noqa: E731
    hfw = lambda: ctx.check(ctx.lib.crux_mlp_forward_cached(pi.head_h, d_f, B, None))                         # noqa: E731
    hbw = lambda: ctx.check(ctx.lib.crux_mlp_backward(pi.head_h, d_f, B, d_q, 1.0, 1, d_df))                  # noqa: E731
    pieces = {k: median_window(f, ctx.sync, a.n, a.reps) for k, f in (("trunk forward", tfw), ("trunk backward", tbw), ("head forward", hfw), ("head backward", hbw))}
    for d in (d_x, d_f, d_df, d_q, d_t):
        ctx.free(d)
    ctx.sync()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--atari", "--n", str(a.n), "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
    try:
        tor = json.loads(child.stdout.strip().splitlines()[-1])
    except Exception:      # noqa: BLE001
        tor = None; sys.stderr.write(child.stderr[-2000:])
    name = {0: "Adam(1e-3)", 1: "Optimiser(ClipValue(1), Adam(1e-3))"}
    for clip in (0, 1):
        ts, te = ours[clip]
        tt = "torch eager: not measured (the torch child process failed)" if tor is None else "torch eager%s %.1f us (%.1f .. %.1f); ratio torch / ours %.2f" % (
            " with clip_grad_value_" if clip else "", tor["atari_clip%d" % clip][0], tor["atari_clip%d" % clip][1], tor["atari_clip%d" % clip][2], tor["atari_clip%d" % clip][0] / ts[0])
        lines.append("td step 80x80x4 -> 16@8/4 -> 32@4/2 -> 2048-256-6, %s, B 32: crux_conv_td_step %.1f us with the info row (%.1f .. %.1f), %.1f us enqueued only (%.1f .. %.1f); %s"
                     % (name[clip], ts[0], ts[1], ts[2], te[0], te[1], te[2], tt))
    for k in ("trunk forward", "trunk backward", "head forward", "head backward"):
        what = {"head forward": " (2048-256-6: M 256, N 32, K 2048 then M 6, K 256; crux_mlp_forward_cached)", "head backward": " (crux_mlp_backward, parameter and input gradients)"}.get(k, "")
        lines.append("%s%s, B 32: %.1f us (%.1f .. %.1f)" % (k, what, pieces[k][0], pieces[k][1], pieces[k][2]))
    passes = sum(pieces[k][0] for k in pieces)
    for clip in (0, 1):
        lines.append("update, %s (DERIVED: the enqueued step minus the four passes above; it also holds the TD head, the norm and the info row): %.1f us" % (name[clip], ours[clip][1][0] - passes))
    d_on, d_off = ours[1][1], ours[0][1]
    lines.append("clamp on vs off, enqueued step: %.1f us (%.1f .. %.1f) vs %.1f us (%.1f .. %.1f): %s" % (d_on[0], d_on[1], d_on[2], d_off[0], d_off[1], d_off[2],
                 "inside the run-to-run spread" if d_on[0] <= d_off[2] else "the clamp-on step is SLOWER than the clamp-off step beyond the spread of these windows"))
    txt = "# tools/conv_bench.py --atari: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_atari_bench.txt"), "w").write(txt)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--n", type=int, default=200); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--save", action="store_true")
    ap.add_argument("--torch-child", action="store_true"); ap.add_argument("--atari", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a)
    global crux
    import crux_jl_amd as crux
    from crux_jl_amd import _lib as L
    if a.atari:
        return atari(a, crux, L)
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines, ours = [], {}
    for B in (32, 128):
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32))
        # ---- the trunk's own passes at the Atari shape
        t = crux.ConvTrunk(chain(32, 256).conv, ctx=ctx, seed=1); F = t.spec.out_features
        d_x, d_y, d_dy = ctx.alloc(x.nbytes), ctx.alloc(4 * F * B), ctx.alloc(4 * F * B); ctx.h2d(d_x, x); ctx.h2d(d_dy, np.ones((F, B), np.float32))
        fwd = lambda: ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, None))                                   # noqa: E731
        bwd = lambda: ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_dy, 1.0, 1, None))                           # noqa: E731
        both = lambda: (fwd(), bwd())                                                                                          # noqa: E731
        tf, tb, tw = median_window(fwd, ctx.sync, a.n, a.reps), median_window(bwd, ctx.sync, a.n, a.reps), median_window(both, ctx.sync, a.n, a.reps)
        ours["trunk%d" % B] = (tw, "trunk 80x80x4 -> 16@8/4 -> 32@4/2 (2048 features)  B %3d: forward (2 launches) %.1f us, backward (6 launches: act', 2 x (wgrad + combine), 1 dgrad) %.1f us, "
                               "forward + backward %.1f us (%.1f .. %.1f)" % (B, tf[0], tb[0], tw[0], tw[1], tw[2]))
        for d in (d_x, d_y, d_dy):
            ctx.free(d)
        # ---- the whole step on the widest head the dense handle takes
        pi = crux.DiscreteNetwork(chain(16, 256), list(range(6)), seed=2, ctx=ctx); pi.attach_optimizer(crux.Adam(np.float32(1e-3)))
        buf = crux.ExperienceBuffer(crux.ContinuousSpace((80, 80, 4)), crux.DiscreteSpace(6), B, ctx=ctx)
        buf.push_({"s": x, "sp": x, "a": np.asfortranarray(np.eye(6, dtype=bool)[:, rng.integers(0, 6, B)]), "r": np.zeros((1, B), np.float32), "done": np.zeros((1, B), bool), "episode_end": np.zeros((1, B), bool)})
        d_t = ctx.alloc(4 * B); ctx.h2d(d_t, np.zeros(B, np.float32)); raw = np.zeros(L.INFO_N, np.float32)
        sync_step = lambda: ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_t, 0, raw.ctypes.data_as(C.c_void_p)))      # noqa: E731
        enq_step = lambda: ctx.check(ctx.lib.crux_conv_td_step(pi.trunk.h, pi.trunk.p.h, pi.head_h, buf.h, d_t, 0, None))                                  # noqa: E731
        ts, te = median_window(sync_step, ctx.sync, a.n, a.reps), median_window(enq_step, ctx.sync, a.n, a.reps)
        ours["step%d" % B] = (ts, "td step 80x80x4 -> 16@8/4 -> 16@4/2 -> 1024-256-6 (the stand-in head; atari.jl's 2048-256-6 is --atari's)  B %3d: crux_conv_td_step (19 launches + 1 memset) "
                              "%.1f us with the info row (%.1f .. %.1f), %.1f us enqueued only" % (B, ts[0], ts[1], ts[2], te[0]))
        ctx.free(d_t)
    ctx.sync()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--n", str(a.n), "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
    try:
        tor = json.loads(child.stdout.strip().splitlines()[-1])
    except Exception:      # noqa: BLE001
        tor = None; sys.stderr.write(child.stderr[-2000:])
    for key in ("trunk32", "step32", "trunk128", "step128"):
        tw, text = ours[key]
        if tor is None:
            lines.append(text + "; torch eager: not measured (the torch child process failed)")
        else:
            tt = tor[key]; lines.append(text + "; torch eager %s %.1f us (%.1f .. %.1f); ratio torch / ours %.2f" % ("forward + backward" if key.startswith("trunk") else "step", tt[0], tt[1], tt[2], tt[0] / tw[0]))
    txt = "# tools/conv_bench.py: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_bench.txt"), "w").write(txt)


if __name__ == "__main__":
    main()
