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
whole step minus the four passes (derived, and says so). Writes profiles/conv_atari_bench.txt with --save.

--pg: an actor's and a critic's Atari trunk over one batch (csrc/conv_pair.hip) -- forward + backward paired beside two single passes of the same build, and the whole
crux_conv_pg_step (ppo_loss + critic mse, 2048-256-6 and 2048-256-1 heads) beside two single-trunk steps and beside the same step in torch-ROCm eager; B = 32 and 128.
Writes profiles/conv_pg_bench.txt with --save.

--pg-gauss: one PPO step of crux_conv_pg_step_gauss (csrc/conv_gauss.hip: Gaussian actor, ad = 3, 2048-256-3 and 2048-256-1 heads) beside crux_conv_pg_step with 3 categorical
outputs at the same shapes, B = 32 and 128. Writes profiles/conv_gauss_bench.txt with --save.

--ensemble: M = 5 and 16 conv members over one batch (csrc/conv_group.hip, the conv entries of csrc/ensemble.hip), B = 32 and 128, at 16x16x2 -> 8@(4,4)/2 -> 12@(3,3)/1 with a
300-64-10 head and at the Atari trunk with a 2048-1024-10 head. The grouped passes (crux_conv_ensemble_passes: trunks and heads, forward + backward) beside the same passes member
by member (crux_conv_forward_cached, crux_mlp_forward_cached, crux_mlp_backward with d_dx, crux_conv_backward); and, at the small shape, the whole crux_conv_ensemble_step beside
those passes plus crux_adam_apply per handle (the baseline has no entry for the loss head, the norms or the gate: it does less; it pays one device-to-device copy of the
features per member, because crux_mlp_forward_cached reads them from a caller's buffer: both are said in the output lines). The Atari head is a wide handle, which the step
refuses, so the Atari step is not measured. Writes profiles/conv_ensemble_bench.txt with --save.

--pool: the textbook image network's trunk, 28x28x1 -> Conv((3,3), 1=>8, relu, pad=1) -> MaxPool((2,2)) -> Conv((3,3), 8=>16, relu, pad=1) -> MaxPool((2,2)) -> flatten (784
features), forward + backward (csrc/conv_pool.hip beside the conv kernels) at B = 32 and 128, beside torch-ROCm eager. Writes profiles/conv_pool_bench.txt with --save.

--bc: behaviour cloning at the Atari trunk with a 2048-256-6 head (csrc/conv_bc.hip), B = 32 and 128: crux_conv_bc_step (logpdf_bc_loss, categorical) and crux_conv_bc_loss over
1024 rows in chunks of B, beside the same step and the same forward-only loss (no_grad, the same chunks, one .item()) in torch-ROCm eager. Writes profiles/conv_bc_bench.txt with --save."""
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


def torch_pool(B, x_host):
    import torch
    dev = torch.device("cuda")
    net = torch.nn.Sequential(torch.nn.Conv2d(1, 8, 3, 1, 1), torch.nn.ReLU(), torch.nn.MaxPool2d(2), torch.nn.Conv2d(8, 16, 3, 1, 1), torch.nn.ReLU(), torch.nn.MaxPool2d(2), torch.nn.Flatten()).to(dev)
    x = torch.tensor(x_host.T.reshape(B, 1, 28, 28).copy(), device=dev); dy = torch.ones(B, 784, device=dev)

    def passes():
        net.zero_grad(set_to_none=True); net(x * (1.0 / 255.0)).backward(dy)
    return passes, torch.cuda.synchronize


def pool(a, crux, L):
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines = []
    spec = crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((3, 3), 1, 8, "relu", pad=1), crux.MaxPool((2, 2)), crux.Conv((3, 3), 8, 16, "relu", pad=1), crux.MaxPool((2, 2)), crux.flatten,
                      crux.Dense(784, 10), input=(28, 28, 1)).conv
    ours = {}
    for B in (32, 128):
        x = np.asfortranarray(rng.integers(0, 256, (784, B)).astype(np.float32))
        t = crux.ConvTrunk(spec, ctx=ctx, seed=1); F = t.spec.out_features
        d_x, d_dy = ctx.alloc(x.nbytes), ctx.alloc(4 * F * B); ctx.h2d(d_x, x); ctx.h2d(d_dy, np.ones((F, B), np.float32))
        fwd = lambda: ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, None))                                   # noqa: E731
        bwd = lambda: ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_dy, 1.0, 1, None))                           # noqa: E731
        both = lambda: (fwd(), bwd())                                                                                          # noqa: E731
        ours[B] = (median_window(fwd, ctx.sync, a.n, a.reps), median_window(bwd, ctx.sync, a.n, a.reps), median_window(both, ctx.sync, a.n, a.reps))
        ctx.free(d_x); ctx.free(d_dy)
    ctx.sync()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--pool", "--n", str(a.n), "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
    try:
        tor = json.loads(child.stdout.strip().splitlines()[-1])
    except Exception:      # noqa: BLE001
        tor = None; sys.stderr.write(child.stderr[-2000:])
    for B in (32, 128):
        tf, tb, tw = ours[B]
        tt = "torch eager: not measured (the torch child process failed)" if tor is None else "torch eager forward + backward %.1f us (%.1f .. %.1f); ratio torch / ours %.2f" % (
            tor["pool%d" % B][0], tor["pool%d" % B][1], tor["pool%d" % B][2], tor["pool%d" % B][0] / tw[0])
        lines.append("trunk 28x28x1 -> 8@3/1 pad 1 -> MaxPool 2 -> 16@3/1 pad 1 -> MaxPool 2 (784 features)  B %3d: forward (4 launches) %.1f us, backward (7 launches: 2 x k_pool_bwd, "
                     "2 x (wgrad + combine), 1 dgrad) %.1f us, forward + backward %.1f us (%.1f .. %.1f); %s" % (B, tf[0], tb[0], tw[0], tw[1], tw[2], tt))
    txt = "# tools/conv_bench.py --pool: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_pool_bench.txt"), "w").write(txt)


def torch_child(a):
    """the torch figures of both shapes and batch sizes as one JSON line"""
    rng = np.random.default_rng(0); out = {}
    if a.pool:
        for B in (32, 128):
            out["pool%d" % B] = median_window(*torch_pool(B, np.asfortranarray(rng.integers(0, 256, (784, B)).astype(np.float32))), a.n, a.reps)
        print(json.dumps(out)); return
    if a.bc:
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, 1024)).astype(np.float32)); act = rng.integers(0, 6, 1024)
        for B in (32, 128):
            step, loss_pass, sync = torch_bc(B, x, act)
            out["step%d" % B] = median_window(step, sync, a.n, a.reps); out["loss%d" % B] = median_window(loss_pass, sync, max(a.n // 10, 1), a.reps)
        print(json.dumps(out)); return
    if a.atari:
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, 32)).astype(np.float32))
        for clip in (0, 1):
            out["atari_clip%d" % clip] = median_window(*torch_atari_step(32, x, clip), a.n, a.reps)
        print(json.dumps(out)); return
    if a.pg:
        for B in (32, 128):
            step, passes, sync = torch_pg(B, np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32)))
            out["step%d" % B] = median_window(step, sync, a.n, a.reps); out["passes%d" % B] = median_window(passes, sync, a.n, a.reps)
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


def torch_pg(B, x_host):
    """the PPO step of crux_conv_pg_step restated: actor and critic as two Sequential nets over one batch, clipped surrogate + entropy, critic mse, norms, two Adam steps;
    and the two trunks' forward + backward alone"""
    import torch
    dev = torch.device("cuda")
    mk = lambda nout: torch.nn.Sequential(torch.nn.Conv2d(4, 16, 8, 4), torch.nn.ReLU(), torch.nn.Conv2d(16, 32, 4, 2), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(2048, 256), torch.nn.ReLU(),      # noqa: E731
                                          torch.nn.Linear(256, nout)).to(dev)
    A, V = mk(6), mk(1); oa, ov = torch.optim.Adam(A.parameters(), lr=1e-3), torch.optim.Adam(V.parameters(), lr=1e-3)
    x = torch.tensor(x_host.T.reshape(B, 4, 80, 80).copy(), device=dev); act = torch.zeros(B, dtype=torch.long, device=dev)
    adv, ret, old = torch.randn(B, device=dev), torch.randn(B, device=dev), torch.full((B,), -1.79, device=dev); dy = torch.ones(B, 2048, device=dev)

    def step():
        oa.zero_grad(set_to_none=True); ov.zero_grad(set_to_none=True); xs = x * (1.0 / 255.0)
        p = torch.softmax(A(xs), 1); lp = torch.log(p.gather(1, act[:, None])[:, 0]); r = torch.exp(lp - old)
        loss = -torch.minimum(r * adv, torch.clamp(r, 0.8, 1.2) * adv).mean() + 0.1 * (p * torch.log(p + 1.1920929e-07)).sum(1).mean()
        closs = ((V(xs)[:, 0] - ret) ** 2).mean(); (loss + closs).backward()
        torch.nn.utils.clip_grad_norm_(A.parameters(), float("inf")); torch.nn.utils.clip_grad_norm_(V.parameters(), float("inf"))
        oa.step(); ov.step(); return (old - lp).mean().item()      # the KL the host reads every step

    def passes():
        oa.zero_grad(set_to_none=True); ov.zero_grad(set_to_none=True); xs = x * (1.0 / 255.0)
        A[:5](xs).backward(dy); V[:5](xs).backward(dy)
    return step, passes, torch.cuda.synchronize


def torch_bc(B, x_host, a_host):
    """crux_conv_bc_step restated (logpdf_bc_loss on a categorical head, the norm, one Adam step, the loss read by the host), and the forward-only loss over all rows in chunks of B"""
    import torch
    dev = torch.device("cuda")
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 16, 8, 4), torch.nn.ReLU(), torch.nn.Conv2d(16, 32, 4, 2), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(2048, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 6)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    x = torch.tensor(x_host.T.reshape(-1, 4, 80, 80).copy(), device=dev); act = torch.tensor(a_host, dtype=torch.long, device=dev)

    def sums(xs, ac):
        p = torch.softmax(net(xs * (1.0 / 255.0)), 1)
        return torch.log(p.gather(1, ac[:, None])[:, 0]).sum(), (p * torch.log(p + 1.1920929e-07)).sum()

    def step():
        opt.zero_grad(set_to_none=True); lp, nh = sums(x[:B], act[:B])
        loss = (-lp + 1e-3 * nh) / B; loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), float("inf")); opt.step(); return loss.item()

    def loss_pass():
        with torch.no_grad():
            tot = 0.0
            for r0 in range(0, x.shape[0], B):
                lp, nh = sums(x[r0:r0 + B], act[r0:r0 + B]); tot = tot + (-lp + 1e-3 * nh)
            return (tot / x.shape[0]).item()
    return step, loss_pass, torch.cuda.synchronize


def bc(a, crux, L):
    """--bc: crux_conv_bc_step and crux_conv_bc_loss over 1024 rows beside torch eager; Atari trunk, 2048-256-6 head"""
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines, ours, N = [], {}, 1024; vp = lambda v: v.ctypes.data_as(C.c_void_p); f = lambda t: "%.1f us (%.1f .. %.1f)" % tuple(t)      # noqa: E731
    x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, N)).astype(np.float32)); act = rng.integers(0, 6, N)
    d_x, d_a = ctx.alloc(x.nbytes), ctx.alloc(6 * N); ctx.h2d(d_x, x); ctx.h2d(d_a, np.asfortranarray(np.eye(6, dtype=np.uint8)[:, act]))
    for B in (32, 128):
        pi = crux.DiscreteNetwork(chain(32, 256), list(range(6)), seed=2, ctx=ctx); pi.attach_optimizer(crux.Adam(np.float32(1e-3)))
        h = (pi.trunk.h, pi.trunk.p.h, pi.head_h); raw, out = np.zeros(L.INFO_N, np.float32), np.zeros(3, np.float32)
        step = lambda: ctx.check(ctx.lib.crux_conv_bc_step(*h, d_x, d_a, 6, B, L.LOSS["logpdf_bc"], 1e-3, vp(raw)))                 # noqa: E731
        loss = lambda: ctx.check(ctx.lib.crux_conv_bc_loss(*h, d_x, d_a, 6, N, B, L.LOSS["logpdf_bc"], 1e-3, vp(out)))              # noqa: E731
        ours[B] = (median_window(step, ctx.sync, a.n, a.reps), median_window(loss, ctx.sync, max(a.n // 10, 1), a.reps))
    ctx.free(d_x); ctx.free(d_a); ctx.sync()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--bc", "--n", str(a.n), "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
    try:
        tor = json.loads(child.stdout.strip().splitlines()[-1])
    except Exception:      # noqa: BLE001
        tor = None; sys.stderr.write(child.stderr[-2000:])
    for B in (32, 128):
        for k, name, o in (("step", "crux_conv_bc_step (logpdf_bc_loss, 2048-256-6 head)", ours[B][0]), ("loss", "crux_conv_bc_loss over %d rows in chunks of %d" % (N, B), ours[B][1])):
            tt = "torch eager: not measured (the torch child process failed)" if tor is None else "torch eager %s; ratio torch / ours %.2f" % (f(tor["%s%d" % (k, B)]), tor["%s%d" % (k, B)][0] / o[0])
            lines.append("%s, B %3d: %s; %s" % (name, B, f(o), tt))
    txt = "# tools/conv_bench.py --bc: one MI355X, f32, median of %d windows of %d calls (%d for the loss pass) (min .. max), host clock around synchronised windows\n" % (a.reps, a.n, max(a.n // 10, 1)) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_bc_bench.txt"), "w").write(txt)


def pg(a, crux, L):
    """--pg: the paired trunk passes beside two single ones, and crux_conv_pg_step (PPO, actor + critic) beside two single-trunk steps and torch eager; Atari trunk, 2048-256 heads"""
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines, ours = [], {}
    for B in (32, 128):
        x = np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32))
        A = crux.DiscreteNetwork(chain(32, 256), list(range(6)), seed=2, ctx=ctx)
        V = crux.ContinuousNetwork(crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((8, 8), 4, 16, "relu", stride=4), crux.Conv((4, 4), 16, 32, "relu", stride=2), crux.flatten, crux.Dense(2048, 256, "relu"),
                                              crux.Dense(256, 1), input=(80, 80, 4)), seed=3, ctx=ctx)
        for q in (A, V):
            q.attach_optimizer(crux.Adam(np.float32(1e-3)))
        ta, tv, F = A.trunk, V.trunk, A.trunk.spec.out_features
        arrs = [x, np.asfortranarray(np.eye(6, dtype=np.uint8)[:, rng.integers(0, 6, B)]), rng.normal(0, 1, B).astype(np.float32), rng.normal(0, 1, B).astype(np.float32), np.full(B, -1.79, np.float32),
                np.ones((F, B), np.float32)]
        d = [ctx.alloc(v.nbytes) for v in arrs]
        for p, v in zip(d, arrs):
            ctx.h2d(p, v)
        d_x, d_a, d_adv, d_ret, d_lp, d_dy = d; raw, craw = np.zeros(L.INFO_N, np.float32), np.zeros(2, np.float32); vp = lambda v: v.ctypes.data_as(C.c_void_p)      # noqa: E731
        pair = lambda: (ctx.check(ctx.lib.crux_conv_forward_pair(ta.h, ta.p.h, tv.h, tv.p.h, d_x, B, None, None)),                                # noqa: E731
                        ctx.check(ctx.lib.crux_conv_backward_pair(ta.h, ta.p.h, tv.h, tv.p.h, d_x, B, d_dy, d_dy, 1.0, 1, None, None)))
        two = lambda: [(ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, None)), ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, d_dy, 1.0, 1, None))) for t in (ta, tv)]      # noqa: E731
        ha, hv, no = (ta.h, ta.p.h, A.head_h), (tv.h, tv.p.h, V.head_h), (None, None, None)
        call = lambda x1, x2, loss: ctx.check(ctx.lib.crux_conv_pg_step(*x1, *x2, d_x, d_a, d_adv, d_ret, d_lp, B, loss, 0.2, 1.0, 0.1, vp(raw), vp(craw)))      # noqa: E731
        step = lambda: call(ha, hv, L.LOSS["ppo"])                                                      # noqa: E731
        step2 = lambda: (call(ha, no, L.LOSS["ppo"]), call(no, hv, L.LOSS["value_mse"]))               # noqa: E731
        ours[B] = {k: median_window(f, ctx.sync, a.n, a.reps) for k, f in (("pair", pair), ("two", two), ("step", step), ("step2", step2))}
        for p in d:
            ctx.free(p)
    ctx.sync()
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--pg", "--n", str(a.n), "--reps", str(a.reps)], capture_output=True, text=True, timeout=300)
    try:
        tor = json.loads(child.stdout.strip().splitlines()[-1])
    except Exception:      # noqa: BLE001
        tor = None; sys.stderr.write(child.stderr[-2000:])
    for B in (32, 128):
        o = ours[B]; f = lambda t: "%.1f us (%.1f .. %.1f)" % t      # noqa: E731
        tt = ("torch eager: not measured (the torch child process failed)", "torch eager: not measured") if tor is None else tuple(
            "torch eager %s; ratio torch / ours %.2f" % (f(tuple(tor["%s%d" % (k, B)])), tor["%s%d" % (k, B)][0] / o[m][0]) for k, m in (("passes", "pair"), ("step", "step")))
        verdict = lambda p, s: "paired is faster" if p[2] < s[1] else ("paired is SLOWER than two single passes beyond the spread" if p[1] > s[2] else "inside the run-to-run spread")      # noqa: E731
        lines.append("two Atari trunks, forward + backward, B %3d: paired %s, two single passes %s, ratio two / paired %.2f (%s); %s" % (B, f(o["pair"]), f(o["two"]), o["two"][0] / o["pair"][0], verdict(o["pair"], o["two"]), tt[0]))
        lines.append("crux_conv_pg_step (ppo_loss + critic mse, 2048-256-6 and 2048-256-1 heads), B %3d: %s, as two single-trunk steps (actor, then critic: two synchronisations) %s, ratio %.2f; %s"
                     % (B, f(o["step"]), f(o["step2"]), o["step2"][0] / o["step"][0], tt[1]))
    txt = "# tools/conv_bench.py --pg: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_pg_bench.txt"), "w").write(txt)


def pg_gauss(a, crux, L):
    """--pg-gauss: crux_conv_pg_step_gauss (PPO, Gaussian actor with ad = 3, critic) beside crux_conv_pg_step with 3 categorical outputs; Atari trunk, 2048-256 heads"""
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines = []; ad = 3; vp = lambda v: v.ctypes.data_as(C.c_void_p); f = lambda t: "%.1f us (%.1f .. %.1f)" % t      # noqa: E731
    atari = lambda nout: crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((8, 8), 4, 16, "relu", stride=4), crux.Conv((4, 4), 16, 32, "relu", stride=2), crux.flatten, crux.Dense(2048, 256, "relu"),      # noqa: E731
                                    crux.Dense(256, nout), input=(80, 80, 4))
    for B in (32, 128):
        G = crux.GaussianPolicy(crux.ContinuousNetwork(atari(ad), seed=2, ctx=ctx), np.full(ad, -0.5, np.float32), seed=2, ctx=ctx)
        D = crux.DiscreteNetwork(atari(ad), list(range(ad)), seed=2, ctx=ctx); V = crux.ContinuousNetwork(atari(1), seed=3, ctx=ctx)
        for q in (G, D, V):
            q.attach_optimizer(crux.Adam(np.float32(1e-3)))
        arrs = [np.asfortranarray(rng.integers(0, 256, (80 * 80 * 4, B)).astype(np.float32)), np.asfortranarray(rng.normal(0, 1, (ad, B)).astype(np.float32)),
                np.asfortranarray(np.eye(ad, dtype=np.uint8)[:, rng.integers(0, ad, B)]), rng.normal(0, 1, B).astype(np.float32), rng.normal(0, 1, B).astype(np.float32), np.full(B, -1.79, np.float32)]
        d = [ctx.alloc(v.nbytes) for v in arrs]
        for p, v in zip(d, arrs):
            ctx.h2d(p, v)
        d_x, d_af, d_a8, d_adv, d_ret, d_lp = d; raw, craw = np.zeros(L.INFO_N, np.float32), np.zeros(2, np.float32)
        hv = (V.trunk.h, V.trunk.p.h, V.head_h)
        gauss = lambda: ctx.check(ctx.lib.crux_conv_pg_step_gauss(G.trunk.h, G.trunk.p.h, G.head_h, *hv, d_x, d_af, ad, d_adv, d_ret, d_lp, B, L.LOSS["ppo"], 0.2, 1.0, 0.1, vp(raw), vp(craw)))      # noqa: E731
        cat = lambda: ctx.check(ctx.lib.crux_conv_pg_step(D.trunk.h, D.trunk.p.h, D.head_h, *hv, d_x, d_a8, d_adv, d_ret, d_lp, B, L.LOSS["ppo"], 0.2, 1.0, 0.1, vp(raw), vp(craw)))      # noqa: E731
        g, c = median_window(gauss, ctx.sync, a.n, a.reps), median_window(cat, ctx.sync, a.n, a.reps)
        verdict = "the Gaussian step is faster" if g[2] < c[1] else ("the Gaussian step is SLOWER beyond the spread of these windows" if g[1] > c[2] else "inside the run-to-run spread")
        lines.append("PPO step, actor + critic, 2048-256-3 and 2048-256-1 heads, B %3d: crux_conv_pg_step_gauss (ad 3) %s, crux_conv_pg_step (3 categorical outputs) %s, ratio gauss / categorical %.3f (%s)"
                     % (B, f(g), f(c), g[0] / c[0], verdict))
        for p in d:
            ctx.free(p)
    txt = "# tools/conv_bench.py --pg-gauss: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_gauss_bench.txt"), "w").write(txt)


def ensemble(a, crux, L):
    ctx = crux.default_context(); rng = np.random.default_rng(0); lines = []; vp = lambda v: v.ctypes.data_as(C.c_void_p); f = lambda t: "%.1f us (%.1f .. %.1f)" % t      # noqa: E731
    arr = lambda hs: (C.c_void_p * len(hs))(*[getattr(h, "value", h) for h in hs])      # noqa: E731
    small = lambda: crux.Chain(crux.Conv((4, 4), 2, 8, "relu", stride=2), crux.Conv((3, 3), 8, 12, "tanh"), crux.flatten, crux.Dense(300, 64, "relu"), crux.Dense(64, 10), input=(16, 16, 2))      # noqa: E731
    atari = lambda: crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((8, 8), 4, 16, "relu", stride=4), crux.Conv((4, 4), 16, 32, "relu", stride=2), crux.flatten, crux.Dense(2048, 1024, "relu"),      # noqa: E731
                               crux.Dense(1024, 10), input=(80, 80, 4))
    for name, gen, nx, F, step_ok in (("16x16x2 -> 8@4/2 -> 12@3/1, head 300-64-10", small, 512, 300, True), ("Atari trunk, head 2048-1024-10", atari, 25600, 2048, False)):
        for M in (5, 16):
            nets = [crux.ContinuousNetwork(gen(), seed=1, stream=m, ctx=ctx) for m in range(M)]
            for q in nets:
                q.attach_optimizer(crux.Adam(np.float32(1e-3)))
            hs = (arr([q.trunk.h for q in nets]), arr([q.trunk.p.h for q in nets]), arr([q.head_h for q in nets]))
            for B in (32, 128):
                host = [rng.integers(0, 2, (nx, B)).astype(np.float32), np.asfortranarray(np.eye(10, dtype=np.float32)[:, rng.integers(0, 10, B)]), np.full((10, B), 0.01, np.float32)]
                d_x, d_y, d_dy = [ctx.alloc(v.nbytes) for v in host]
                for p, v in zip((d_x, d_y, d_dy), host):
                    ctx.h2d(p, v)
                d_f, d_df = [ctx.alloc(4 * F * B) for _ in range(M)], [ctx.alloc(4 * F * B) for _ in range(M)]; raw = np.zeros(L.INFO_N + 2 * M, np.float32)
                nul, dys, dfs = arr([None] * M), arr([d_dy] * M), arr(d_df)
                grouped = lambda: ctx.check(ctx.lib.crux_conv_ensemble_passes(*hs, M, d_x, B, dys, nul, dfs))      # noqa: E731

                def single(adam=False):
                    for q, pf, pd in zip(nets, d_f, d_df):
                        t = q.trunk
                        ctx.check(ctx.lib.crux_conv_forward_cached(t.h, t.p.h, d_x, B, pf)); ctx.check(ctx.lib.crux_mlp_forward_cached(q.head_h, pf, B, None))
                        ctx.check(ctx.lib.crux_mlp_backward(q.head_h, pf, B, d_dy, 1.0, 1, pd)); ctx.check(ctx.lib.crux_conv_backward(t.h, t.p.h, d_x, B, pd, 1.0, 1, None))
                        if adam:
                            ctx.check(ctx.lib.crux_adam_apply(t.p.h, 1.0)); ctx.check(ctx.lib.crux_adam_apply(q.head_h, 1.0))
                g, o = median_window(grouped, ctx.sync, a.n, a.reps), median_window(single, ctx.sync, a.n, a.reps)
                lines.append("%s, M %2d, B %3d: passes grouped %s, member by member (with a device copy of each member's features, which the head's entry reads from a caller's buffer) %s, ratio %.2f" % (name, M, B, f(g), f(o), o[0] / g[0]))
                if step_ok:
                    step = lambda: ctx.check(ctx.lib.crux_conv_ensemble_step(*hs, M, L.ENS["class"], d_x, d_y, None, B, vp(raw)))      # noqa: E731
                    g, o = median_window(step, ctx.sync, a.n, a.reps), median_window(lambda: single(True), ctx.sync, a.n, a.reps)
                    lines.append("%s, M %2d, B %3d: crux_conv_ensemble_step %s, member-by-member passes + crux_adam_apply per handle (no loss head, norms or gate) %s, ratio %.2f" % (name, M, B, f(g), f(o), o[0] / g[0]))
                else:
                    lines.append("%s, M %2d, B %3d: crux_conv_ensemble_step not measured (a 2048-wide head is a wide handle, which the step refuses)" % (name, M, B))
                for p in [d_x, d_y, d_dy] + d_f + d_df:
                    ctx.free(p)
    txt = "# tools/conv_bench.py --ensemble: one MI355X, f32, median of %d windows of %d calls (min .. max), host clock around synchronised windows\n" % (a.reps, a.n) + "\n".join(lines) + "\n"
    print(txt)
    if a.save:
        open(os.path.join(ROOT, "profiles", "conv_ensemble_bench.txt"), "w").write(txt)


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--n", type=int, default=200); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--save", action="store_true")
    ap.add_argument("--torch-child", action="store_true"); ap.add_argument("--atari", action="store_true"); ap.add_argument("--pg", action="store_true"); ap.add_argument("--pg-gauss", action="store_true"); ap.add_argument("--ensemble", action="store_true"); ap.add_argument("--pool", action="store_true"); ap.add_argument("--bc", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a)
    global crux
    import crux_jl_amd as crux
    from crux_jl_amd import _lib as L
    if a.atari:
        return atari(a, crux, L)
    if a.pg:
        return pg(a, crux, L)
    if a.pg_gauss:
        return pg_gauss(a, crux, L)
    if a.ensemble:
        return ensemble(a, crux, L)
    if a.pool:
        return pool(a, crux, L)
    if a.bc:
        return bc(a, crux, L)
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
