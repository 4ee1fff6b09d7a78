"""us per minibatch of the two-headed Gaussian learner (ppo_loss on a handle whose last layer is [mu; logSigma(s)]: csrc/train_dense.hip, k_pg_head_sigma) against the
constant-logSigma learner of the same trunk on the same build. At the minibatch sizes below the library runs the constant form on the dense-engine chain too (k_pg_head),
so the two sides differ in the head kernel and in the last layer's rows; the window holds the chain's per-epoch host synchronisation on both sides.

    python tools/sigma_pg_bench.py > profiles/sigma_pg_bench.txt

Per shape: a buffer of 8 minibatches of synthetic columns (actions drawn from the policy, old logprob = logpdf + N(0, 0.05), advantages N(0, 1)); 2 warm-up calls of
crux_batch_train per side, then 7 repeats of one call of 4 epochs (32 minibatches) per side, the two sides alternating within a repeat. The time is the library's own HIP-event
pair around the learner launches on the context's stream (crux_prof, slot train_actor): it excludes the epoch orders composed before the launch and the buffer permutation
after it, which both sides share. lr = 1e-5 and lambda_e = 0, so the steps do not drive either policy away from its buffer. Median and (min .. max) of the repeats are
reported. Nothing is promised: the constant form is the yardstick, and the file says what was found. A measurement path that finds no GPU fails."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux  # noqa: E402
from crux_jl_amd import _lib as L  # noqa: E402

# (trunk dims, act_dim, batch_size): at these minibatch sizes both forms run the dense-engine chain, so the difference is the head kernel and the last layer's rows
SHAPES = [((3, 64, 64), 1, 512), ((17, 256, 256), 6, 256), ((17, 256, 256), 6, 4000)]
WARM, REPS, EPOCHS, NMB = 2, 7, 4, 8


def actor(ctx, trunk, ad, two):
    base = [crux.Dense(trunk[i], trunk[i + 1], "relu") for i in range(len(trunk) - 1)]
    if two:
        pi = crux.GaussianPolicy(crux.Chain(*base, crux.Dense(trunk[-1], ad)), crux.Chain(*base, crux.Dense(trunk[-1], ad)), ctx=ctx, seed=1)
        p = pi.get_params(); p[-ad:] = -0.5; pi.set_params(p)      # logSigma's bias: the constant form's log-std
    else:
        pi = crux.GaussianPolicy(crux.Chain(*base, crux.Dense(trunk[-1], ad)), np.full(ad, -0.5, np.float32), ctx=ctx, seed=1)
    pi.attach_optimizer(crux.Adam(np.float32(1e-5))); return pi


def buffer(ctx, pi, od, ad, n, rng, two):
    s = np.asfortranarray(rng.normal(0, 1, (od, n)).astype(np.float32))
    if two:
        a, lp = pi.exploration(s, 5, 0)
    else:      # the constant form has no host exploration method: mu(s) + sigma eps and its log-density written out
        mu = pi.forward(s); eps = rng.normal(0, 1, (ad, n)).astype(np.float32); sg = np.float32(np.exp(-0.5)); a = (mu + sg * eps).astype(np.float32)
        lp = (-(eps * eps) / 2 - np.float32(0.9189385332046727) + 0.5).sum(0, keepdims=True).astype(np.float32)
    b = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.ContinuousSpace(ad), n, ["return", "logprob", "advantage"], ctx=ctx)
    b.push_({"s": s, "a": np.asfortranarray(a), "sp": s, "r": np.zeros((1, n), np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool),
             "return": rng.normal(0, 1, (1, n)).astype(np.float32), "logprob": (lp + rng.normal(0, 0.05, (1, n))).astype(np.float32), "advantage": rng.normal(0, 1, (1, n)).astype(np.float32)})
    return b


def main():
    ctx = crux.default_context(); lib = ctx.lib; rng = np.random.default_rng(0); ctx.prof_enable(True)
    print("ppo_loss learner, us per minibatch by HIP events around the learner launches: %d warm-up calls + %d x %d minibatches per side (alternating): median (min .. max)" % (WARM, REPS, EPOCHS * NMB))
    for trunk, ad, bs in SHAPES:
        od, n = trunk[0], NMB * bs; sides = {}
        for two in (True, False):
            pi = actor(ctx, trunk, ad, two); sides[two] = (pi, buffer(ctx, pi, od, ad, n, rng, two))
        cfg = L.TrainCfg(); cfg.loss, cfg.head, cfg.batch_size, cfg.epochs, cfg.max_batches = L.LOSS["ppo"], L.HEAD["gaussian"], bs, EPOCHS, 0
        cfg.eps_clip, cfg.lambda_p, cfg.lambda_e, cfg.target_kl, cfg.shuffle_seed, cfg.shuffle_counter = 0.2, 1.0, 0.0, -1.0, 3, 0
        info = np.zeros(L.INFO_N, np.float32)

        def call(two):
            pi, b = sides[two]; ctx.prof_reset()
            ctx.check(lib.crux_batch_train(pi.h, b.h, C.byref(cfg), None, info.ctypes.data_as(C.c_void_p), None)); ctx.sync()
            ms, k = ctx.prof_get(L.PROF["train_actor"]); nb = int(info[L.INFO["batches_trained"]])
            assert k >= 1 and nb == EPOCHS * NMB and np.isfinite(info[:2]).all(), (k, nb, info)
            return 1e3 * ms / nb
        for _ in range(WARM):
            call(True); call(False)
        t = {True: [], False: []}
        for _ in range(REPS):
            for two in (True, False):
                t[two].append(call(two))
        tag = "%-10s x%d bs %4d" % ("-".join(map(str, trunk)), ad, bs)
        for two, name in ((True, "two-headed  (2 x %d output rows)" % ad), (False, "constant logSigma (%d rows + %d extras)" % (ad, ad))):
            print("%s  %-40s %8.1f (%.1f .. %.1f)" % (tag, name, np.median(t[two]), min(t[two]), max(t[two])))
        print("%s  ratio two-headed / constant %.2f" % (tag, np.median(t[True]) / np.median(t[False])))


if __name__ == "__main__":
    main()
