"""Does crux_batch_train equal the chain of crux_train_step calls over the same minibatches BIT FOR BIT? Measured for the constant-logSigma GaussianPolicy 3-64-64-1 (the
register-resident learners: the feature-split kernel for the batch, the one-CU kernel for single steps with ids) beside the two-headed 3-64-64-2x1 of the same trunk (both routes
are the dense-engine chain): 3 epochs of 300 rows at batch_size 128 (minibatches of 128, 128, 44), ppo_loss, lambda_e = 0, Adam(1e-2).
tests/test_gpu_sigma_pg.py::test_batch_train_equals_the_step_by_step_chain cites the result.

    python tools/sigma_pg_chain_probe.py > profiles/sigma_pg_chain_probe.txt

A measurement path that finds no GPU fails."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity  # noqa: E402
from parity import crux, L, O  # noqa: E402

N, BS, E, SEED = 300, 128, 3, 29
ACTS = ["relu", "relu", "identity"]


def vp(x):
    return x.ctypes.data_as(C.c_void_p)


def make(ctx, two, p0):
    if two:
        base = [crux.Dense(3, 64, "relu"), crux.Dense(64, 64, "relu")]
        pi = crux.GaussianPolicy(crux.Chain(*base, crux.Dense(64, 1)), crux.Chain(*base, crux.Dense(64, 1)), ctx=ctx, seed=3)
    else:
        pi = crux.GaussianPolicy(parity.chain([3, 64, 64, 1], ACTS), np.full(1, -0.3, np.float32), ctx=ctx, seed=3)
    p0 = pi.get_params() if p0 is None else p0
    pi.set_params(p0); pi.attach_optimizer(crux.Adam(np.float32(1e-2)))
    b = crux.ExperienceBuffer(crux.ContinuousSpace(3), crux.ContinuousSpace(1), N, ["return", "logprob", "advantage"], ctx=ctx); r = np.random.default_rng(2)
    b.push_({"s": r.normal(0, 1, (3, N)).astype(np.float32), "a": r.normal(0, 0.7, (1, N)).astype(np.float32), "sp": r.normal(0, 1, (3, N)).astype(np.float32),
             "r": np.zeros((1, N), np.float32), "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": r.normal(0, 1, (1, N)).astype(np.float32),
             "logprob": r.normal(-1.2, 0.3, (1, N)).astype(np.float32), "advantage": r.normal(0, 1, (1, N)).astype(np.float32)})
    return pi, b, p0


def orders():
    """the composed epoch orders of batch_train!: o_e[j] = o_(e-1)[perm_e[j]] (include/crux_rng.h)"""
    out, prev = [], np.arange(N)
    for e in range(E):
        perm = np.zeros(N, np.int64); O.lib().orc_perm(SEED, e, N, O.vpz(perm)); prev = prev[perm]; out.append(prev)
    return out


def main():
    ctx = crux.default_context(); raw = np.zeros(L.INFO_N, np.float32)
    for two, name in ((False, "constant-logSigma 3-64-64-1"), (True, "two-headed 3-64-64-2x1")):
        pi, b, p0 = make(ctx, two, None); cfg = parity.train_cfg("ppo", "gaussian", BS, E, seed=SEED, le=0.0)
        ctx.check(ctx.lib.crux_batch_train(pi.h, b.h, C.byref(cfg), None, vp(raw), None)); pa = pi.get_params(); nb = int(raw[L.INFO["batches_trained"]])
        pi, b, _ = make(ctx, two, p0)
        for o in orders():
            for q in range(0, N, BS):
                ids = np.ascontiguousarray(o[q:q + BS], np.int64); c1 = parity.train_cfg("ppo", "gaussian", len(ids), 1, le=0.0)
                ctx.check(ctx.lib.crux_train_step(pi.h, b.h, C.byref(c1), vp(ids), ids.size, vp(raw)))
        pb = pi.get_params()
        print("%-28s %d steps: crux_batch_train against the crux_train_step chain: same bits %s, largest difference %.3e (parameters moved by up to %.3e)"
              % (name, nb, np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), np.abs(pa - pb).max(), np.abs(pa - p0).max()))


if __name__ == "__main__":
    main()
