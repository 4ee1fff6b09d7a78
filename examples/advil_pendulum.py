#!/usr/bin/env python
"""AdVIL on the committed Pendulum demonstrations (tests/golden/pendulum_transitions.npz) -- the reference's AdVIL constructor (src/model_free/il/AdVIL.jl) on a small
task, next to BC from the same initialisation: 70 % of the rows train, 30 % are held out, and the held-out mean((pi(s) - a)^2) is printed before and after."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux


def actor(w, od, ad):
    return crux.ContinuousNetwork(crux.Chain(crux.Dense(od, w, "tanh"), crux.Dense(w, w, "tanh"), crux.Dense(w, ad)), seed=1)


def buffer(d, ids, S, A):
    b = crux.ExperienceBuffer(S, A, len(ids))
    b.push_({k: np.ascontiguousarray(d[k][:, ids]) for k in ("s", "a", "sp", "r", "done")}); return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=60); ap.add_argument("--width", type=int, default=64); ap.add_argument("--batch_size", type=int, default=128)
    a = ap.parse_args()
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "pendulum_transitions.npz")))
    od, ad, n = d["s"].shape[0], d["a"].shape[0], d["s"].shape[1]
    S = crux.ContinuousSpace(od, mu=d["s"].mean(1).astype(np.float32), sigma=d["s"].std(1).astype(np.float32)); A = crux.ContinuousSpace(ad)
    order = np.random.default_rng(0).permutation(n); cut = int(round(0.7 * n))
    demo, held = buffer(d, order[:cut], S, A), crux.normalize_(buffer(d, order[cut:], S, A), S, A)
    err = lambda pi: float(np.mean((pi.forward(held["s"]).astype(np.float64) - held["a"]) ** 2))      # noqa: E731
    print("demonstrations: %d rows to train on, %d held out" % (cut, n - cut))

    pi = crux.ActorCritic(actor(a.width, od, ad), crux.ContinuousNetwork(crux.Chain(crux.Dense(od + ad, a.width, "tanh"), crux.Dense(a.width, a.width, "tanh"), crux.Dense(a.width, 1)), seed=2))
    before = err(pi.A)
    sv = crux.AdVIL(pi, S, demo, a_opt={"epochs": a.epochs, "batch_size": a.batch_size})
    crux.solve(sv)
    h = sv.history[-1]
    print("AdVIL  held-out bc mse %.4f -> %.4f   D_expert %.4f  D_policy %.4f  grad_pen %.5f  orth_reg %.6f" % (before, err(pi.A), h["D_expert"], h["D_policy"], h["grad_pen"], h["orth_reg"]))

    bc_pi = actor(a.width, od, ad)
    bc = crux.BC(bc_pi, S, demo, opt={"epochs": a.epochs, "batch_size": a.batch_size}, window=10**6)
    crux.solve(bc)
    print("BC     held-out bc mse %.4f -> %.4f" % (before, err(bc_pi)))


if __name__ == "__main__":
    main()
