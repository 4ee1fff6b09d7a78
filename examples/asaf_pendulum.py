#!/usr/bin/env python
"""ASAF on Pendulum after the reference's imitation benchmark (examples/il/pendulum.jl:102-110): SquashedGaussianPolicy(2 -> 64 -> 64 -> 1 relu, logSigma 0, ascale 2),
dN = 2000, minibatches of 256, 10 epochs per iteration, Optimiser(ClipValue(1), Adam(1e-3)), max_steps = 100, on the committed Pendulum demonstrations
(tests/golden/pendulum_transitions.npz; the state space whitened by their statistics, + 1e-3 on sigma as in the example). 70 % of the rows are the demonstrations, 30 %
are held out; the held-out mean logpdf(pi, s_E, a_E) is printed before and after. The demonstrations store the reference's (theta, thetadot) states while the library's
Pendulum observes (cos, sin, thetadot), so the rollouts come from the two-observation SYNTH dynamics (SynthMDP(2, 1))."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux


def buffer(d, ids, S, A):
    b = crux.ExperienceBuffer(S, A, len(ids))
    b.push_({k: np.ascontiguousarray(d[k][:, ids]) for k in ("s", "a", "sp", "r", "done")}); return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=50000); ap.add_argument("--dN", type=int, default=2000); ap.add_argument("--n_envs", type=int, default=20)
    a = ap.parse_args()
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "pendulum_transitions.npz")))
    od, ad, n = d["s"].shape[0], d["a"].shape[0], d["s"].shape[1]
    S = crux.ContinuousSpace(od, mu=d["s"].mean(1).astype(np.float32), sigma=(d["s"].std(1) + 1e-3).astype(np.float32)); A = crux.ContinuousSpace(ad)
    order = np.random.default_rng(0).permutation(n); cut = int(round(0.7 * n))
    demo, held = buffer(d, order[:cut], S, A), crux.normalize_(buffer(d, order[cut:], S, A), S, A)
    pi = crux.SquashedGaussianPolicy(crux.Chain(crux.Dense(od, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, ad)), np.zeros(ad, np.float32), 2.0, seed=1)
    out = crux.il_on_policy._DeviceVec(pi.ctx, len(held))

    def score():
        crux.asaf_freeze_(pi, held, out.p); return float(np.mean(out.get().astype(np.float64)))
    mdp = crux.SynthMDP(od, ad, n_envs=a.n_envs, seed=0)
    sv = crux.ASAF(pi, S, demo, dN=a.dN, N=a.N, max_steps=100, clip_value=1.0, a_opt={"batch_size": 256, "epochs": 10, "optimizer": crux.Adam(np.float32(1e-3))})
    print("demonstrations: %d rows, %d held out; %d iterations of %d steps" % (cut, n - cut, a.N // a.dN, a.dN))
    before = score()
    crux.solve(sv, mdp)
    h = sv.history[-1]
    print("ASAF  held-out mean logpdf %.4f -> %.4f   last iteration: actor_loss %.4f  actor_grad_norm %.4f  entropy %.4f  batches %d"
          % (before, score(), h["actor_loss"], h["actor_grad_norm"], h["entropy"], h["actor_batches_trained"]))


if __name__ == "__main__":
    main()
