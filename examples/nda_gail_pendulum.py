#!/usr/bin/env python
"""NDA-GAIL-JS on Pendulum (src/model_free/il/nda_gail_js.jl): LagrangePPO whose rewards come from a discriminator D trained on the committed Pendulum demonstrations
(tests/golden/pendulum_transitions.npz) and whose costs come from a second discriminator Dnda trained on negative demonstrations, c = max(0, r_nda - r).

Negative demonstrations, the rule: the same recorded states with the action mirrored, a -> -a (the torque that pushes the pendulum the wrong way); nothing else of a row
changes. The recording stores (theta, thetadot) while the library's Pendulum observes (cos, sin, thetadot): the states are mapped to observations first.

ActorCritic(GaussianPolicy(3 -> 64 -> 64 -> 1 relu, logSigma 0), critic 3 -> 64 -> 64 -> 1), Vc of the critic's shape, D and Dnda 4 -> 64 -> 64 -> 1; dN = 1024 steps from
8 environments per iteration, every learner 4 epochs of minibatches of 256. The callback of every iteration is one C call (crux_nda_gail_round).
--gan-loss picks the discriminators' loss from GANLosses (src/extras/gans.jl): BCE (the default), LS, Hinge and W keep the one-call round; WGP (Wasserstein + gradient
penalty) runs the round's parts in turn with a host loop of discriminator steps -- 512 demonstration rows and 1024 rollout rows under minibatches of 256 give equal halves.
lagrange_ppo_loss estimates the episode cost from EVERY minibatch (sum(cost) / sum(episode_end), ppo.jl:86), which needs episode ends in every minibatch: episodes of
16 steps put 64 of them into the 1024 rows."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux


def net(dims, seed):
    return crux.Chain(*[crux.Dense(i, o, "relu" if k < len(dims) - 2 else "identity") for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]), seed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=20 * 1024); ap.add_argument("--dN", type=int, default=1024); ap.add_argument("--n_envs", type=int, default=8)
    ap.add_argument("--gan-loss", choices=list(crux.GANLosses), default="BCE")
    a = ap.parse_args()
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "pendulum_transitions.npz")))
    n = d["s"].shape[1]; S, A = crux.ContinuousSpace(3), crux.ContinuousSpace(1)
    obs3 = lambda x: np.vstack([np.cos(x[0]), np.sin(x[0]), x[1]]).astype(np.float32)
    rows = {"s": obs3(d["s"]), "sp": obs3(d["sp"]), "a": d["a"], "r": d["r"], "done": d["done"], "episode_end": np.zeros((1, n), bool)}
    demo = crux.ExperienceBuffer(S, A, n); demo.push_(rows)
    nda = crux.ExperienceBuffer(S, A, n); nda.push_(dict(rows, a=-d["a"]))      # the rule above
    ch, sd = net([3, 64, 64, 1], 1)
    pi = crux.ActorCritic(crux.GaussianPolicy(ch, np.zeros(1, np.float32), seed=sd), crux.ContinuousNetwork(net([3, 64, 64, 1], 2)[0], seed=2))
    Vc = crux.ContinuousNetwork(net([3, 64, 64, 1], 5)[0], seed=5)
    D, Dnda = crux.ContinuousNetwork(net([4, 64, 64, 1], 3)[0], seed=3), crux.ContinuousNetwork(net([4, 64, 64, 1], 4)[0], seed=4)
    opt = {"epochs": 4, "batch_size": 256}
    sv = crux.NDA_GAIL_JS(pi, S, demo, nda, Vc, 0.99, D, Dnda, N=a.N, dN=a.dN, max_steps=16, normalize_demo=False, a_opt=dict(opt), c_opt=dict(opt), cost_opt=dict(opt),
                          d_opt=dict(opt), d_opt_nda=dict(opt), gan_loss=crux.GANLosses[a.gan_loss])
    print("demonstrations: %d rows, as many negative ones; %d iterations of %d steps; discriminator loss %r" % (n, a.N // a.dN, a.dN, crux.GANLosses[a.gan_loss]))
    crux.solve(sv, crux.PendulumMDP(n_envs=a.n_envs, seed=0))
    for k in (0, len(sv.history) - 1):
        h = sv.history[k]
        print("iteration %3d  discriminator_loss %.4f  nda_discriminator_loss %.4f  disc_reward %.4f  disc_nda_cost %.4f  penalty %.4f" % (
            k + 1, h["discriminator_loss"], h["nda_discriminator_loss"], h["disc_reward"], h["disc_nda_cost"], h.get("penalty", float("nan"))))


if __name__ == "__main__":
    main()
