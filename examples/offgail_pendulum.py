#!/usr/bin/env python
"""Off-policy imitation on Pendulum -- the pattern of the reference's examples/il/pendulum.jl: an expert (a short SAC run), its transitions as demonstrations,
then OffPolicyGAIL and AdRIL from the same initialisation. Prints the learning curve of each learner: the undiscounted return of the greedy policy (fixed
evaluation seed) after every `--chunk` environment steps. The discriminator is a plain ContinuousNetwork with two outputs; `--sn` builds it from three
DenseSN layers instead, like the reference example's spectrally normalised D_SN."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux


def nets(w, seed=1):
    mlp = lambda i, o: crux.Chain(crux.Dense(i, w, "relu"), crux.Dense(w, w, "relu"), crux.Dense(w, o))                               # noqa: E731
    return crux.ActorCritic(crux.GaussianPolicy(mlp(3, 1), np.zeros(1, np.float32), seed=seed),
                            crux.DoubleNetwork(crux.ContinuousNetwork(mlp(4, 1), seed=seed + 1), crux.ContinuousNetwork(mlp(4, 1), seed=seed + 2)))


def evaluate(pi):
    return crux.undiscounted_return(crux.Sampler(crux.PendulumMDP(n_envs=1, seed=100), crux.PolicyParams(pi.A), max_steps=200), Neps=5)


def curve(name, sv, mdp, pi, total, chunk):
    print("%-14s steps %6d  return %8.1f" % (name, 0, evaluate(pi)))
    for done in range(chunk, total + 1, chunk):
        crux.solve(sv, mdp)
        h = sv.history[-1]
        extra = "  discriminator_loss %.4f" % h["discriminator_loss"] if "discriminator_loss" in h else ""
        print("%-14s steps %6d  return %8.1f  critic_loss %.4f%s" % (name, done, evaluate(pi), h["critic_loss"], extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expert_steps", type=int, default=10000); ap.add_argument("--steps", type=int, default=10000); ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--n_demo", type=int, default=2000); ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--sn", action="store_true", help="spectrally normalised discriminator (DenseSN, DenseSN, DenseSN)")
    a = ap.parse_args()
    mdp = crux.PendulumMDP(n_envs=1, seed=0)
    S, A = mdp.state_space(), crux.ContinuousSpace(1)
    opt = lambda: {"batch_size": 128, "optimizer": crux.Adam(np.float32(1e-3))}                                                        # noqa: E731
    kw = lambda: dict(dN=50, max_steps=200, buffer_size=100000, c_opt=opt(), a_opt=opt(), SAC_alpha_opt=opt())                         # noqa: E731

    expert = nets(a.width)
    sv = crux.SAC(expert, S, N=a.chunk, buffer_init=1000, **kw())
    curve("expert (SAC)", sv, mdp, expert, a.expert_steps, a.chunk)
    demo = crux.ExperienceBuffer(S, A, a.n_demo)
    crux.steps_(crux.Sampler(mdp, crux.PolicyParams(expert.A), max_steps=200), demo, Nsteps=a.n_demo, explore=False)
    print("demonstrations: %d transitions, mean reward %.3f" % (len(demo), float(demo["r"].mean())))

    pi = nets(a.width)
    lay = crux.DenseSN if a.sn else crux.Dense
    D = crux.ContinuousNetwork(crux.Chain(lay(4, a.width, "relu"), lay(a.width, a.width, "relu"), lay(a.width, 2)), seed=7)
    gail = crux.OffPolicyGAIL(pi, S, demo, D, N=a.chunk, buffer_init=1000, d_opt={"epochs": 5, "batch_size": 128, "optimizer": crux.Adam(np.float32(3e-4))}, **kw())
    curve("OffPolicyGAIL", gail, mdp, pi, a.steps, a.chunk)

    pi = nets(a.width)
    k = kw(); k.pop("dN")
    adril = crux.AdRIL(pi, S, demo, dN=50, N=a.chunk, **k)
    curve("AdRIL", adril, mdp, pi, a.steps, a.chunk)


if __name__ == "__main__":
    main()
