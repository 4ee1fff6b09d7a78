#!/usr/bin/env python
"""PPO on Pendulum-v1 with a two-headed actor: a SquashedGaussianPolicy with ascale = 2 whose logSigma is a network sharing its 3-64-64 trunk with mu (the actor of
examples/sac_squashed_pendulum.py, the reference's idiom of examples/rl/half_cheetah_mujoco.jl:37-43),

    base = Chain(Dense(3, 64, relu), Dense(64, 64, relu));  mu = Chain(base..., Dense(64, 1));  logSigma = Chain(base..., Dense(64, 1))

trained by ppo_loss under the settings of the reference's Pendulum PPO example (examples/rl/pendulum.jl:32: dN = 2048, actor batch_size 512, lambda_e = 0, everything else
the defaults: 80 epochs with the 0.012 KL early stop, Adam(3f-4), 100-step episodes) on the dense-engine learner (csrc/train_dense.hip: k_pg_head_sigma).
--actor constant runs the reference's own actor there, the constant-logSigma SquashedGaussianPolicy of the same trunk, under the same budget and evaluation, for a learning curve beside it.
The solve is cut into --chunks pieces; after each the greedy policy's undiscounted return over 10 episodes is printed (chunk 0 = the untrained policy)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--N", type=int, default=98304); ap.add_argument("--dN", type=int, default=2048); ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--actor", choices=["two-headed", "constant"], default="two-headed"); a = ap.parse_args()
    mdp = crux.PendulumMDP(n_envs=8, seed=0)
    S = mdp.state_space()
    if a.actor == "two-headed":
        base = [crux.Dense(3, 64, "relu"), crux.Dense(64, 64, "relu")]
        G = crux.SquashedGaussianPolicy(crux.Chain(*base, crux.Dense(64, 1)), crux.Chain(*base, crux.Dense(64, 1)), 2.0, seed=1)
    else:
        G = crux.SquashedGaussianPolicy(crux.Chain(crux.Dense(3, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 1)), np.zeros(1, np.float32), 2.0, seed=1)      # the reference's SG()
    V = crux.ContinuousNetwork(crux.Chain(crux.Dense(3, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 1)), seed=2)
    n = max(a.dN, a.N // a.chunks // a.dN * a.dN)
    solver = crux.PPO(crux.ActorCritic(G, V), S, N=n, dN=a.dN, max_steps=100, lambda_e=0.0, a_opt={"batch_size": 512}, two_headed=a.actor == "two-headed")
    evaluate = lambda: crux.undiscounted_return(crux.Sampler(mdp, crux.PolicyParams(solver.agent.pi), max_steps=100), Neps=10)      # noqa: E731
    print("%s actor: steps %6d  undiscounted return %8.1f  (untrained)" % (a.actor, 0, evaluate()))
    for k in range(a.chunks):
        crux.solve(solver, mdp)
        h = solver.history[-1]
        print("%s actor: steps %6d  undiscounted return %8.1f  actor_loss %.4f  critic_loss %.4f  kl %.4f  clip_fraction %.3f  entropy %.3f"
              % (a.actor, solver.i, evaluate(), h["actor_loss"], h["critic_loss"], h["kl"], h["clip_fraction"], h["entropy"]))


if __name__ == "__main__":
    main()
