#!/usr/bin/env python
"""SAC on Pendulum-v1 with the actor the reference's SAC examples build (examples/rl/pendulum.jl, half_cheetah_mujoco.jl:37-43): a SquashedGaussianPolicy with ascale = 2
whose logSigma is a network sharing its 3-64-64 trunk with mu,

    base = Chain(Dense(3, 64, relu), Dense(64, 64, relu));  mu = Chain(base..., Dense(64, 1));  logSigma = Chain(base..., Dense(64, 1))

--actor constant runs examples/sac_pendulum.py's actor (unsquashed, constant logSigma) under the same budget and evaluation, for a learning curve beside it.
The solve is cut into --chunks pieces; after each the greedy policy's undiscounted return over 10 episodes is printed (chunk 0 = the untrained policy)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--N", type=int, default=4000); ap.add_argument("--width", type=int, default=64); ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--actor", choices=["squashed", "constant"], default="squashed"); a = ap.parse_args()
    mdp = crux.PendulumMDP(n_envs=1, seed=0)
    S = mdp.state_space()
    w = a.width
    if a.actor == "squashed":
        base = [crux.Dense(3, w, "relu"), crux.Dense(w, w, "relu")]
        G = crux.SquashedGaussianPolicy(crux.Chain(*base, crux.Dense(w, 1)), crux.Chain(*base, crux.Dense(w, 1)), 2.0, seed=1)
    else:
        G = crux.GaussianPolicy(crux.Chain(crux.Dense(3, w, "relu"), crux.Dense(w, w, "relu"), crux.Dense(w, 1)), np.zeros(1, np.float32), seed=1)
    QSA = lambda s: crux.ContinuousNetwork(crux.Chain(crux.Dense(4, w, "relu"), crux.Dense(w, w, "relu"), crux.Dense(w, 1)), seed=s)
    opt = {"batch_size": 100, "optimizer": crux.Adam(np.float32(1e-3))}
    fill = 1000                                                  # buffer_init: the first solve spends it on filling the replay buffer before it trains (off_policy.jl:122-126)
    n = max(50, (a.N - fill) // a.chunks // 50 * 50)
    solver = crux.SAC(crux.ActorCritic(G, crux.DoubleNetwork(QSA(2), QSA(3))), S, N=fill + n, dN=50, c_opt=dict(opt), a_opt=dict(opt), SAC_alpha_opt=dict(opt),
                      buffer_size=100000, buffer_init=fill, max_steps=200, pi_explore=crux.GaussianNoiseExplorationPolicy(0.5, a_min=-2.0, a_max=2.0))
    evaluate = lambda: crux.undiscounted_return(crux.Sampler(mdp, crux.PolicyParams(solver.agent.pi), max_steps=200), Neps=10)
    print("%s actor: steps %6d  undiscounted return %8.1f  (untrained)" % (a.actor, 0, evaluate()))
    for k in range(a.chunks):
        crux.solve(solver, mdp)
        solver.N = n                                             # the next call continues from solver.i for n more interactions
        h = solver.history[-1]
        print("%s actor: steps %6d  undiscounted return %8.1f  critic_loss %.4f  actor_loss %.4f  alpha %.4f  entropy %.3f"
              % (a.actor, solver.i, evaluate(), h["critic_loss"], h["actor_loss"], h["SAC alpha"], h["entropy"]))


if __name__ == "__main__":
    main()
