#!/usr/bin/env python
"""IQ-Learn on CartPole from demonstrations -- the reference's examples/il/cartpole.jl (OnlineIQLearn: N=10000, dN=1, c_opt epochs=1, reg=false, gp=false),
on the 512 demonstration rows committed under tests/golden/ (a slice of the reference's examples/il/expert_data/cartpole.bson)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--N", type=int, default=10000); ap.add_argument("--gp", action="store_true"); a = ap.parse_args()
    mdp = crux.CartPoleMDP(n_envs=1, seed=0)
    S = mdp.state_space()
    d = np.load(os.path.join(ROOT, "tests", "golden", "cartpole_transitions.npz"))
    demo = crux.ExperienceBuffer(S, crux.DiscreteSpace(2), d["s"].shape[1])
    demo.push_({k: d[k] for k in ("s", "a", "sp", "r", "done")})
    Q = crux.DiscreteNetwork(crux.Chain(crux.Dense(4, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 2)), [1, 2], seed=0)
    solver = crux.OnlineIQLearn(Q, S, demo, gamma=np.float32(mdp.discount), N=a.N, dN=1, c_opt={"epochs": 1}, reg=False, gp=a.gp, max_steps=200, buffer_size=a.N)
    crux.solve(solver, mdp)
    h = solver.history[-1]
    print("iterations %d  last critic_loss %.4f  avg_R_expert_IQ %.4f" % (len(solver.history), h["critic_loss"], h["avg_R_expert_IQ"]))
    greedy = crux.DiscreteNetwork(Q.network, Q.outputs); crux.copyto_(greedy, Q)
    print("greedy evaluation: undiscounted return %.1f" % crux.undiscounted_return(crux.Sampler(crux.CartPoleMDP(n_envs=1, seed=5), greedy, max_steps=200), Neps=20))


if __name__ == "__main__":
    main()
