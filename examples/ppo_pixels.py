#!/usr/bin/env python
"""PPO from pixels on the environment of examples/dqn_pixels.py (Catch: a ball falls on a W x H grid, a paddle on the bottom row catches it, +1, or misses, -1; two stacked
frames of 0 / 255 pixel values). Actor and critic are separate chains of one shape, as in every ActorCritic of the reference's examples:
    A = Chain(Scale(1 / 255), Conv((3, 3), 2 => 8, relu), Conv((3, 3), 8 => 16, relu), flatten, Dense(., 64, relu), Dense(64, 3))      V = the same, ending in Dense(64, 1)
so every minibatch goes through both trunks in one launch per layer (csrc/conv_pair.hip). The environment lives on the host (a HostMDP). Writes the learning curve to
profiles/conv_pg_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "examples"))
import crux_jl_amd as crux  # noqa: E402
from dqn_pixels import Catch, greedy_return  # noqa: E402,F401


def _chain(W, H, hidden, nout):
    feats = (W - 4) * (H - 4) * 16
    return crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((3, 3), 2, 8, "relu"), crux.Conv((3, 3), 8, 16, "relu"), crux.flatten, crux.Dense(feats, hidden, "relu"), crux.Dense(hidden, nout),
                      input=(W, H, 2))


def actor_critic(W, H, seed=0, hidden=64, ctx=None):
    kw = {"ctx": ctx} if ctx is not None else {}
    return crux.ActorCritic(crux.DiscreteNetwork(_chain(W, H, hidden, 3), [0, 1, 2], seed=seed, **kw), crux.ContinuousNetwork(_chain(W, H, hidden, 1), seed=seed + 1, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=8); ap.add_argument("--H", type=int, default=8); ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--dN", type=int, default=512); ap.add_argument("--envs", type=int, default=8); ap.add_argument("--chunk", type=int, default=2048); ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    env = Catch(a.W, a.H, seed=0); mdp = env.mdp(n_envs=a.envs)
    pi = actor_critic(a.W, a.H)
    opt = lambda: {"batch_size": 128, "epochs": 4, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    solver = crux.PPO(pi, crux.ContinuousSpace((a.W, a.H, 2)), N=a.chunk, dN=a.dN, max_steps=a.H, lambda_e=0.01, a_opt=opt(), c_opt=opt())
    lines = ["# examples/ppo_pixels.py: PPO, Catch %d x %d x 2, actor and critic Scale(1/255) -> Conv((3,3),2=>8,relu) -> Conv((3,3),8=>16,relu) -> flatten -> Dense(%d,64,relu) -> Dense(64, 3 | 1)" % (a.W, a.H, (a.W - 4) * (a.H - 4) * 16),
             "# dN = %d on %d copies, 4 epochs of minibatches of 128, Adam(1e-3), eps 0.2, lambda_e 0.01, target_kl 0.012; greedy undiscounted return over 100 episodes (-1 = every ball missed, +1 = every ball caught)" % (a.dN, a.envs),
             "# interactions  greedy_return  actor_loss  critic_loss  kl  entropy"]
    lines.append("%8d  %+.3f  -  -  -  -" % (0, greedy_return(env, pi.A)))
    for _ in range(a.N // a.chunk):
        crux.solve(solver, mdp)
        h = solver.history[-1]
        lines.append("%8d  %+.3f  %+.5f  %.5f  %+.5f  %.4f" % (solver.i, greedy_return(env, pi.A), h["actor_loss"], h["critic_loss"], h["kl"], h["entropy"]))
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.save:
        with open(os.path.join(ROOT, "profiles", "conv_pg_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
