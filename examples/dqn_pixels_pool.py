#!/usr/bin/env python
"""DQN from pixels on a pooled chain: examples/dqn_pixels.py's Catch game and run, with the textbook image network
    Chain(Scale(1 / 255), Conv((3, 3), 2 => 8, relu, pad=1), MaxPool((2, 2)), Conv((3, 3), 8 => 16, relu, pad=1), MaxPool((2, 2)), flatten, Dense(., 64, relu), Dense(64, 3)).
Trunk (conv and pooling kernels) and head run on the device. Writes the learning curve to profiles/conv_pool_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "examples"))
import crux_jl_amd as crux  # noqa: E402
from dqn_pixels import Catch, greedy_return  # noqa: E402


def pooled_chain(W, H, hidden, nout, pool=None):
    pool = pool or crux.MaxPool
    feats = (W // 2 // 2) * (H // 2 // 2) * 16
    return crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((3, 3), 2, 8, "relu", pad=1), pool((2, 2)), crux.Conv((3, 3), 8, 16, "relu", pad=1), pool((2, 2)), crux.flatten,
                      crux.Dense(feats, hidden, "relu"), crux.Dense(hidden, nout), input=(W, H, 2))


def q_network(W, H, seed=0, hidden=64, ctx=None):
    return crux.DiscreteNetwork(pooled_chain(W, H, hidden, 3), [0, 1, 2], seed=seed, **({"ctx": ctx} if ctx is not None else {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=8); ap.add_argument("--H", type=int, default=8); ap.add_argument("--N", type=int, default=6000)
    ap.add_argument("--chunk", type=int, default=1000); ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    env = Catch(a.W, a.H, seed=0); mdp = env.mdp()
    S = crux.ContinuousSpace((a.W, a.H, 2))
    Q = q_network(a.W, a.H)
    solver = crux.DQN(Q, S, N=a.chunk, dN=4, c_opt={"batch_size": 32, "optimizer": crux.Adam(np.float32(1e-3))}, buffer_size=5000, buffer_init=200, max_steps=a.H,
                      pi_explore=crux.EpsGreedyPolicy(crux.LinearDecaySchedule(1.0, 0.05, a.N // 2), [0, 1, 2]))
    lines = ["# examples/dqn_pixels_pool.py: DQN, Catch %d x %d x 2, Scale(1/255) -> Conv((3,3),2=>8,relu,pad=1) -> MaxPool((2,2)) -> Conv((3,3),8=>16,relu,pad=1) -> MaxPool((2,2)) -> flatten -> Dense(%d,64,relu) -> Dense(64,3)"
             % (a.W, a.H, Q.network.dims[0]),
             "# batch 32, Adam(1e-3), dN = 4, epsilon 1 -> 0.05 over %d interactions; greedy undiscounted return over 100 episodes (-1 = every ball missed, +1 = every ball caught)" % (a.N // 2),
             "# interactions  greedy_return  critic_loss  Qavg"]
    lines.append("%8d  %+.3f  %s  %s" % (0, greedy_return(env, Q), "-", "-"))
    for _ in range(a.N // a.chunk):
        crux.solve(solver, mdp)
        h = solver.history[-1]
        lines.append("%8d  %+.3f  %.5f  %+.4f" % (solver.i, greedy_return(env, Q), h["critic_loss"], h["Qavg"]))
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.save:
        with open(os.path.join(ROOT, "profiles", "conv_pool_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
