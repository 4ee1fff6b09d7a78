#!/usr/bin/env python
"""DQN from pixels (the shape of the reference's examples/rl/atari.jl, at toy size): a ball falls on a W x H grid, a paddle on the bottom row catches it (+1) or misses (-1).
The observation is two stacked frames (the current and the previous one) as a W x H x 2 image of 0 / 255 pixel values; the Q network is
    Chain(Scale(1 / 255), Conv((3, 3), 2 => 8, relu), Conv((3, 3), 8 => 16, relu), flatten, Dense(., 64, relu), Dense(64, 3)).
The environment lives on the host (a HostMDP); trunk and head run on the device. Writes the learning curve to profiles/conv_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402


class Catch:
    """state: (ball column, ball row, paddle column, previous frame); row 0 is the top, the paddle lives on row H - 1. Actions: 0 left, 1 stay, 2 right."""

    def __init__(self, W, H, seed=0):
        self.W, self.H, self.seed = int(W), int(H), int(seed)

    def frame(self, bx, by, px):
        f = np.zeros((self.W, self.H), np.float32); f[bx, by] = 255.0; f[px, self.H - 1] = 255.0
        return f

    def initialstate(self, e, n_resets):
        rng = np.random.default_rng([self.seed, e, n_resets])
        return (int(rng.integers(self.W)), 0, int(rng.integers(self.W)), np.zeros((self.W, self.H), np.float32))

    def gen(self, e, s, a, n_steps):
        bx, by, px, _ = s
        px2 = min(max(px + int(a) - 1, 0), self.W - 1); by2 = by + 1
        r = 0.0 if by2 < self.H - 1 else (1.0 if bx == px2 else -1.0)
        return (bx, by2, px2, self.frame(bx, by, px)), r

    def isterminal(self, s):
        return s[1] >= self.H - 1

    def observation(self, s):
        bx, by, px, prev = s
        return np.stack([self.frame(bx, by, px), prev], axis=2).reshape(-1, order="F")      # index w + W (h + H c)

    def mdp(self, n_envs=1):
        return crux.HostMDP(self.initialstate, self.gen, self.isterminal, self.observation, obs_dim=self.W * self.H * 2, act_dim=3, discrete=True, n_envs=n_envs,
                            seed=self.seed, discount=0.99)


def q_network(W, H, seed=0, hidden=64, ctx=None):
    c1, c2 = crux.Conv((3, 3), 2, 8, "relu"), crux.Conv((3, 3), 8, 16, "relu")
    feats = (W - 4) * (H - 4) * 16
    chain = crux.Chain(crux.Scale(1.0 / 255.0), c1, c2, crux.flatten, crux.Dense(feats, hidden, "relu"), crux.Dense(hidden, 3), input=(W, H, 2))
    return crux.DiscreteNetwork(chain, [0, 1, 2], seed=seed, **({"ctx": ctx} if ctx is not None else {}))


def greedy_return(env, Q, Neps=100, seed_offset=10_000):
    """mean undiscounted return of Neps greedy episodes on fresh seeds, the Neps copies stepped side by side (one value(pi, s) call per time step)"""
    st = [env.initialstate(seed_offset + e, 0) for e in range(Neps)]; total = 0.0
    while not env.isterminal(st[0]):      # every episode has H - 1 steps
        q = crux.value(Q, np.stack([env.observation(s) for s in st], axis=1))
        for e in range(Neps):
            st[e], r = env.gen(e, st[e], int(np.argmax(q[:, e])), 0); total += r
    return total / Neps


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
    lines = ["# examples/dqn_pixels.py: DQN, Catch %d x %d x 2, Scale(1/255) -> Conv((3,3),2=>8,relu) -> Conv((3,3),8=>16,relu) -> flatten -> Dense(%d,64,relu) -> Dense(64,3)" % (a.W, a.H, (a.W - 4) * (a.H - 4) * 16),
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
        with open(os.path.join(ROOT, "profiles", "conv_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
