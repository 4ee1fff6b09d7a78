#!/usr/bin/env python
"""DQN with the network and the optimiser of the reference's examples/rl/atari.jl, literally:

    Q() = DiscreteNetwork(Chain(x -> x ./ 255f0, Conv((8,8), 4=>16, relu, stride=4), Conv((4,4), 16=>32, relu, stride=2), flatten, Dense(2048, 256, relu), Dense(256, n)), as)
    DQN(pi=Q(), ..., c_opt=(optimizer=Flux.Optimiser(ClipValue(1f0), Adam(1f-3)),))

on a synthetic HostMDP, since no Atari emulator ships here: the catch game of examples/dqn_pixels.py on an 80 x 80 grid with four stacked frames (80 x 80 x 4 pixel values 0 / 255;
ball and paddle drawn as BLOCK x BLOCK squares so that the stride-4 first layer sees them). The dense head 2048-256-n is a wide handle (crux_mlp_create_wide); the update is
AdamClipGatedOp. Writes the learning curve to profiles/conv_atari_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402

W = H = 80; FRAMES = 4; BLOCK = 8; CELLS = W // BLOCK      # a 10 x 10 game drawn at 8 pixels per cell


class Catch80:
    """state: (ball cell column, ball cell row, paddle cell column, the three previous frames); actions 0 left, 1 stay, 2 right; +1 caught, -1 missed"""

    def __init__(self, seed=0):
        self.seed = int(seed)

    def frame(self, bx, by, px):
        f = np.zeros((W, H), np.float32)
        f[bx * BLOCK:(bx + 1) * BLOCK, by * BLOCK:(by + 1) * BLOCK] = 255.0; f[px * BLOCK:(px + 1) * BLOCK, H - BLOCK:H] = 255.0
        return f

    def initialstate(self, e, n_resets):
        rng = np.random.default_rng([self.seed, e, n_resets]); z = np.zeros((W, H), np.float32)
        return (int(rng.integers(CELLS)), 0, int(rng.integers(CELLS)), (z, z, z))

    def gen(self, e, s, a, n_steps):
        bx, by, px, prev = s
        px2 = min(max(px + int(a) - 1, 0), CELLS - 1); by2 = by + 1
        r = 0.0 if by2 < CELLS - 1 else (1.0 if bx == px2 else -1.0)
        return (bx, by2, px2, (self.frame(bx, by, px),) + prev[:2]), r

    def isterminal(self, s):
        return s[1] >= CELLS - 1

    def observation(self, s):
        bx, by, px, prev = s
        return np.stack((self.frame(bx, by, px),) + prev, axis=2).reshape(-1, order="F")      # index w + W (h + H c)

    def mdp(self, n_envs=1):
        return crux.HostMDP(self.initialstate, self.gen, self.isterminal, self.observation, obs_dim=W * H * FRAMES, act_dim=3, discrete=True, n_envs=n_envs, seed=self.seed, discount=0.99)


def q_network(n_actions=3, seed=0, ctx=None):
    chain = crux.Chain(crux.Scale(1.0 / 255.0), crux.Conv((8, 8), 4, 16, "relu", stride=4), crux.Conv((4, 4), 16, 32, "relu", stride=2), crux.flatten,
                       crux.Dense(2048, 256, "relu"), crux.Dense(256, n_actions), input=(W, H, FRAMES))
    return crux.DiscreteNetwork(chain, list(range(n_actions)), seed=seed, **({"ctx": ctx} if ctx is not None else {}))


def greedy_return(env, Q, Neps=50, seed_offset=10_000):
    st = [env.initialstate(seed_offset + e, 0) for e in range(Neps)]; total = 0.0
    while not env.isterminal(st[0]):      # every episode has CELLS - 1 steps
        q = crux.value(Q, np.stack([env.observation(s) for s in st], axis=1))
        for e in range(Neps):
            st[e], r = env.gen(e, st[e], int(np.argmax(q[:, e])), 0); total += r
    return total / Neps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=6000); ap.add_argument("--chunk", type=int, default=1000); ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    env = Catch80(seed=0); mdp = env.mdp(); S = crux.ContinuousSpace((W, H, FRAMES)); Q = q_network()
    opt = crux.Optimiser(crux.ClipValue(np.float32(1)), crux.Adam(np.float32(1e-3)))
    solver = crux.DQN(Q, S, N=a.chunk, dN=4, c_opt={"batch_size": 32, "optimizer": opt}, buffer_size=4000, buffer_init=200, max_steps=CELLS,
                      pi_explore=crux.EpsGreedyPolicy(crux.LinearDecaySchedule(1.0, 0.05, a.N // 2), [0, 1, 2]))
    lines = ["# examples/dqn_atari_network.py: DQN, catch on 80 x 80 x 4, Scale(1/255) -> Conv((8,8),4=>16,relu,stride=4) -> Conv((4,4),16=>32,relu,stride=2) -> flatten -> Dense(2048,256,relu) -> Dense(256,3)",
             "# Optimiser(ClipValue(1), Adam(1e-3)), batch 32, dN = 4, epsilon 1 -> 0.05 over %d interactions; greedy undiscounted return over 50 episodes (-1 = every ball missed, +1 = every ball caught)" % (a.N // 2),
             "# interactions  greedy_return  critic_loss  critic_grad_norm  Qavg"]
    lines.append("%8d  %+.3f  %s  %s  %s" % (0, greedy_return(env, Q), "-", "-", "-"))
    for _ in range(a.N // a.chunk):
        crux.solve(solver, mdp)
        h = solver.history[-1]
        lines.append("%8d  %+.3f  %.5f  %.4f  %+.4f" % (solver.i, greedy_return(env, Q), h["critic_loss"], h["critic_grad_norm"], h["Qavg"]))
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.save:
        with open(os.path.join(ROOT, "profiles", "conv_atari_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
