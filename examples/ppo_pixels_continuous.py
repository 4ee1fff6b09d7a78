#!/usr/bin/env python
"""PPO from pixels with a CONTINUOUS action: the Catch game of examples/ppo_pixels.py with a real-valued paddle. The action a in R moves the paddle by clip(a, -1, 1)
columns; it is drawn, and catches, at the nearest column. The actor is the reference's continuous form, GaussianPolicy(ContinuousNetwork(chain ending in 1 output), logSigma)
with a constant trainable logSigma (examples/rl/pendulum.jl), the critic a chain of the same shape: every minibatch goes through both trunks in one launch per layer
(csrc/conv_pair.hip) and the Gaussian column head of csrc/conv_gauss.hip. Writes the greedy (mu) return before and after training to profiles/conv_gauss_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "examples"))
import crux_jl_amd as crux  # noqa: E402
from dqn_pixels import Catch  # noqa: E402
from ppo_pixels import _chain  # noqa: E402


class CatchContinuous(Catch):
    """state: (ball column, ball row, paddle position in [0, W - 1], previous frame)"""

    @staticmethod
    def col(px):
        return int(np.floor(px + 0.5))

    def initialstate(self, e, n_resets):
        bx, by, px, prev = super().initialstate(e, n_resets)
        return (bx, by, float(px), prev)

    def gen(self, e, s, a, n_steps):
        bx, by, px, _ = s
        px2 = min(max(px + float(np.clip(np.asarray(a, np.float32).reshape(-1)[0], -1.0, 1.0)), 0.0), self.W - 1.0); by2 = by + 1
        r = 0.0 if by2 < self.H - 1 else (1.0 if bx == self.col(px2) else -1.0)
        return (bx, by2, px2, self.frame(bx, by, self.col(px))), r

    def observation(self, s):
        bx, by, px, prev = s
        return np.stack([self.frame(bx, by, self.col(px)), prev], axis=2).reshape(-1, order="F")

    def mdp(self, n_envs=1):
        return crux.HostMDP(self.initialstate, self.gen, self.isterminal, self.observation, obs_dim=self.W * self.H * 2, act_dim=1, discrete=False, n_envs=n_envs,
                            seed=self.seed, discount=0.99)


def actor_critic(W, H, seed=0, hidden=64, log_sigma=-0.7, ctx=None):
    kw = {"ctx": ctx} if ctx is not None else {}
    A = crux.GaussianPolicy(crux.ContinuousNetwork(_chain(W, H, hidden, 1), seed=seed, **kw), np.full(1, log_sigma, np.float32), seed=seed, **kw)
    return crux.ActorCritic(A, crux.ContinuousNetwork(_chain(W, H, hidden, 1), seed=seed + 1, **kw))


def greedy_return(env, A, Neps=100, seed_offset=10_000):
    """mean undiscounted return of Neps episodes under action(pi, s) = mu(s) on fresh seeds, the copies stepped side by side"""
    st = [env.initialstate(seed_offset + e, 0) for e in range(Neps)]; total = 0.0
    while not env.isterminal(st[0]):      # every episode has H - 1 steps
        mu = A.action(np.stack([env.observation(s) for s in st], axis=1))
        for e in range(Neps):
            st[e], r = env.gen(e, st[e], mu[:, e], 0); total += r
    return total / Neps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=8); ap.add_argument("--H", type=int, default=8); ap.add_argument("--N", type=int, default=16384)
    ap.add_argument("--dN", type=int, default=512); ap.add_argument("--envs", type=int, default=8); ap.add_argument("--chunk", type=int, default=2048); ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    env = CatchContinuous(a.W, a.H, seed=0); mdp = env.mdp(n_envs=a.envs)
    pi = actor_critic(a.W, a.H)
    opt = lambda: {"batch_size": 128, "epochs": 4, "optimizer": crux.Adam(np.float32(1e-3))}      # noqa: E731
    solver = crux.PPO(pi, crux.ContinuousSpace((a.W, a.H, 2)), N=a.chunk, dN=a.dN, max_steps=a.H, lambda_e=0.0, a_opt=opt(), c_opt=opt())
    lines = ["# examples/ppo_pixels_continuous.py: PPO, Catch %d x %d x 2 with a real-valued paddle move clip(a, -1, 1); actor GaussianPolicy(Scale(1/255) -> Conv((3,3),2=>8,relu) -> "
             "Conv((3,3),8=>16,relu) -> flatten -> Dense(%d,64,relu) -> Dense(64,1), logSigma = [-0.7]), critic the same chain" % (a.W, a.H, (a.W - 4) * (a.H - 4) * 16),
             "# dN = %d on %d copies, 4 epochs of minibatches of 128, Adam(1e-3), eps 0.2, lambda_e 0, target_kl 0.012; greedy (mu) undiscounted return over 100 episodes on fixed seeds "
             "(-1 = every ball missed, +1 = every ball caught); the first row is the untrained policy" % (a.dN, a.envs),
             "# interactions  greedy_return  actor_loss  critic_loss  kl  logSigma"]
    lines.append("%8d  %+.3f  -  -  -  %+.4f" % (0, greedy_return(env, pi.A), pi.A.log_sigma()[0]))
    for _ in range(a.N // a.chunk):
        crux.solve(solver, mdp)
        h = solver.history[-1]
        lines.append("%8d  %+.3f  %+.5f  %.5f  %+.5f  %+.4f" % (solver.i, greedy_return(env, pi.A), h["actor_loss"], h["critic_loss"], h["kl"], pi.A.log_sigma()[0]))
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.save:
        with open(os.path.join(ROOT, "profiles", "conv_gauss_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
