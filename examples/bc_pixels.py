#!/usr/bin/env python
"""Behaviour cloning from pixels on the environment of examples/dqn_pixels.py (Catch). A scripted expert moves the paddle under the ball; its (image, action) pairs go into an
ExperienceBuffer, and crux.BC clones a conv DiscreteNetwork
    Chain(Scale(1 / 255), Conv((3, 3), 2 => 8, relu), Conv((3, 3), 8 => 16, relu), flatten, Dense(., 64, relu), Dense(64, 3))
from them with logpdf_bc_loss: every minibatch is one crux_conv_bc_step over trunk + head, the validation error after each epoch one forward-only crux_conv_bc_loss over the
validation split (csrc/conv_bc.hip). Prints the validation error per epoch and the greedy returns of the untrained policy, the clone and the expert, all from this run.
Writes them to profiles/conv_bc_example.txt with --save."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "examples"))
import crux_jl_amd as crux  # noqa: E402
from dqn_pixels import Catch, greedy_return  # noqa: E402
from ppo_pixels import _chain as chain  # noqa: E402


def expert_action(s):
    """0 left, 1 stay, 2 right: towards the ball's column"""
    bx, _, px, _ = s
    return 1 + int(np.sign(bx - px))


def policy(W, H, seed=0, hidden=64, ctx=None):
    return crux.DiscreteNetwork(chain(W, H, hidden, 3), [0, 1, 2], seed=seed, **({"ctx": ctx} if ctx is not None else {}))


def rollouts(env, act, Neps, seed_offset):
    """(observations [W H C x n], actions [n], mean undiscounted return) of Neps episodes under act(state)"""
    obs, acts, total = [], [], 0.0
    for e in range(Neps):
        s = env.initialstate(seed_offset + e, 0)
        while not env.isterminal(s):
            a = act(s); obs.append(env.observation(s)); acts.append(a)
            s, r = env.gen(e, s, a, 0); total += r
    return np.stack(obs, axis=1), np.asarray(acts), total / Neps


def demonstrations(env, S, n, ctx=None, seed_offset=0):
    """an ExperienceBuffer of the expert's first n transitions (s and a are what BC reads; the other columns are zeros)"""
    obs, acts, _ = rollouts(env, expert_action, -(-n // (env.H - 1)), seed_offset); obs, acts = np.asfortranarray(obs[:, :n]), acts[:n]
    b = crux.ExperienceBuffer(S, crux.DiscreteSpace(3), n, [], **({"ctx": ctx} if ctx is not None else {}))
    b.push_({"s": obs, "sp": obs, "a": np.asfortranarray(np.eye(3, dtype=bool)[:, acts]), "r": np.zeros((1, n), np.float32), "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool)})
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=8); ap.add_argument("--H", type=int, default=8); ap.add_argument("--demos", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=20); ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    env = Catch(a.W, a.H, seed=0); S = crux.ContinuousSpace((a.W, a.H, 2))
    demo = demonstrations(env, S, a.demos); expert = rollouts(env, expert_action, 100, 10_000)[2]
    untrained = greedy_return(env, policy(a.W, a.H, seed=1)); pi = policy(a.W, a.H); before = greedy_return(env, pi)
    solver = crux.BC(pi, S, demo, opt={"batch_size": 128, "epochs": a.epochs - 1, "optimizer": crux.Adam(np.float32(1e-3))}, window=a.epochs)
    crux.solve(solver)
    after = greedy_return(env, pi)
    lines = ["# examples/bc_pixels.py: BC (logpdf_bc_loss, lambda_e 1e-3), Catch %d x %d x 2, %d expert transitions (70 %% training, 30 %% validation), minibatches of 128, Adam(1e-3)" % (a.W, a.H, a.demos),
             "# greedy undiscounted return over 100 episodes (-1 = every ball missed, +1 = every ball caught)", "# epoch  loss  validation_error  entropy"]
    lines += ["%4d  %.5f  %.5f  %.4f" % (e + 1, h["loss"], h["validation_error"], h["entropy"]) for e, h in enumerate(solver.history)]
    lines += ["# return: untrained (another seed) %+.3f, before %+.3f, after %+.3f, expert %+.3f; after > untrained: %s" % (untrained, before, after, expert, after > untrained)]
    print("\n".join(lines))
    if a.save:
        with open(os.path.join(ROOT, "profiles", "conv_bc_example.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
