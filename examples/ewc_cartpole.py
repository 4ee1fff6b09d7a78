#!/usr/bin/env python
"""Elastic weight consolidation on two CartPole tasks -- DiagonalFisherRegularizer (src/extras/fisher_information.jl) on cruxhip.

    reference (Julia)                                              this library
    R = DiagonalFisherRegularizer(Flux.params(pi), lam)            R = crux.DiagonalFisherRegularizer(actor, lam)
    update_fisher!(R, D, loss, Flux.params(pi), batch_size)        crux.update_fisher_(R, D, p, P, batch_size)
    TrainingParams(; loss, regularizer=R, ...)                     crux.TrainingParams(loss=..., regularizer=R, ...)

Task 1 is the device CartPole; task 2 is a numpy CartPole with the two actions swapped, stepped by the caller (HostMDP). After PPO on task 1 the Fisher diagonal of
logpdf_bc_loss on the last rollout buffer is taken; PPO then continues on task 2 with lam = 0 and with lam > 0, and the task-1 return is printed before and
after. Nothing about the outcome is asserted."""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux


def swapped_cartpole(n_envs, seed):
    """CartPole-v1's dynamics in numpy with action 0 pushing right and action 1 pushing left"""
    g, mc, mp, l, fm, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02

    def initialstate(e, n_resets):
        return np.random.default_rng([seed, e, n_resets]).uniform(-0.05, 0.05, 4)

    def gen(e, s, a, n_steps):
        x, xd, th, thd = s; f = fm if int(a) == 0 else -fm
        ct, st = math.cos(th), math.sin(th); tmp = (f + mp * l * thd * thd * st) / (mc + mp)
        tha = (g * st - ct * tmp) / (l * (4.0 / 3.0 - mp * ct * ct / (mc + mp))); xa = tmp - mp * l * tha * ct / (mc + mp)
        return np.array([x + tau * xd, xd + tau * xa, th + tau * thd, thd + tau * tha]), 1.0

    return crux.HostMDP(initialstate, gen, lambda sp: abs(sp[0]) > 2.4 or abs(sp[2]) > 12 * math.pi / 180, lambda s: np.asarray(s, np.float32), 4, 2, True,
                        n_envs=n_envs, seed=seed, discount=0.99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--lam", type=float, nargs="+", default=[1e5, 1e7], help="penalty weights tried on task 2 beside lam = 0 (F is a mean of squared batch-mean gradients: small numbers)")
    ap.add_argument("--eval", type=int, default=20)
    a = ap.parse_args()
    task1 = crux.CartPoleMDP(n_envs=a.envs, seed=0, discount=0.99); task2 = swapped_cartpole(a.envs, 1)
    S = task1.state_space(); dN = a.envs * a.T
    A = crux.DiscreteNetwork(crux.Chain(crux.Dense(4, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 2)), [1, 2], seed=1, stream=0)
    V = crux.ContinuousNetwork(crux.Chain(crux.Dense(4, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 1)), seed=1, stream=1)
    opts = {"batch_size": 128, "epochs": 10}
    ret1 = lambda pi: crux.undiscounted_return(crux.Sampler(task1, pi, max_steps=200), Neps=a.eval)

    def ret2(pi):      # the caller-stepped task: the mean undiscounted return of the episodes that end in one greedy block of steps!
        buf = crux.ExperienceBuffer(S, crux.DiscreteSpace(2), dN)
        return crux.steps_(crux.Sampler(task2, pi, S=S, max_steps=200), buf, Nsteps=dN, explore=False, i=0, reset=True)["avg_r"]

    solver = crux.PPO(crux.ActorCritic(A, V), S, N=a.iterations * dN, dN=dN, max_steps=200, a_opt=dict(opts), c_opt=dict(opts))
    pi1 = crux.solve(solver, task1)
    print("after task 1:             task-1 return %6.1f   task-2 return %6.1f" % (ret1(pi1), ret2(pi1)))

    # the Fisher diagonal of the behaviour-cloning log-likelihood on the last rollout of task 1
    R1 = crux.DiagonalFisherRegularizer(crux.actor(pi1), 1.0)
    crux.update_fisher_(R1, solver.buffer, crux.TrainingParams(loss=crux.logpdf_bc_loss, batch_size=128), {}, 128, per_minibatch=True)
    F, prev, N = R1.F, R1.theta_prev, R1.N
    print("Fisher diagonal from %d minibatch gradients: mean %.3g, max %.3g" % (N, F.mean(), F.max()))

    for lam in [0.0] + list(a.lam):
        pi = crux.clone_policy(pi1)
        R = crux.DiagonalFisherRegularizer(crux.actor(pi), lam); R.set_(F=F, theta_prev=prev, N=N)
        s2 = crux.PPO(pi, S, N=a.iterations * dN, dN=dN, max_steps=200, a_opt=dict(opts, regularizer=R), c_opt=dict(opts))
        crux.solve(s2, task2)
        print("after task 2, lam = %-6g task-1 return %6.1f   task-2 return %6.1f   R(pi) = %.4g   last actor_loss %+.4f" % (
            lam, ret1(pi), ret2(pi), R(), s2.history[-1]["actor_loss"]))


if __name__ == "__main__":
    main()
