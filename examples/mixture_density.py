"""MixtureNetwork on the reference's DeepGMM experiment (test/mixture_network_tests.jl): the target is 0.5 N(1, 0.2) + 0.5 N(-1, 1), the input is the constant 0.1, and two
2-32-1 GaussianPolicy components with a 2-32-2 weight network are trained with `fit` on -mean(logpdf). Prints the falling negative log-likelihood and the fitted
alpha, mu and sigma; a single Gaussian cannot get below 0.5 log(2 pi e var) = 1.63 on this target, the mixture does.

    python examples/mixture_density.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux  # noqa: E402


def target(n, rng):
    first = rng.uniform(0, 1, n) < 0.5
    return np.where(first, rng.normal(1.0, 0.2, n), rng.normal(-1.0, 1.0, n)).astype(np.float32).reshape(1, n)


def main(epochs=60, n=8192, seed=0):
    rng = np.random.default_rng(seed)
    x, y, y_held = np.full((2, n), 0.1, np.float32), target(n, rng), target(n, rng)
    comps = [crux.GaussianPolicy(crux.Chain(crux.Dense(2, 32, "relu"), crux.Dense(32, 1)), np.zeros(1, np.float32), seed=seed, stream=k) for k in range(2)]
    pi = crux.MixtureNetwork(comps, crux.Chain(crux.Dense(2, 32, "relu"), crux.Dense(32, 2)), seed=seed)
    pi.attach_optimizer(crux.Adam(np.float32(3e-3)))
    nll = lambda yy: float(-pi.logpdf(x, yy).mean(dtype=np.float64))      # noqa: E731
    print("single-Gaussian optimum on the held-out sample: %.4f" % (0.5 * np.log(2 * np.pi * np.e * y_held.var(dtype=np.float64))))
    print("NLL before: train %.4f  held-out %.4f" % (nll(y), nll(y_held)))
    for k in range(0, epochs, 10):
        h = pi.fit(x, y, batch_size=256, epochs=10, seed=seed + k)
        print("epochs %3d  loss %.4f  grad norm %.4f  mean responsibilities %s" % (k + 10, h["loss"], h["grad_norm"], np.round(h["responsibilities"], 3)))
    print("NLL after:  train %.4f  held-out %.4f" % (nll(y), nll(y_held)))
    alpha = pi.weights(x[:, :1])[:, 0]; mu = [float(m[0, 0]) for m in pi.means(x[:, :1])]; sigma = [float(np.exp(c.get_params()[-1])) for c in comps]
    print("fitted: %.2f N(%.2f, %.2f) + %.2f N(%.2f, %.2f)   (target 0.50 N(1.00, 0.20) + 0.50 N(-1.00, 1.00))" % (alpha[0], mu[0], sigma[0], alpha[1], mu[1], sigma[1]))
    a, lp, k = pi.exploration(x[:, :8], seed=seed, counter=0)
    print("eight draws: %s from components %s" % (np.round(a[0], 2), k))
    return nll(y_held)


if __name__ == "__main__":
    main()
