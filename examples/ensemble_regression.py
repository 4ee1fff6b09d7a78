"""DeepEnsemble on a 1-D heteroscedastic toy (src/extras/deep_ensembles.jl): y = sin(3x) + noise whose spread grows with |x|, x in [-1, 1]; five 1-64-64-2
members trained with `fit`. Prints the falling training loss and the ensemble variance inside and far outside the data range: the members agree where they saw
data and disagree where they did not, which is what var* = mean(var_m + mu_m^2) - mu*^2 measures.

    python examples/ensemble_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import crux_jl_amd as crux  # noqa: E402


def main(epochs=60, n=1024, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (1, n)).astype(np.float32)
    y = (np.sin(3 * x) + (0.05 + 0.3 * np.abs(x)) * rng.standard_normal((1, n))).astype(np.float32)
    ens = crux.DeepEnsemble(lambda: crux.Chain(crux.Dense(1, 64, "relu"), crux.Dense(64, 64, "relu"), crux.Dense(64, 2)), 5, seed=seed)
    ens.attach_optimizer(crux.Adam(np.float32(3e-3)))
    print("training_loss before: %.4f" % crux.training_loss(ens, x, y))
    for k in range(0, epochs, 10):
        h = ens.fit(x, y, batch_size=128, epochs=10, seed=seed + k)
        print("epochs %3d  loss %.4f  member losses %s" % (k + 10, h["loss"], np.round(h["member_losses"], 3)))
    print("training_loss after:  %.4f" % crux.training_loss(ens, x, y))
    grid = np.array([[-0.9, 0.0, 0.9, 3.0, -4.0]], np.float32)
    mean, var = ens(grid)
    for g, m, v in zip(grid[0], mean[0], var[0]):
        print("x = %5.1f  mu* = %7.3f  var* = %8.4f  (%s the data)" % (g, m, v, "inside" if abs(g) <= 1 else "outside"))
    return var[0]


if __name__ == "__main__":
    main()
