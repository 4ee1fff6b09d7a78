"""DeepClassificationEnsemble over images (src/extras/deep_ensembles.jl with a conv generator): which quadrant of a 12 x 12 x 1 image holds a 4 x 4 blob, under noise; five
Conv((3, 3), 1 => 4, relu) -> flatten -> Dense(400, 4) members on the member-grouped conv passes. Prints the cross-entropy and the ensemble accuracy before and after `fit`.

    python examples/ensemble_images.py [--save]      (--save writes the printed lines to profiles/conv_ensemble_example.txt)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import crux_jl_amd as crux      # noqa: E402


def blobs(n, rng, noise=0.5):
    X = rng.normal(0, noise, (12, 12, 1, n)).astype(np.float32); c = rng.integers(0, 4, n)
    for j, k in enumerate(c):
        X[6 * (k % 2) + 1:6 * (k % 2) + 5, 6 * (k // 2) + 1:6 * (k // 2) + 5, 0, j] += 1.0
    return X, np.asfortranarray(np.eye(4, dtype=np.float32)[:, c]), c


def main():
    rng = np.random.default_rng(0); X, Y, c = blobs(512, rng); Xt, Yt, ct = blobs(256, rng)
    ens = crux.DeepClassificationEnsemble(lambda: crux.Chain(crux.Conv((3, 3), 1, 4, "relu"), crux.flatten, crux.Dense(400, 4), input=(12, 12, 1)), 5, seed=1)
    ens.attach_optimizer(crux.Adam(np.float32(3e-3)))
    lines = []
    report = lambda tag: lines.append("%s: cross-entropy train %.4f test %.4f, ensemble accuracy train %.3f test %.3f" % (      # noqa: E731
        tag, crux.training_loss(ens, X, Y), crux.training_loss(ens, Xt, Yt), float((np.argmax(ens(X), 0) == c).mean()), float((np.argmax(ens(Xt), 0) == ct).mean())))
    report("before fit")
    out = ens.fit(X, Y, batch_size=64, epochs=20, seed=2)
    lines.append("fit: %d epochs, %d batches, last step's loss %.4f, grad norm %.4f" % (out["epochs_run"], out["batches_trained"], out["loss"], out["grad_norm"]))
    report("after fit")
    print("\n".join(lines))
    if "--save" in sys.argv:
        open(os.path.join(ROOT, "profiles", "conv_ensemble_example.txt"), "w").write("# python examples/ensemble_images.py: M = 5, 512 training and 256 test images\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
