"""step time of batch_train! with a DiagonalFisherRegularizer (elastic weight consolidation): Gaussian PPO 17-256-256-6, minibatches of 256, one epoch of 16 minibatches.

  (a) crux_batch_train               unregularised: the dense-engine learner's chain as it is
  (b) crux_batch_train_fisher        the regulariser inside that chain (two more launches per minibatch, the un-fused layer-0 pullback)
  (c) batch_train_ with a numpy closure that computes the same penalty -- the host seam (crux_loss_grad, gradient to the host and back, crux_adam_apply per minibatch):
      the only way to run EWC without the device regulariser, so this line is the baseline

Every timed call ends in a synchronisation (its info rows are read back); host clock, us per minibatch, the median of `reps` calls after a warm-up call."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import crux_jl_amd as crux
import fisher_reference as FR

DIMS, AD, BS, NMB, LAM = [17, 256, 256, 6], 6, 256, 16, 0.7


def make():
    acts = ["tanh", "tanh", "identity"]
    A = crux.GaussianPolicy(crux.Chain(*[crux.Dense(DIMS[i], DIMS[i + 1], acts[i]) for i in range(3)]), np.full(AD, -0.5, np.float32), seed=1)
    rng = np.random.default_rng(0); n = BS * NMB; extras = ["return", "logprob", "advantage"]
    buf = crux.ExperienceBuffer(crux.ContinuousSpace(DIMS[0]), crux.ContinuousSpace(AD), n, extras)
    d = {"s": rng.standard_normal((DIMS[0], n)).astype(np.float32), "sp": rng.standard_normal((DIMS[0], n)).astype(np.float32), "r": np.ones((1, n), np.float32),
         "done": np.zeros((1, n), bool), "episode_end": np.zeros((1, n), bool), "a": rng.normal(0, 0.7, (AD, n)).astype(np.float32),
         "return": rng.standard_normal((1, n)).astype(np.float32), "advantage": rng.standard_normal((1, n)).astype(np.float32),
         "logprob": rng.normal(-1.2 * AD, 0.05, (1, n)).astype(np.float32)}
    buf.push_(d)
    return A, buf, rng


def timed(A, buf, p, P, reps):
    crux.batch_train_(A, p, P, buf)                       # warm-up: code objects, workspaces, the optimiser state
    ts = []
    for _ in range(reps):
        buf.ctx.sync(); t0 = time.perf_counter(); info = crux.batch_train_(A, p, P, buf); buf.ctx.sync()
        ts.append(1e6 * (time.perf_counter() - t0) / info["x_batches_trained"])
    return float(np.median(ts))


def main(reps=9):
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.0}
    A, buf, rng = make(); n = A.n_params; tab = FR.array_table(DIMS, AD)
    prev = (A.get_params() + 0.01 * rng.standard_normal(n)).astype(np.float32); F = (rng.standard_normal(n) ** 2).astype(np.float32)
    kw = dict(loss=crux.ppo_loss, batch_size=BS, epochs=1, target_kl=None, name="x_", optimizer=crux.Adam(np.float32(1e-5)))
    a = timed(A, buf, crux.TrainingParams(**kw), P, reps)
    R = crux.DiagonalFisherRegularizer(A, LAM); R.set_(F=F, theta_prev=prev)
    b = timed(A, buf, crux.TrainingParams(regularizer=R, **kw), P, reps)

    def closure(theta):                                   # the same penalty in numpy: (value, gradient) over the flat parameter vector
        return (np.float32(FR.value_f32(theta, prev, F, LAM, tab)), FR.gradient_f32(theta, prev, F, LAM, tab))
    c = timed(A, buf, crux.TrainingParams(regularizer=closure, **kw), P, max(3, reps // 3))
    print("Gaussian PPO %s, minibatch %d, %d minibatches per epoch, us per minibatch (median of %d calls):" % ("-".join(map(str, DIMS)), BS, NMB, reps))
    print("(a) crux_batch_train, unregularised                 %8.1f" % a)
    print("(b) crux_batch_train_fisher                         %8.1f   (+%.1f over (a))" % (b, b - a))
    print("(c) batch_train_ with a numpy closure (host seam)   %8.1f   (%.1fx (b))" % (c, c / b))


if __name__ == "__main__":
    main()
