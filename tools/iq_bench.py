"""OnlineIQLearn's critic step: us per crux_iq_step with the gradient penalty on and off, at the CartPole shape (Q 4 -> 64 -> 64 -> 2, B = 128) and a wide shape
(8 -> 256 -> 256 -> 4, B = 256, the LunarLander-discrete fixture's 256 rows as the demo half). Device-synchronised host timing after warm-up; every call ends in
its own host synchronisation (the info read), so the figure includes one round trip. One JSON line per case."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import crux_jl_amd as crux  # noqa: E402


def chain(dims, acts):
    return crux.Chain(*[crux.Dense(dims[i], dims[i + 1], acts[i]) for i in range(len(acts))])


def run(dims, B, gp, act="relu", reps=200, fixture=None):
    ctx = crux.default_context(); rng = np.random.default_rng(0)
    od, A = dims[0], dims[-1]
    Q = crux.DiscreteNetwork(chain(dims, [act] * (len(dims) - 2) + ["identity"]), list(range(1, A + 1)), seed=1)
    Q.attach_optimizer(crux.Adam(np.float32(1e-4)))
    data = {"s": rng.normal(0, 1, (od, B)).astype(np.float32), "a": np.eye(A, dtype=bool)[rng.integers(0, A, B)].T.copy(),
            "sp": rng.normal(0, 1, (od, B)).astype(np.float32), "r": np.zeros((1, B), np.float32), "done": rng.random((1, B)) < 0.05}
    if fixture:                          # the demo half from the committed demonstrations
        f = np.load(os.path.join(ROOT, "tests", "golden", fixture + "_transitions.npz"))
        for k in ("s", "a", "sp", "done"):
            data[k][:, B // 2:] = f[k][:, :B // 2]
    D = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(A), B, ctx=ctx); D.push_(data)
    info, iq = np.zeros(crux._lib.INFO_N, np.float32), np.zeros(6, np.float32)
    step = lambda i: ctx.check(ctx.lib.crux_iq_step(Q.h, D.h, B // 2, 0.9, 1, 0.5, 1 if gp else 0, 10.0, 0, i,          # noqa: E731
                                                    info.ctypes.data_as(C.c_void_p), iq.ctypes.data_as(C.c_void_p)))
    for i in range(10):
        step(i)
    ctx.sync(); t0 = time.perf_counter()
    for i in range(reps):
        step(10 + i)
    ctx.sync(); us = 1e6 * (time.perf_counter() - t0) / reps
    r = {"shape": "-".join(map(str, dims)), "act": act, "B": B, "gp": gp, "iq_step_us": round(us, 1), "loss": float(info[0]), "grad_pen": float(iq[4])}
    print(json.dumps(r)); sys.stdout.flush()
    return r


CASES = [([4, 64, 64, 2], 128, False, "relu", None), ([8, 256, 256, 4], 256, False, "relu", "lunar_lander_discrete"),
         ([4, 64, 64, 2], 128, True, "relu", None), ([8, 256, 256, 4], 256, True, "relu", "lunar_lander_discrete"),
         ([8, 256, 256, 4], 256, True, "tanh", "lunar_lander_discrete")]

if __name__ == "__main__":
    # --case k: that case alone (k = 0..4, the order above), e.g. under rocprofv3 --kernel-trace --stats: 210 steps, 10 of them warm-up
    pick = [CASES[int(sys.argv[sys.argv.index("--case") + 1])]] if "--case" in sys.argv else CASES
    for dims, B, gp, act, fx in pick:
        run(dims, B, gp, act=act, fixture=fx)
