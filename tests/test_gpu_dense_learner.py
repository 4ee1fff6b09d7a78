"""crux_train_dense_run (csrc/train_dense.hip) against the oracle at the minibatch sizes of the reference's own on-policy examples: 256, 512 (Pendulum) and 4000 (HalfCheetah).

Every minibatch above 128 trains on the dense engine: k_gather_obs, the staging carve (bmax), k_pg_head's one-block walk with Float64 statistics, the ragged last minibatch, the
per-step host sync under target_kl / max_batches and the NaN gate (adam_gated behind k_sumsq2) all depend on the minibatch size. The steps are driven through batch_train_ with
injected permutations (single-step entry points carry ids, which crux_train_dense_eligible sends to the generic learner), and every tolerance is one the suite already asserts:
gradient 1e-4 x scale, infos 1e-4, parameters 2e-5, Adam moments 1e-5 (test_gpu_components.py), teacher-forced windows 2e-6 (test_gpu_round3.py).
That the dense chain is what runs: no minibatch above 128 is taken by the register-resident kernels (learner_route.h: a.bs > 128), and the generic learner announces itself on
stderr for every network of 2048 parameters or more -- the tests assert that it did not (the hook of test_gpu_round2.py / test_gpu_round3.py).
"""
import ctypes as C

import numpy as np
import pytest

import crux_jl_amd as crux
from crux_jl_amd import _lib as L
import dense_reference as R
import oracle as O
import parity

pytestmark = pytest.mark.gpu
P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
EXTRAS = ["return", "logprob", "advantage"]


def _not_generic(capfd):
    assert "outside the MFMA learner family" not in capfd.readouterr().err


def _pair(kind, dims, acts, n, rng, seed=21):
    """_train_pair of test_gpu_components.py, with kink-free observations (at the initial parameters) for relu members"""
    od = dims[0]; ad = dims[-1] if kind != "value" else 2; disc = kind == "categorical"
    g, o = parity.make_pair(dims, acts, seed, 0, "discrete" if disc else ("gaussian" if kind == "gaussian" else "continuous"), n_extra=dims[-1] if kind == "gaussian" else 0, extra_init=-0.3)
    A = crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad)
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), A, n, EXTRAS); ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, n, EXTRAS)
    d = {"s": rng.standard_normal((od, n)).astype(np.float32), "sp": rng.standard_normal((od, n)).astype(np.float32), "r": rng.standard_normal((1, n)).astype(np.float32),
         "done": rng.random((1, n)) < 0.2, "episode_end": rng.random((1, n)) < 0.2}
    if "relu" in acts:
        d["s"] = np.ascontiguousarray(R.kink_free_inputs(o.params, dims, acts, n, rng, 1e-4))
    if disc:
        a = np.zeros((ad, n), np.bool_); a[rng.integers(0, ad, n), np.arange(n)] = True; d["a"] = a
    else:
        d["a"] = rng.standard_normal((ad, n)).astype(np.float32)
    for k in EXTRAS:
        d[k] = rng.standard_normal((1, n)).astype(np.float32)
    d["logprob"] = (-0.7 + 0.05 * rng.standard_normal((1, n))).astype(np.float32) if disc else (-1.2 * ad + 0.1 * rng.standard_normal((1, n))).astype(np.float32)
    gb.push_(d); ob.push(d)
    return g, o, gb, ob


RELU, TANH = "relu", "tanh"
STEP_CASES = [("categorical", [4, 64, 64, 2], RELU, 256), ("categorical", [4, 64, 64, 2], RELU, 512), ("categorical", [4, 64, 64, 2], RELU, 4000),
              ("value", [4, 64, 64, 1], RELU, 256), ("value", [4, 64, 64, 1], RELU, 512), ("value", [4, 64, 64, 1], RELU, 4000),
              ("gaussian", [3, 64, 64, 1], RELU, 512), ("value", [3, 64, 64, 1], RELU, 512),                                    # the Pendulum example
              ("gaussian", [17, 64, 32, 6], TANH, 4000), ("value", [17, 64, 32, 1], TANH, 4000),                                # cheetah_ref
              ("gaussian", [17, 64, 64, 6], TANH, 256), ("gaussian", [17, 64, 64, 6], TANH, 512), ("gaussian", [17, 64, 64, 6], TANH, 4000),
              ("categorical", [8, 256, 256, 4], RELU, 256), ("categorical", [8, 256, 256, 4], RELU, 512),                        # 256 / 192 wide: at 256 the fused pullback (Wgrad2Op, Dgrad2W1Op, Sumsq2Op's quarter combine)
              ("value", [4, 192, 192, 1], RELU, 256), ("value", [4, 192, 192, 1], RELU, 512), ("value", [4, 192, 192, 1], TANH, 256),
              ("categorical", [6, 32, 5], RELU, 256)]


@pytest.mark.parametrize("kind,dims,act,bs", STEP_CASES, ids=["%s_%s_%s_bs%d" % (k, "-".join(map(str, d)), a, b) for k, d, a, b in STEP_CASES])
def test_dense_learner_step_and_three_adam_steps_match_oracle(gpu_ctx, capfd, kind, dims, act, bs):
    """The body of test_gpu_components.py::test_train_step_and_loss_grad_match_oracle with its tolerances, at n = 2 bs + 37 (a ragged tail shorter than 128): one step
    (max_batches = 1), then the three minibatches of a second permutation (max_batches = 3: bs, bs, 37 rows). 6-32-5 has 389 parameters and stays, by
    crux_train_dense_eligible's own rule (n_params >= 512), on the generic learner: it is here for the minibatch size."""
    rng = np.random.default_rng(7); acts = [act] * (len(dims) - 2) + ["identity"]; n = 2 * bs + 37
    g, o, gb, ob = _pair(kind, dims, acts, n, rng)
    loss = crux.value_mse_loss if kind == "value" else crux.ppo_loss
    lname, head = ("value_mse", "deterministic") if kind == "value" else ("ppo", kind)
    o.adam_init(float(np.float32(3e-4)))
    # the oracle's gradient of the first minibatch, then the step itself on both sides
    perm = rng.permutation(n).astype(np.int64); ids = np.ascontiguousarray(perm[:bs])
    cfg = parity.train_cfg(lname, head, bs, 1, max_batches=1); oinfo = np.zeros(L.INFO_N, np.float32)
    O.chk(O.lib().orc_loss_grad(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(oinfo)))
    ograds = o.grads.copy()
    p1 = crux.TrainingParams(loss=loss, batch_size=bs, epochs=1, max_batches=1, name="x_")
    info = crux.batch_train_(g, p1, P, gb, perms=perm[None, :] + 1)
    assert info["x_batches_trained"] == 1
    gg = np.empty(o.n, np.float32); g.ctx.d2h(g.ctx.lib.crux_mlp_grads_ptr(g.h), gg)
    scale = max(1.0, np.abs(ograds).max())
    print("STEP %s grad %.3g of scale %.3g" % (dims, np.abs(gg - ograds).max(), scale))
    assert np.abs(gg - ograds).max() < 1e-4 * scale, np.abs(gg - ograds).max()
    raw = {"loss": info["x_loss"], "grad_norm": info["x_grad_norm"]}
    if kind != "value":
        raw.update({k: info[k] for k in ("kl", "entropy", "clip_fraction", "avg_advantage", "avg_return")})
    for k, v in raw.items():
        assert abs(v - oinfo[L.INFO[k]]) < 1e-4 * max(1.0, abs(oinfo[L.INFO[k]])), k
    oi = np.zeros(L.INFO_N, np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(np.ascontiguousarray(perm[None, :])), O.vpz(oi), None))
    assert int(oi[L.INFO["batches_trained"]]) == 1
    assert np.abs(g.get_params() - o.params).max() < 2e-5
    # three Adam steps on the minibatches of another permutation, the last one ragged
    perm2 = rng.permutation(n).astype(np.int64)
    p3 = crux.TrainingParams(loss=loss, optimizer=p1.optimizer, batch_size=bs, epochs=1, max_batches=3, name="x_")
    info3 = crux.batch_train_(g, p3, P, gb, perms=perm2[None, :] + 1)
    cfg3 = parity.train_cfg(lname, head, bs, 1, max_batches=3)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg3), O.vpz(np.ascontiguousarray(perm2[None, :])), O.vpz(oi), None))
    assert info3["x_batches_trained"] == int(oi[L.INFO["batches_trained"]]) == 3
    assert abs(info3["x_loss"] - oi[0]) < 1e-4 * max(1, abs(oi[0]))
    d = np.abs(g.get_params() - o.params).max(); print("STEP %s params after 4 steps %.3g" % (dims, d))
    assert d < 2e-5
    m, v, bp = g.adam_state(); om, ov, obp = o.adam_state()
    assert np.abs(m - om).max() < 1e-5 * max(1, np.abs(om).max()) and np.allclose(bp, obp, rtol=1e-12)
    for k in gb.keys():
        assert np.array_equal(gb[k], ob[k]), k
    _not_generic(capfd)


WINDOW_CASES = [("categorical", [4, 64, 64, 2], RELU, 256), ("categorical", [4, 64, 64, 2], RELU, 512), ("value", [3, 64, 64, 1], RELU, 512), ("gaussian", [3, 64, 64, 1], RELU, 256),
                ("gaussian", [17, 64, 64, 6], TANH, 256), ("gaussian", [17, 64, 64, 6], TANH, 512), ("value", [17, 64, 64, 1], TANH, 512),
                ("gaussian", [17, 64, 32, 6], TANH, 4000), ("value", [17, 64, 32, 1], "cheetah_critic", 4000), ("gaussian", [17, 64, 64, 6], TANH, 4000), ("value", [17, 64, 64, 1], TANH, 4000)]


@pytest.mark.parametrize("kind,dims,act,bs", WINDOW_CASES, ids=["%s_%s_%s_bs%d" % (k, "-".join(map(str, d)), a, b) for k, d, a, b in WINDOW_CASES])
def test_dense_learner_teacher_forced_windows(gpu_ctx, capfd, kind, dims, act, bs):
    """Two teacher-forced windows of four minibatch steps (steps 2..5 and 9..12 of the oracle's trajectory) as in test_learner_dispatch_over_random_shapes_matches_the_oracle,
    with named shapes instead of drawn ones and the minibatches of the reference's examples.
    (Its Gaussian rows of 4..8 actions train on fully clipped, dead surrogate gradients -- logprob ~ N(-1.2, 0.05); live gradients and the row edges: test_gpu_learner_row_edges.py.)"""
    rng = np.random.default_rng(2027); od = dims[0]; ad = dims[-1] if kind != "value" else 2; disc = kind == "categorical"; N = bs * 14
    acts = parity.CRITIC_ACTS["cheetah_ref"] if act == "cheetah_critic" else [act, act, "identity"]
    act_col = np.eye(ad, dtype=bool)[:, rng.integers(0, ad, N)] if disc else rng.normal(0, 0.7, (ad, N)).astype(np.float32)
    data0 = {"s": rng.normal(0, 1, (od, N)).astype(np.float32), "a": act_col, "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
             "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": rng.normal(0, 1, (1, N)).astype(np.float32),
             "logprob": rng.normal(-1.2, 0.05, (1, N)).astype(np.float32), "advantage": rng.normal(0, 1, (1, N)).astype(np.float32)}
    if kind == "categorical":
        (g, o), loss, head = parity.make_pair(dims, acts, 411, 0, "discrete"), "ppo", "categorical"
    elif kind == "gaussian":
        (g, o), loss, head = parity.make_pair(dims, acts, 411, 0, "gaussian", n_extra=ad, extra_init=-0.5), "ppo", "gaussian"
    else:
        (g, o), loss, head = parity.make_pair(dims, acts, 411, 0), "value_mse", "deterministic"
    res, _ = parity.learner_window_parity(g, o, data0, od, ad, disc, loss, head, bs, 1, [2, 9], 4, seed=811)
    assert len(res) == 2, res
    for start, W, d in res:
        print("WINDOW %s bs %d start %d: %.3g" % (dims, bs, start, d))
        assert d < 2e-6, (start, d)
    _not_generic(capfd)


def test_dense_learner_whole_epochs_ragged_early_stop_and_max_batches(gpu_ctx, capfd):
    """test_batch_train_early_stop_perms_and_ragged at a minibatch of 256 on 1300 rows (5 x 256 + 20)."""
    rng = np.random.default_rng(8); n, bs, epochs = 1300, 256, 3; nmb = 6
    g, o, gb, ob = _pair("categorical", [4, 64, 64, 2], ["relu", "relu", "identity"], n, rng)
    perms = np.stack([rng.permutation(n) + 1 for _ in range(epochs)])
    # (a) injected permutations, ragged last minibatch, no early stop
    p = crux.TrainingParams(loss=crux.ppo_loss, optimizer=crux.Adam(1e-3), batch_size=bs, epochs=epochs, name="actor_")
    o.adam_init(1e-3)
    info = crux.batch_train_(g, p, P, gb, perms=perms)
    cfg = parity.train_cfg("ppo", "categorical", bs, epochs); oinfo = np.zeros(L.INFO_N, np.float32); oep = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(np.ascontiguousarray(perms - 1)), O.vpz(oinfo), O.vpz(oep)))
    assert info["actor_batches_trained"] == int(oinfo[L.INFO["batches_trained"]]) == epochs * nmb
    d = np.abs(g.get_params() - o.params).max(); print("EPOCHS params after %d steps %.3g" % (epochs * nmb, d))
    assert d < 2e-5
    assert np.allclose(info["_epoch_infos"][:, :7], oep[:, :7], rtol=2e-3, atol=2e-5)
    for k in gb.keys():
        assert np.array_equal(gb[k], ob[k]), k
    # (b) KL early stopping with an aggressive step: the per-minibatch host sync (step_sync) must stop at the oracle's minibatch
    p2 = crux.TrainingParams(loss=crux.ppo_loss, optimizer=crux.Adam(0.03), batch_size=bs, epochs=5, target_kl=0.01, name="actor_", shuffle_seed=5)
    o.adam_init(0.03); g.optimizer = None
    info2 = crux.batch_train_(g, p2, P, gb)
    cfg2 = parity.train_cfg("ppo", "categorical", bs, 5, 0.01, 5)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg2), None, O.vpz(oinfo), None))
    assert info2["actor_batches_trained"] == int(oinfo[L.INFO["batches_trained"]]) and info2["_epochs_run"] == int(oinfo[L.INFO["epochs_run"]])
    assert info2["actor_batches_trained"] < 5 * nmb                                     # it did stop early
    assert info2["kl"] > 0.01 and abs(info2["kl"] - oinfo[L.INFO["kl"]]) < 1e-5
    # (c) max_batches not a multiple of the minibatches of an epoch: 13 = 2 x 6 + 1
    p3 = crux.TrainingParams(loss=crux.ppo_loss, batch_size=bs, epochs=5, name="actor_", max_batches=13, shuffle_seed=9); g.optimizer = None
    info3 = crux.batch_train_(g, p3, P, gb)
    assert info3["actor_batches_trained"] == 13 and info3["_epochs_run"] == 3
    _not_generic(capfd)


def test_dense_learner_nan_return_is_reported_and_nothing_moves(gpu_ctx, capfd):
    """A NaN :return column under the value loss at a minibatch of 512: CRUX_ENAN (src/training.jl:20), parameters and Adam state untouched -- adam_gated behind k_sumsq2."""
    rng = np.random.default_rng(9); n, bs = 1061, 512
    g, o, gb, ob = _pair("value", [4, 64, 64, 1], ["relu", "relu", "identity"], n, rng)
    p = crux.TrainingParams(loss=crux.value_mse_loss, batch_size=bs, epochs=2, name="critic_")
    crux.batch_train_(g, p, {}, gb)                                        # some real steps first: the Adam state is not all zeros
    gb["return"] = np.full((1, n), np.nan, np.float32)
    before = g.get_params(); m0, v0, bp0 = g.adam_state()
    assert np.abs(m0).max() > 0
    with pytest.raises(crux.CruxError) as e:
        crux.batch_train_(g, p, {}, gb)
    assert e.value.code == L.ENAN and np.array_equal(g.get_params(), before)
    m1, v1, bp1 = g.adam_state()
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(np.asarray(bp0), np.asarray(bp1))
    _not_generic(capfd)


@pytest.mark.parametrize("bs", [256, 512])
@pytest.mark.parametrize("family", ["cartpole", "synth_c5"])
def test_dense_actor_and_critic_as_a_pair_on_the_two_learner_streams(gpu_ctx, capfd, family, bs):
    """One whole PPO iteration with actor and critic trained by one call: both chains are dense at these minibatch sizes, each with its own staging block and workspace."""
    res = parity.ppo_iteration_parity(n_envs=8, T=128, batch_size=bs, epochs=2, pair=True, family=family)
    assert res["ok"], res
    assert res["actor_batches"][0] == res["critic_batches"][0] == 2 * (1024 // bs)
    _not_generic(capfd)
