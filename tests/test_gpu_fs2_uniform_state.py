"""k_train_fs2 (csrc/train_fs2_kernel.h) reads the kernel arguments that a step does not need -- the network / Adam pointers, the status and epoch-info rows, the shuffle
arguments, the speculative-run word, the column pointers of the un-packed rows -- from the kernarg segment at the place of use, and keeps the packed rows' base and offsets in
the helper waves' vector registers. These cases walk every argument whose load moved, on the problem of test_gpu_fs2_misc_lanes.py: 200 rows, minibatches of 128 (one full and
one ragged 72-row minibatch per epoch), two epochs; the four learners of the benchmark (4-64-64-2 categorical, 4-64-64-1 value, 17-64-64-6 Gaussian tanh, 17-64-64-1 value tanh)
and 4-64-64-2 lagrange. Each case is held against the sample-split learner (CRUX_FS=0) and the oracle under the bars of test_gpu_fs2.py (2e-5 on parameters and moments, the
beta powers exactly / to 1e-12, 2e-4 on the info rows):
  (a) the default path: packed rows, the epoch orders composed ahead of the launch (explicit perms);
  (b) CRUX_PACK_ROWS=0: the column pointers;
  (c) the shuffle defined by seeds instead of explicit perms;
  (d) the pair call: the critic's order continues the actor's epochs;
  (e) max_batches ends the launch in the middle of the second epoch;
  (f) a KL stop in the first epoch;
  (g) a suspect (NaN observation) step leaves the bits of a run stopped one minibatch earlier.
The kernel's own composition of the orders (ord_all == NULL: order_a / order_b, perms, seeds, pre_epochs read inside the kernel) is not reachable through any public entry
for this kernel -- batch_train! and the pair call always compose ahead of the launch, and the multi-replica call, which does not, runs the one- / two-CU kernels -- so (c) and
(d) cover those arguments as far as the host forwards them."""
import ctypes as C

import numpy as np
import pytest

import parity
from parity import L, O, crux

pytestmark = pytest.mark.gpu

N_ROWS, BS, EPOCHS = 200, 128, 2
EXTRAS = ["return", "logprob", "advantage"]
LAG_EXTRAS = ["return", "advantage", "logprob", "cost_advantage", "cost", "cost_return"]
INFO_COLS = ("loss", "grad_norm", "entropy", "kl", "clip_fraction", "avg_advantage", "avg_return")
TANH = ["tanh", "tanh", "identity"]

# name: (obs, act, discrete, dims, activations, policy kind, head, oracle env kind, loss)
SHAPES = {
    "4-64-64-2-categorical": (4, 2, True, [4, 64, 64, 2], parity.ACTS, "discrete", "categorical", "cartpole", "ppo"),
    "4-64-64-1-value": (4, 2, True, [4, 64, 64, 1], parity.ACTS, "continuous", "deterministic", "cartpole", "value_mse"),
    "17-64-64-6-gaussian-tanh": (17, 6, False, [17, 64, 64, 6], TANH, "gaussian", "gaussian", "synth", "ppo"),
    "17-64-64-1-value-tanh": (17, 6, False, [17, 64, 64, 1], TANH, "continuous", "deterministic", "synth", "value_mse"),
    "4-64-64-2-lagrange": (4, 2, True, [4, 64, 64, 2], parity.ACTS, "discrete", "categorical", "cartpole", "lagrange_ppo"),
}
PLAIN = [s for s in SHAPES if not s.endswith("lagrange")]
GLOSS = {"ppo": crux.ppo_loss, "value_mse": crux.value_mse_loss, "lagrange_ppo": crux.lagrange_ppo_loss}

_shards = {}


def _shard(shape, seed=940):
    """200 rows of an oracle rollout of the shape's policy (GAE, returns, whitened advantage; the lagrange shape with its cost columns), computed once and left unchanged"""
    if (shape, seed) in _shards:
        return _shards[(shape, seed)]
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    lag = loss == "lagrange_ppo"
    adims = dims if loss != "value_mse" else [od, 64, 64, ad]
    _, oa = parity.make_pair(adims, acts, 50, 0, "discrete" if disc else "gaussian", n_extra=0 if disc else ad, extra_init=-0.5)
    _, oc = parity.make_pair([od, 64, 64, 1], acts, 50, 1)
    extras = LAG_EXTRAS if lag else EXTRAS
    E, T = 4, N_ROWS // 4
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, E * T, extras)
    env = O.OEnv("cartpole", E, 12 if lag else 60, 0.99, seed) if okind == "cartpole" else O.OEnv(okind, E, 60, 0.99, seed, so=od, sa=ad)
    env.rollout(oa, parity.rollout_cfg(head="categorical" if disc else "gaussian"), ob, T)
    ol = O.lib()
    O.chk(ol.orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(ol.orc_fill_returns(ob.h, 0.99))
    if lag:
        _, ov = parity.make_pair([od, 64, 64, 1], acts, 50, 2)
        O.chk(ol.orc_fill_gae_keys(ob.h, ov.h, 0.95, 0.99, L.COL["cost"], L.COL["cost_advantage"])); O.chk(ol.orc_fill_returns_keys(ob.h, 0.99, L.COL["cost"], L.COL["cost_return"]))
    O.chk(ol.orc_whiten(ob.h, L.COL["advantage"]))
    data = {k: ob[k].copy() for k in ob.keys()}
    _shards[(shape, seed)] = data
    return data


def _pair(shape, seed=31, stream=0):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    return parity.make_pair(dims, acts, seed, stream, kind, n_extra=ad if kind == "gaussian" else 0, extra_init=-0.5)


def _buffers(shape, data):
    od, ad, disc = SHAPES[shape][:3]
    extras = LAG_EXTRAS if SHAPES[shape][8] == "lagrange_ppo" else EXTRAS
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad), N_ROWS, extras); gb.push_(data)
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, N_ROWS, extras); ob.push(data)
    return gb, ob


def _lag():
    g = L.Lagrange(); g.target_cost, g.penalty_max, g.Ki_max, g.Ki, g.Kp, g.Kd, g.ema_alpha = 0.05, np.inf, 10.0, 1e-3, 1.0, 0.5, 0.95
    return g


def _params(shape):
    P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
    if SHAPES[shape][8] == "lagrange_ppo":
        P["lagrange"] = _lag()
    return P


def _state(net):
    m, v, bp = net.adam_state()
    return [net.get_params(), m, v, bp]


def _perms(seed=5, epochs=EPOCHS):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N_ROWS) for _ in range(epochs)])


def _close(a, b, what):
    """the info bar of test_gpu_fs2.py: 2e-4 relative (absolute below 1)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    print(what, "max |d| = %.3g" % float(np.abs(a - b).max()))
    assert np.all(np.abs(a - b) <= 2e-4 * np.maximum(1.0, np.abs(b))), (what, a, b)


def _check_state(got, ref, what, exact_bp):
    d = [float(np.abs(got[i] - ref[i]).max()) for i in range(3)]
    print(what, "max |dtheta| = %.3g, |dm| = %.3g, |dv| = %.3g" % tuple(d))
    assert d[0] < 2e-5 and d[1] <= 2e-5 and d[2] <= 2e-5, (what, d)          # the parameter / moment bars of test_gpu_fs2.py
    assert np.array_equal(got[3], ref[3]) if exact_bp else np.allclose(got[3], ref[3], rtol=1e-12), what


def _same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def _three_ways(monkeypatch, shape, steps, epochs_run, fs2_env=(), perms=None, seed=None, max_batches=0, target_kl=None, lr=None):
    """one batch_train! call on k_train_fs2 (with the switches of fs2_env), on the sample-split learner and in the oracle: parameters, Adam state, beta powers, the epoch info
    rows and what the launch status carries (minibatches trained, epochs run)"""
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    data = _shard(shape); name = "n_"
    kw = {} if lr is None else {"optimizer": crux.Adam(lr)}
    if seed is not None:
        kw["shuffle_seed"] = seed
    out = {}
    for form in ("fs2", "split"):
        monkeypatch.setenv("CRUX_FS", "1" if form == "fs2" else "0")
        for k, v in fs2_env:
            if form == "fs2":
                monkeypatch.setenv(k, v)
            else:
                monkeypatch.delenv(k, raising=False)
        g, _ = _pair(shape); gb, _ = _buffers(shape, data)
        opt = crux.TrainingParams(loss=GLOSS[loss], batch_size=BS, epochs=EPOCHS, max_batches=max_batches or None, target_kl=target_kl, name=name, **kw)
        info = crux.batch_train_(g, opt, _params(shape), gb, **({} if perms is None else {"perms": perms + 1}))
        out[form] = (_state(g), info)
    _, o = _pair(shape); _, ob = _buffers(shape, data)
    o.adam_init(float(np.float32(3e-4 if lr is None else lr)))
    cfg = parity.train_cfg(loss, head, BS, EPOCHS, -1.0 if target_kl is None else target_kl, 0 if seed is None else seed, 0, max_batches)
    oi = np.zeros(L.INFO_N, np.float32); oep = np.zeros((EPOCHS, L.INFO_N), np.float32)
    op = None if perms is None else O.vpz(np.ascontiguousarray(perms, np.int64))
    if loss == "lagrange_ppo":
        olag = _lag(); O.chk(O.lib().orc_batch_train_lagrange(o.h, ob.h, C.byref(cfg), C.byref(olag), op, O.vpz(oi), O.vpz(oep)))
    else:
        O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), op, O.vpz(oi), O.vpz(oep)))
    om, ov, obp = o.adam_state()
    (s2, i2), (s1, i1) = out["fs2"], out["split"]
    assert int(i2[name + "batches_trained"]) == int(i1[name + "batches_trained"]) == int(oi[L.INFO["batches_trained"]]) == steps
    assert int(i2["_epochs_run"]) == int(i1["_epochs_run"]) == epochs_run
    _check_state(s2, s1, shape + " vs split:", True)
    _check_state(s2, [o.params, om, ov, obp], shape + " vs oracle:", False)
    cols = [L.INFO[k] for k in INFO_COLS] + ([L.INFO[k] for k in ("penalty", "cur_cost", "cost_loss", "p_loss")] if loss == "lagrange_ppo" else [])
    e2, e1 = np.asarray(i2["_epoch_infos"]), np.asarray(i1["_epoch_infos"])
    assert e2.shape[0] == e1.shape[0] == epochs_run
    _close(e2[:, cols], e1[:, cols], shape + " epoch infos vs split:")
    _close(e2[:, cols], oep[:epochs_run][:, cols], shape + " epoch infos vs oracle:")
    return s2, i2


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_packed_rows_and_orders_composed_ahead(gpu_ctx, monkeypatch, shape):
    _three_ways(monkeypatch, shape, 2 * EPOCHS, EPOCHS, perms=_perms())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_b_column_pointers_without_packed_rows(gpu_ctx, monkeypatch, shape):
    """CRUX_PACK_ROWS=0: the helper waves gather s, a, logprob, advantage and return from the buffer's columns. The same rows in the same order: the bits of the packed form."""
    s0, _ = _three_ways(monkeypatch, shape, 2 * EPOCHS, EPOCHS, fs2_env=(("CRUX_PACK_ROWS", "0"),), perms=_perms())
    monkeypatch.setenv("CRUX_FS", "1"); monkeypatch.delenv("CRUX_PACK_ROWS", raising=False)
    g, _ = _pair(shape); gb, _ = _buffers(shape, _shard(shape))
    crux.batch_train_(g, crux.TrainingParams(loss=GLOSS[SHAPES[shape][8]], batch_size=BS, epochs=EPOCHS, name="n_"), _params(shape), gb, perms=_perms() + 1)
    assert _same_bits(s0[:3], _state(g)[:3]) and np.array_equal(s0[3], _state(g)[3])


@pytest.mark.parametrize("shape", ["4-64-64-2-categorical", "17-64-64-6-gaussian-tanh", "17-64-64-1-value-tanh"])
def test_c_the_shuffle_from_seeds(gpu_ctx, monkeypatch, shape):
    """no explicit perms: every epoch's order is Philox(shuffle_seed, counter + epoch), composed ahead of the launch; (a) has the explicit perms"""
    _three_ways(monkeypatch, shape, 2 * EPOCHS, EPOCHS, seed=17)


def test_d_the_critic_continues_the_actors_epochs(gpu_ctx, monkeypatch):
    """the pair call (actor || critic on the two learner streams): the critic's epoch orders are composed onto the actor's last one. On k_train_fs2 it leaves the bits of the two
    calls made one after the other on k_train_fs2, and what the sample-split learners leave to 2e-5."""
    sa, sc = "4-64-64-2-categorical", "4-64-64-1-value"; data = _shard(sa); P = _params(sa)

    def opts():          # (fresh for every run: a TrainingParams counts the shuffles it has handed out)
        return (crux.TrainingParams(loss=crux.ppo_loss, batch_size=BS, epochs=EPOCHS, name="actor_", shuffle_seed=3),
                crux.TrainingParams(loss=crux.value_mse_loss, batch_size=BS, epochs=EPOCHS, name="critic_", shuffle_seed=4))
    out = {}
    for form in ("fs2", "split"):
        monkeypatch.setenv("CRUX_FS", "1" if form == "fs2" else "0")
        a, _ = _pair(sa, stream=0); c, _ = _pair(sc, stream=1); gb, _ = _buffers(sa, data)

        class _S:
            pass
        s = _S(); s.agent = crux.PolicyParams(crux.ActorCritic(a, c)); s.P = P; s.a_opt, s.c_opt = opts()
        info = crux.policy_gradient_training(s, gb)
        out[form] = (_state(a), _state(c), info, gb["s"])
    f2, f1 = out["fs2"], out["split"]
    assert f2[2]["actor_batches_trained"] == f1[2]["actor_batches_trained"] == 2 * EPOCHS and f2[2]["critic_batches_trained"] == f1[2]["critic_batches_trained"] == 2 * EPOCHS
    _check_state(f2[0], f1[0], "pair actor vs split:", True); _check_state(f2[1], f1[1], "pair critic vs split:", True)
    assert np.array_equal(f2[3], f1[3])          # the buffer's row order after both learners
    i2, i1 = f2[2], f1[2]
    assert set(i2) == set(i1)
    for k in i2:          # the launch status words (minibatches trained, epochs run) exactly; the reported statistics and epoch info rows under the info bar
        v2, v1 = np.asarray(i2[k], np.float64), np.asarray(i1[k], np.float64)
        assert v2.shape == v1.shape, (k, v2.shape, v1.shape)
        if k.endswith("epochs_run") or k.endswith("batches_trained"):
            assert np.array_equal(v2, v1), (k, v2, v1)
        else:
            assert np.array_equal(np.isnan(v2), np.isnan(v1)), (k, v2, v1)
            _close(np.nan_to_num(v2), np.nan_to_num(v1), "pair " + k + " vs split:")
    monkeypatch.setenv("CRUX_FS", "1")
    a, _ = _pair(sa, stream=0); c, _ = _pair(sc, stream=1); gb, _ = _buffers(sa, data)
    a_opt, c_opt = opts()
    crux.batch_train_(a, a_opt, P, gb); crux.batch_train_(c, c_opt, P, gb)
    assert _same_bits(_state(a)[:3], f2[0][:3]) and _same_bits(_state(c)[:3], f2[1][:3]) and np.array_equal(gb["s"], f2[3])
    assert np.array_equal(_state(a)[3], f2[0][3]) and np.array_equal(_state(c)[3], f2[1][3])


@pytest.mark.parametrize("shape", ["4-64-64-2-categorical", "17-64-64-1-value-tanh", "4-64-64-2-lagrange"])
def test_e_max_batches_ends_the_launch_inside_the_second_epoch(gpu_ctx, monkeypatch, shape):
    _three_ways(monkeypatch, shape, 3, EPOCHS, perms=_perms(), max_batches=3)


def test_f_a_kl_stop_in_the_first_epoch(gpu_ctx, monkeypatch):
    """target_kl = 0.05 with Adam(0.01) on this problem (test_gpu_fs2_misc_lanes.py: the KL is 0.023 at the full first minibatch and 0.128 at the ragged second one): the first
    epoch ends after its two steps and no second one starts"""
    _, i2 = _three_ways(monkeypatch, "4-64-64-2-categorical", 2, 1, perms=_perms(), target_kl=0.05, lr=0.01)
    assert i2["kl"] > 0.05


@pytest.mark.parametrize("shape", PLAIN)
def test_g_a_suspect_step_leaves_the_bits_of_the_step_before(gpu_ctx, shape):
    """a NaN observation in the second minibatch: CRUX_ENAN in the launch status, and parameters and Adam state with the bits of a run stopped after the first minibatch"""
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    clean = _shard(shape); perm = _perms(7, 1)[0]
    data = dict(clean); data["s"] = clean["s"].copy(); data["s"][0, perm[BS + 5]] = np.nan
    P = _params(shape)
    g, _ = _pair(shape); gb, _ = _buffers(shape, data)
    with pytest.raises(crux.CruxError) as e:
        crux.batch_train_(g, crux.TrainingParams(loss=GLOSS[loss], batch_size=BS, epochs=EPOCHS, name="n_"), P, gb, perms=np.stack([perm, perm]) + 1)
    assert e.value.code == L.ENAN
    got = _state(g)
    g1, _ = _pair(shape); gb1, _ = _buffers(shape, clean)
    before = g1.get_params()
    crux.batch_train_(g1, crux.TrainingParams(loss=GLOSS[loss], batch_size=BS, epochs=1, max_batches=1, name="n_"), P, gb1, perms=perm[None, :] + 1)
    ref = _state(g1)
    assert _same_bits(got[:3], ref[:3])
    assert np.array_equal(got[3], ref[3])    # the beta powers: one step's
    assert np.any(got[0] != before)          # the first step did train
