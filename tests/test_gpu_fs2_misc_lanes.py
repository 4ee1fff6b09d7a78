"""k_train_fs2's two maps of the small parameters (csrc/train_fs2_kernel.h, Fs2LayoutFor) on buffers of 200 rows with minibatches of 128 (one full and one ragged 72-row
minibatch per epoch), two epochs.
The misc-lane map -- b3 and log-sigma ride with the statistics in the tile's partial block and are owned by the lanes that carry them -- runs where it saves a round of dealt
parameters: 4-64-64-2 (512 + 2; plain and lagrange, with the cost lane behind b3) and 11-64-64-3 Gaussian (1024 + 6: b3 and log-sigma owned, the entropy term on log-sigma).
ONLY these three cases exercise the new code. The other shapes (4-64-64-1, 3-64-64-1, 8-64-64-4, 17-64-32-6) run the dealt map, whose instruction stream is the parent's: they pin the
other side of the layout flag on the same ragged problem, not the misc lanes. No instantiated shape that takes the misc map has more than 13 lanes (11-64-64-3); the 19-lane
block of a 17-x-x-6 Gaussian head does not occur, because those shapes save no round.
  * against the sample-split learner (CRUX_FS=0) and against the oracle: parameters, Adam state and the epoch info rows, under the bars of test_gpu_fs2.py;
  * a suspect (NaN) step puts b3 and log-sigma back like every other parameter: the bits of a run stopped one minibatch earlier;
  * a KL stop in the first epoch reports what the sample-split learner reports."""
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

# name: (obs, act, discrete, dims, activations, policy kind, head, oracle env kind, loss)
SHAPES = {
    "4-64-64-2-categorical": (4, 2, True, [4, 64, 64, 2], parity.ACTS, "discrete", "categorical", "cartpole", "ppo"),          # 514 small parameters: misc lanes, two rounds -> one
    "4-64-64-1-value": (4, 2, True, [4, 64, 64, 1], parity.ACTS, "continuous", "deterministic", "cartpole", "value_mse"),      # 449: one round either way, the dealt map
    "3-64-64-1-gaussian": (3, 1, False, [3, 64, 64, 1], parity.ACTS, "gaussian", "gaussian", "synth", "ppo"),                  # dealt map: b3, log-sigma and its entropy term in the round
    "8-64-64-4-categorical": (8, 4, True, [8, 64, 64, 4], parity.ACTS, "discrete", "categorical", "synth_discrete", "ppo"),    # 900: two rounds either way, the dealt map
    "11-64-64-3-gaussian": (11, 3, False, [11, 64, 64, 3], parity.ACTS, "gaussian", "gaussian", "synth", "ppo"),               # 1030: misc lanes, three rounds -> two; b3 and log-sigma owned, the entropy term
    "17-64-32-6-gaussian": (17, 6, False, [17, 64, 32, 6], ["tanh", "tanh", "identity"], "gaussian", "gaussian", "synth", "ppo"),      # the widest b3 | log-sigma block (12 words), H2 = 32, the dealt map
    "4-64-64-2-lagrange": (4, 2, True, [4, 64, 64, 2], parity.ACTS, "discrete", "categorical", "cartpole", "lagrange_ppo"),    # misc lanes: the cost lane behind b3
}
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
    _, oc = parity.make_pair([od, 64, dims[2], 1], acts, 50, 1)
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


def _pair(shape, seed=31):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    return parity.make_pair(dims, acts, seed, 0, kind, n_extra=ad if kind == "gaussian" else 0, extra_init=-0.5)


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


@pytest.mark.parametrize("shape", list(SHAPES))
def test_misc_owned_b3_and_logsigma_against_the_sample_split_learner_and_the_oracle(gpu_ctx, monkeypatch, shape):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    data = _shard(shape); perms = _perms()
    name = "n_"
    out = {}
    for form in ("fs2", "split"):
        monkeypatch.setenv("CRUX_FS", "1" if form == "fs2" else "0")
        g, _ = _pair(shape); gb, _ = _buffers(shape, data)
        info = crux.batch_train_(g, crux.TrainingParams(loss=GLOSS[loss], batch_size=BS, epochs=EPOCHS, name=name), _params(shape), gb, perms=perms + 1)
        out[form] = (_state(g), info)
    # the oracle: batch_train! on the same rows and shuffles
    _, o = _pair(shape); _, ob = _buffers(shape, data)
    o.adam_init(float(np.float32(3e-4)))
    cfg = parity.train_cfg(loss, head, BS, EPOCHS, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32); oep = np.zeros((EPOCHS, L.INFO_N), np.float32)
    op = O.vpz(np.ascontiguousarray(perms, np.int64))
    if loss == "lagrange_ppo":
        olag = _lag(); O.chk(O.lib().orc_batch_train_lagrange(o.h, ob.h, C.byref(cfg), C.byref(olag), op, O.vpz(oi), O.vpz(oep)))
    else:
        O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), op, O.vpz(oi), O.vpz(oep)))
    om, ov, obp = o.adam_state()
    (s2, i2), (s1, i1) = out["fs2"], out["split"]
    steps = EPOCHS * 2
    assert int(i2[name + "batches_trained"]) == int(i1[name + "batches_trained"]) == int(oi[L.INFO["batches_trained"]]) == steps
    _check_state(s2, s1, shape + " vs split:", True)
    _check_state(s2, [o.params, om, ov, obp], shape + " vs oracle:", False)
    cols = [L.INFO[k] for k in INFO_COLS] + ([L.INFO[k] for k in ("penalty", "cur_cost", "cost_loss", "p_loss")] if loss == "lagrange_ppo" else [])
    e2, e1 = np.asarray(i2["_epoch_infos"]), np.asarray(i1["_epoch_infos"])
    assert e2.shape[0] == e1.shape[0] == EPOCHS
    _close(e2[:, cols], e1[:, cols], shape + " epoch infos vs split:")
    _close(e2[:, cols], oep[:, cols], shape + " epoch infos vs oracle:")
    if kind == "gaussian":          # log-sigma moved: the entropy term reached it
        ls = s2[0][-ad:]
        assert np.all(ls != np.float32(-0.5)) and np.abs(ls - o.params[-ad:]).max() < 2e-5


@pytest.mark.parametrize("shape", ["4-64-64-2-categorical", "11-64-64-3-gaussian", "3-64-64-1-gaussian"])
def test_a_suspect_step_puts_b3_and_logsigma_back(gpu_ctx, shape):
    """one poisoned row in the second minibatch: the call fails with CRUX_ENAN (training.jl:20) and every parameter and moment -- b3 and log-sigma included -- has the bits of a
    run stopped after the first minibatch. The NaN sits in the row's observation, as in test_gpu_fs2.py: a NaN ADVANTAGE never makes a step suspect in the register-resident
    learners (the clipped surrogate's comparison, gsel = (u <= cl) ? A : 0, drops that sample's gradient; only the reported loss turns NaN), with or without the misc lanes."""
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
    for x, y in zip(got[:3], ref[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    nm = ad + (ad if kind == "gaussian" else 0)
    assert np.all(got[0][-nm:] != before[-nm:])          # the first step did move b3 (and log-sigma)


def test_kl_early_stop_reports_what_the_sample_split_learner_reports(gpu_ctx, monkeypatch):
    """target_kl = 0.05 with Adam(0.01): the oracle's KL of this problem is 0.023 at the full first minibatch and 0.128 at the ragged second one, so the first epoch stops
    after two steps; the reported minibatch is the ragged one, its statistics come through the misc lanes (wave 7's last seven threads, b3 with threads 0 and 1)"""
    shape = "4-64-64-2-categorical"; data = _shard(shape); perms = _perms()
    out = {}
    for form in ("fs2", "split"):
        monkeypatch.setenv("CRUX_FS", "1" if form == "fs2" else "0")
        g, _ = _pair(shape); gb, _ = _buffers(shape, data)
        opt = crux.TrainingParams(loss=crux.ppo_loss, optimizer=crux.Adam(0.01), batch_size=BS, epochs=EPOCHS, target_kl=0.05, name="n_")
        out[form] = crux.batch_train_(g, opt, _params(shape), gb, perms=perms + 1)
    i2, i1 = out["fs2"], out["split"]
    assert int(i2["n_batches_trained"]) == int(i1["n_batches_trained"]) == 2 and int(i2["_epochs_run"]) == int(i1["_epochs_run"]) == 1
    assert i2["kl"] > 0.05
    for k in ("kl", "entropy", "clip_fraction", "n_loss"):
        _close(i2[k], i1[k], k + " at the KL stop:")
    cols = [L.INFO[k] for k in INFO_COLS]
    _close(np.asarray(i2["_epoch_infos"])[:, cols], np.asarray(i1["_epoch_infos"])[:, cols], "epoch info row at the KL stop:")
