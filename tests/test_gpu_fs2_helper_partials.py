"""k_train_fs2's plain forms form two of the compute waves' small partials later in the step than the other forms do: the dW3 partials behind the wave's acknowledgement of
its W2 stores, from a register copy of h2 (not in front of B_1), and db2 between the dW2 stores and dH1 (csrc/train_fs2_kernel.h: LATE_W3, LATE_B2; the helper waves forming
them, which this file is named after, was measured and not adopted: DESIGN 4.1). The replica-group forms keep the parent's text. The helpers and the bars are those of
test_gpu_fs2_report_steps.py; buffers of 200 rows (128 + 72: the ragged minibatch leaves invalid samples in both tiles of some workgroups), minibatches of 128, three
epochs, explicit permutations, Adam(0.01):
  (a) the plain learner against the replica-group form of ONE rank (attached as bench.py's selftest does, through tests/replica_group.py): DESIGN 4.1 holds that every form of
      the kernel produces the same bits -- theta, m, v, beta powers, info and epoch rows;
  (b) against the sample-split learner (CRUX_FS=0) and the oracle: 2e-5 on theta / m / v, 2e-4 on the info columns;
  (c) max_batches ending mid-epoch, and a suspect step (a NaN observation placed by the order in minibatch 1 of epoch 0): code, state and rows are the sample-split
      learner's, the launch returns, and a second launch on the same context gives the bits of a fresh one.
Shapes: 4-64-64-2 categorical relu (misc map, two b3 words), 4-64-64-1 value, 3-64-64-1 Gaussian (dealt map), 17-64-64-6 Gaussian tanh (three dW3 passes, statistics on
every step), 17-64-32-6 Gaussian tanh (one 16-feature tile per half, two passes; CRUX_FS=0 is the dense engine there)."""
import ctypes as C

import numpy as np
import pytest

import parity
import replica_group as RG
from parity import L, O, crux

pytestmark = pytest.mark.gpu

BS = 128
LR = 0.01
ROWS = 200
EPOCHS = 3
EXTRAS = ["return", "logprob", "advantage"]
INFO_COLS = ("loss", "grad_norm", "entropy", "kl", "clip_fraction", "avg_advantage", "avg_return")
TANH = ["tanh", "tanh", "identity"]

# name: (obs, act, discrete, dims, activations, policy kind, head, oracle env kind, loss)
SHAPES = {
    "4-64-64-2-categorical": (4, 2, True, [4, 64, 64, 2], parity.ACTS, "discrete", "categorical", "cartpole", "ppo"),
    "4-64-64-1-value": (4, 2, True, [4, 64, 64, 1], parity.ACTS, "continuous", "deterministic", "cartpole", "value_mse"),
    "3-64-64-1-gaussian": (3, 1, False, [3, 64, 64, 1], parity.ACTS, "gaussian", "gaussian", "synth", "ppo"),
    "17-64-64-6-gaussian-tanh": (17, 6, False, [17, 64, 64, 6], TANH, "gaussian", "gaussian", "synth", "ppo"),
    "17-64-32-6-gaussian-tanh": (17, 6, False, [17, 64, 32, 6], TANH, "gaussian", "gaussian", "synth", "ppo"),
}
GLOSS = {"ppo": crux.ppo_loss, "value_mse": crux.value_mse_loss}
P_PPO = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
WHAT = ("theta", "m", "v", "beta powers", "info", "epoch rows")

_shards = {}


def _shard(shape, seed=947):
    """ROWS rows of an oracle rollout of the shape's policy (GAE, returns, whitened advantage), computed once and left unchanged"""
    if (shape, seed) in _shards:
        return _shards[(shape, seed)]
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    adims = dims if loss != "value_mse" else [od, 64, 64, ad]
    _, oa = parity.make_pair(adims, acts, 50, 0, "discrete" if disc else "gaussian", n_extra=0 if disc else ad, extra_init=-0.5)
    _, oc = parity.make_pair([od, 64, 64, 1], acts, 50, 1)
    E, T = 4, ROWS // 4
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, ROWS, EXTRAS)
    env = O.OEnv("cartpole", E, 60, 0.99, seed) if okind == "cartpole" else O.OEnv(okind, E, 60, 0.99, seed, so=od, sa=ad)
    env.rollout(oa, parity.rollout_cfg(head="categorical" if disc else "gaussian"), ob, T)
    ol = O.lib()
    O.chk(ol.orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(ol.orc_fill_returns(ob.h, 0.99)); O.chk(ol.orc_whiten(ob.h, L.COL["advantage"]))
    data = {k: ob[k].copy() for k in ob.keys()}
    _shards[(shape, seed)] = data
    return data


def _pair(shape, seed=31):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    return parity.make_pair(dims, acts, seed, 0, kind, n_extra=ad if kind == "gaussian" else 0, extra_init=-0.5)


def _perms(epochs, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(ROWS) for _ in range(epochs)])


def _state(net):
    m, v, bp = net.adam_state()
    return [net.get_params(), m, v, bp]


def _launch(shape, data, epochs, perms, fs, monkeypatch, max_batches=None):
    """one batch_train! launch through the library, so that the code, the info and the epoch rows are there after a failure too: (code, state, info, epoch rows)"""
    from crux_jl_amd import core
    monkeypatch.setenv("CRUX_FS", "1" if fs else "0")
    od, ad, disc = SHAPES[shape][:3]
    g, _ = _pair(shape)
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad), ROWS, EXTRAS); gb.push_(data)
    kw = {} if max_batches is None else {"max_batches": max_batches}
    opt = crux.TrainingParams(loss=GLOSS[SHAPES[shape][8]], optimizer=crux.Adam(LR), batch_size=BS, epochs=epochs, target_kl=None, name="n_", **kw)
    core._ensure_opt(g, opt)
    cfg = core._train_cfg(g, opt, P_PPO)
    pp = np.ascontiguousarray(np.asarray(perms, np.int64)); assert pp.shape == (epochs, ROWS)
    raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((epochs, L.INFO_N), np.float32)
    rc = g.ctx.lib.crux_batch_train(g.h, gb.h, C.byref(cfg), core._vp(pp), core._vp(raw), core._vp(ep))
    return int(rc), _state(g), raw, ep


def _oracle(shape, data, epochs, perms):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    _, o = _pair(shape)
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, ROWS, EXTRAS); ob.push(data)
    o.adam_init(float(np.float32(LR)))
    cfg = parity.train_cfg(loss, head, BS, epochs, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32); oep = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(np.ascontiguousarray(perms, np.int64)), O.vpz(oi), O.vpz(oep)))
    om, ov, obp = o.adam_state()
    return [np.array(o.params, copy=True), om, ov, obp], oi, oep      # (a copy: the oracle network does not outlive this call)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _close(a, b, what):
    """the info bar of test_gpu_fs2_report_steps.py: 2e-4 relative (absolute below 1); NaN where the reference has NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    f = ~np.isnan(b)
    print(what, "max |d| = %.3g" % (float(np.abs(a[f] - b[f]).max()) if f.any() else 0.0))
    assert np.all(np.abs(a[f] - b[f]) <= 2e-4 * np.maximum(1.0, np.abs(b[f]))), (what, a, b)


def _check_state(got, ref, what, exact_bp):
    """the parameter / moment bars of test_gpu_fs2_report_steps.py"""
    d = [float(np.abs(got[i] - ref[i]).max()) for i in range(3)]
    print(what, "max |dtheta| = %.3g, |dm| = %.3g, |dv| = %.3g" % tuple(d))
    assert d[0] < 2e-5 and d[1] <= 2e-5 and d[2] <= 2e-5, (what, d)
    assert np.array_equal(got[3], ref[3]) if exact_bp else np.allclose(got[3], ref[3], rtol=1e-12), what


def _cols(shape):
    return [L.INFO[k] for k in (INFO_COLS if SHAPES[shape][8] != "value_mse" else ("loss", "grad_norm"))]


_plain = {}


def _plain_run(shape, monkeypatch):
    """the plain learner's full run of a shape, launched once and shared by (a) and (b)"""
    if shape not in _plain:
        rc, s, i, e = _launch(shape, _shard(shape), EPOCHS, _perms(EPOCHS), True, monkeypatch)
        assert rc == L.OK and int(i[L.INFO["batches_trained"]]) == 2 * EPOCHS and int(i[L.INFO["epochs_run"]]) == EPOCHS
        _plain[shape] = (s, i, e)
    return _plain[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_plain_form_has_the_bits_of_a_group_of_one(gpu_ctx, monkeypatch, shape):
    s2, i2, e2 = _plain_run(shape, monkeypatch)
    RG.attach_or_skip([gpu_ctx])
    try:
        rc1, s1, i1, e1 = _launch(shape, _shard(shape), EPOCHS, _perms(EPOCHS), True, monkeypatch)
    finally:
        gpu_ctx.peer_detach()
    assert rc1 == L.OK and int(i1[L.INFO["batches_trained"]]) == 2 * EPOCHS
    for x, y, what in zip(s2 + [i2, e2], s1 + [i1, e1], WHAT):
        assert _bits(x, y), (shape, what, float(np.nanmax(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)))))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_sample_split_learner_and_the_oracle(gpu_ctx, monkeypatch, shape):
    data = _shard(shape); perms = _perms(EPOCHS)
    s2, i2, e2 = _plain_run(shape, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, data, EPOCHS, perms, False, monkeypatch)
    assert rc1 == L.OK and int(i1[L.INFO["batches_trained"]]) == 2 * EPOCHS
    so, oi, oep = _oracle(shape, data, EPOCHS, perms)
    assert int(oi[L.INFO["batches_trained"]]) == 2 * EPOCHS
    _check_state(s2, s1, shape + " vs split:", True)
    _check_state(s2, so, shape + " vs oracle:", False)
    cols = _cols(shape)
    _close(e2[:, cols], e1[:, cols], shape + " epoch rows vs split:")
    _close(e2[:, cols], oep[:, cols], shape + " epoch rows vs oracle:")
    _close(i2[cols], i1[cols], shape + " info vs split:")


def _fresh_again(shape, monkeypatch):
    """a launch on the context that has just ended early: the bits of the shared full run"""
    s2, i2, e2 = _plain_run(shape, monkeypatch)
    rc, s, i, e = _launch(shape, _shard(shape), EPOCHS, _perms(EPOCHS), True, monkeypatch)
    assert rc == L.OK
    for x, y, what in zip(s2 + [i2, e2], s + [i, e], WHAT):
        assert _bits(x, y), (shape, "second launch", what)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_max_batches_ends_the_launch_mid_epoch(gpu_ctx, monkeypatch, shape):
    """max_batches = 3: both steps of epoch 0, then the full minibatch of epoch 1 -- the loop ends on a step in the middle of an epoch"""
    data = _shard(shape); perms = _perms(EPOCHS)
    _plain_run(shape, monkeypatch)
    rc2, s2, i2, e2 = _launch(shape, data, EPOCHS, perms, True, monkeypatch, max_batches=3)
    rc1, s1, i1, e1 = _launch(shape, data, EPOCHS, perms, False, monkeypatch, max_batches=3)
    assert rc2 == rc1 == L.OK
    assert int(i2[L.INFO["batches_trained"]]) == int(i1[L.INFO["batches_trained"]]) == 3
    assert int(i2[L.INFO["epochs_run"]]) == int(i1[L.INFO["epochs_run"]]) == 2
    _check_state(s2, s1, shape + " vs split:", True)
    cols = _cols(shape)
    _close(i2[cols], i1[cols], shape + " info at max_batches vs split:")
    _close(e2[:2, cols], e1[:2, cols], shape + " epoch rows at max_batches vs split:")
    _fresh_again(shape, monkeypatch)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_suspect_step_in_minibatch_1_of_epoch_0(gpu_ctx, monkeypatch, shape):
    clean = _shard(shape); perms = _perms(EPOCHS, seed=7)
    _plain_run(shape, monkeypatch)
    data = dict(clean); data["s"] = clean["s"].copy(); data["s"][0, perms[0][BS + 5]] = np.nan
    rc2, s2, i2, e2 = _launch(shape, data, EPOCHS, perms, True, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, data, EPOCHS, perms, False, monkeypatch)
    assert rc2 == rc1 == L.ENAN
    # every parameter and moment: the bits of a run stopped after minibatch 0
    rcr, sr, _, _ = _launch(shape, clean, 1, perms[:1], True, monkeypatch, max_batches=1)
    assert rcr == L.OK
    for x, y in zip(s2[:3], sr[:3]):
        assert _bits(x, y)
    assert np.any(s2[0] != _pair(shape)[0].get_params())
    _check_state(s2, s1, shape + " vs split:", True)
    assert np.isnan(i2[L.INFO["grad_norm"]]) == np.isnan(i1[L.INFO["grad_norm"]])
    if SHAPES[shape][3][2] == 64:      # (a 32-wide second layer has no sample-split learner: CRUX_FS=0 is the dense engine, which counts the failed minibatch in batches_trained)
        _close(i2, i1, shape + " info of the failed launch vs split:")
        _close(e2, e1, shape + " epoch rows of the failed launch vs split:")
    _fresh_again(shape, monkeypatch)
