"""k_train_fs2's plain forms acknowledge their W2 stores inside dH1, and helper wave 4 + wt forms db2 of its (tile, half) behind its own acknowledgement
(csrc/train_fs2_kernel.h: EARLY_ACK, HELP_B2): the helper waves then write partial words that every wave's tail reads, and are counted at the B_2 meeting point. The
replica-group forms keep the parent's text, so the plain form against a group of one pins the moved block. No case names a build flag: the file passes on the parent's
library as well. Shapes, helpers and bars are those of test_gpu_fs2_helper_partials.py (2e-5 on theta / m / v, 2e-4 on the info columns; minibatches of 128, three epochs,
explicit permutations, Adam(0.01)); two buffer sizes, chosen for the words the helpers now write:
  200 rows: the ragged minibatch of 72 leaves invalid samples in both tiles of some workgroups;
  136 rows: the ragged minibatch of 8 leaves seven of the eight tiles, and three of the four workgroups, without a valid sample.
Per shape and size: (a) the plain form against the replica-group form of one rank, bit for bit; (b) against CRUX_FS=0 and the oracle; (c) max_batches = 3 ending
mid-epoch; (d) a NaN observation in minibatch 1 of epoch 0 -- code, state and rows are the sample-split learner's, and a second launch on the context gives a fresh run's bits."""
import ctypes as C

import numpy as np
import pytest

import parity
import replica_group as RG
from parity import L, O, crux
from test_gpu_fs2_helper_partials import BS, EPOCHS, EXTRAS, GLOSS, LR, P_PPO, SHAPES, WHAT, _bits, _check_state, _close, _cols, _pair, _state

pytestmark = pytest.mark.gpu

SIZES = (200, 136)
CASES = [(s, r) for s in SHAPES for r in SIZES]
IDS = ["%s-%d" % c for c in CASES]

_shards = {}
_plain = {}


def _shard(shape, rows, seed=947):
    """`rows` rows of an oracle rollout of the shape's policy (GAE, returns, whitened advantage), computed once and left unchanged"""
    if (shape, rows) in _shards:
        return _shards[(shape, rows)]
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    adims = dims if loss != "value_mse" else [od, 64, 64, ad]
    _, oa = parity.make_pair(adims, acts, 50, 0, "discrete" if disc else "gaussian", n_extra=0 if disc else ad, extra_init=-0.5)
    _, oc = parity.make_pair([od, 64, 64, 1], acts, 50, 1)
    E, T = 4, rows // 4
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, rows, EXTRAS)
    env = O.OEnv("cartpole", E, 60, 0.99, seed) if okind == "cartpole" else O.OEnv(okind, E, 60, 0.99, seed, so=od, sa=ad)
    env.rollout(oa, parity.rollout_cfg(head="categorical" if disc else "gaussian"), ob, T)
    ol = O.lib()
    O.chk(ol.orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(ol.orc_fill_returns(ob.h, 0.99)); O.chk(ol.orc_whiten(ob.h, L.COL["advantage"]))
    data = {k: ob[k].copy() for k in ob.keys()}
    _shards[(shape, rows)] = data
    return data


def _perms(rows, epochs, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(rows) for _ in range(epochs)])


def _launch(shape, rows, data, epochs, perms, fs, monkeypatch, max_batches=None):
    """one batch_train! launch through the library: (code, state, info, epoch rows)"""
    from crux_jl_amd import core
    monkeypatch.setenv("CRUX_FS", "1" if fs else "0")
    od, ad, disc = SHAPES[shape][:3]
    g, _ = _pair(shape)
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad), rows, EXTRAS); gb.push_(data)
    kw = {} if max_batches is None else {"max_batches": max_batches}
    opt = crux.TrainingParams(loss=GLOSS[SHAPES[shape][8]], optimizer=crux.Adam(LR), batch_size=BS, epochs=epochs, target_kl=None, name="n_", **kw)
    core._ensure_opt(g, opt)
    cfg = core._train_cfg(g, opt, P_PPO)
    pp = np.ascontiguousarray(np.asarray(perms, np.int64)); assert pp.shape == (epochs, rows)
    raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((epochs, L.INFO_N), np.float32)
    rc = g.ctx.lib.crux_batch_train(g.h, gb.h, C.byref(cfg), core._vp(pp), core._vp(raw), core._vp(ep))
    return int(rc), _state(g), raw, ep


def _oracle(shape, rows, data, epochs, perms):
    od, ad, disc, dims, acts, kind, head, okind, loss = SHAPES[shape]
    _, o = _pair(shape)
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, rows, EXTRAS); ob.push(data)
    o.adam_init(float(np.float32(LR)))
    cfg = parity.train_cfg(loss, head, BS, epochs, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32); oep = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(np.ascontiguousarray(perms, np.int64)), O.vpz(oi), O.vpz(oep)))
    om, ov, obp = o.adam_state()
    return [np.array(o.params, copy=True), om, ov, obp], oi, oep


def _plain_run(shape, rows, monkeypatch):
    """the plain learner's full run of a shape and size, launched once and shared by the cases"""
    if (shape, rows) not in _plain:
        rc, s, i, e = _launch(shape, rows, _shard(shape, rows), EPOCHS, _perms(rows, EPOCHS), True, monkeypatch)
        assert rc == L.OK and int(i[L.INFO["batches_trained"]]) == 2 * EPOCHS and int(i[L.INFO["epochs_run"]]) == EPOCHS
        _plain[(shape, rows)] = (s, i, e)
    return _plain[(shape, rows)]


@pytest.mark.parametrize("shape,rows", CASES, ids=IDS)
def test_the_plain_form_has_the_bits_of_a_group_of_one(gpu_ctx, monkeypatch, shape, rows):
    s2, i2, e2 = _plain_run(shape, rows, monkeypatch)
    RG.attach_or_skip([gpu_ctx])
    try:
        rc1, s1, i1, e1 = _launch(shape, rows, _shard(shape, rows), EPOCHS, _perms(rows, EPOCHS), True, monkeypatch)
    finally:
        gpu_ctx.peer_detach()
    assert rc1 == L.OK and int(i1[L.INFO["batches_trained"]]) == 2 * EPOCHS
    for x, y, what in zip(s2 + [i2, e2], s1 + [i1, e1], WHAT):
        assert _bits(x, y), (shape, rows, what, float(np.nanmax(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)))))


@pytest.mark.parametrize("shape,rows", CASES, ids=IDS)
def test_against_the_sample_split_learner_and_the_oracle(gpu_ctx, monkeypatch, shape, rows):
    data = _shard(shape, rows); perms = _perms(rows, EPOCHS)
    s2, i2, e2 = _plain_run(shape, rows, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, rows, data, EPOCHS, perms, False, monkeypatch)
    assert rc1 == L.OK and int(i1[L.INFO["batches_trained"]]) == 2 * EPOCHS
    so, oi, oep = _oracle(shape, rows, data, EPOCHS, perms)
    assert int(oi[L.INFO["batches_trained"]]) == 2 * EPOCHS
    tag = "%s / %d rows" % (shape, rows)
    _check_state(s2, s1, tag + " vs split:", True)
    _check_state(s2, so, tag + " vs oracle:", False)
    cols = _cols(shape)
    _close(e2[:, cols], e1[:, cols], tag + " epoch rows vs split:")
    _close(e2[:, cols], oep[:, cols], tag + " epoch rows vs oracle:")
    _close(i2[cols], i1[cols], tag + " info vs split:")


def _fresh_again(shape, rows, monkeypatch):
    """a launch on the context that has just ended early: the bits of the shared full run"""
    s2, i2, e2 = _plain_run(shape, rows, monkeypatch)
    rc, s, i, e = _launch(shape, rows, _shard(shape, rows), EPOCHS, _perms(rows, EPOCHS), True, monkeypatch)
    assert rc == L.OK
    for x, y, what in zip(s2 + [i2, e2], s + [i, e], WHAT):
        assert _bits(x, y), (shape, rows, "second launch", what)


@pytest.mark.parametrize("shape,rows", CASES, ids=IDS)
def test_max_batches_ends_the_launch_mid_epoch(gpu_ctx, monkeypatch, shape, rows):
    """max_batches = 3: both steps of epoch 0, then the full minibatch of epoch 1 -- the loop ends on a step in the middle of an epoch"""
    data = _shard(shape, rows); perms = _perms(rows, EPOCHS)
    _plain_run(shape, rows, monkeypatch)
    rc2, s2, i2, e2 = _launch(shape, rows, data, EPOCHS, perms, True, monkeypatch, max_batches=3)
    rc1, s1, i1, e1 = _launch(shape, rows, data, EPOCHS, perms, False, monkeypatch, max_batches=3)
    assert rc2 == rc1 == L.OK
    assert int(i2[L.INFO["batches_trained"]]) == int(i1[L.INFO["batches_trained"]]) == 3
    assert int(i2[L.INFO["epochs_run"]]) == int(i1[L.INFO["epochs_run"]]) == 2
    tag = "%s / %d rows" % (shape, rows)
    _check_state(s2, s1, tag + " vs split:", True)
    cols = _cols(shape)
    _close(i2[cols], i1[cols], tag + " info at max_batches vs split:")
    _close(e2[:2, cols], e1[:2, cols], tag + " epoch rows at max_batches vs split:")
    _fresh_again(shape, rows, monkeypatch)


@pytest.mark.parametrize("shape,rows", CASES, ids=IDS)
def test_a_suspect_step_in_minibatch_1_of_epoch_0(gpu_ctx, monkeypatch, shape, rows):
    clean = _shard(shape, rows); perms = _perms(rows, EPOCHS, seed=7)
    _plain_run(shape, rows, monkeypatch)
    data = dict(clean); data["s"] = clean["s"].copy(); data["s"][0, perms[0][BS + 5]] = np.nan
    rc2, s2, i2, e2 = _launch(shape, rows, data, EPOCHS, perms, True, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, rows, data, EPOCHS, perms, False, monkeypatch)
    assert rc2 == rc1 == L.ENAN
    # every parameter and moment: the bits of a run stopped after minibatch 0
    rcr, sr, _, _ = _launch(shape, rows, clean, 1, perms[:1], True, monkeypatch, max_batches=1)
    assert rcr == L.OK
    for x, y in zip(s2[:3], sr[:3]):
        assert _bits(x, y)
    assert np.any(s2[0] != _pair(shape)[0].get_params())
    tag = "%s / %d rows" % (shape, rows)
    _check_state(s2, s1, tag + " vs split:", True)
    assert np.isnan(i2[L.INFO["grad_norm"]]) == np.isnan(i1[L.INFO["grad_norm"]])
    if SHAPES[shape][3][2] == 64:      # (a 32-wide second layer has no sample-split learner: CRUX_FS=0 is the dense engine, which counts the failed minibatch in batches_trained)
        _close(i2, i1, tag + " info of the failed launch vs split:")
        _close(e2, e1, tag + " epoch rows of the failed launch vs split:")
    _fresh_again(shape, rows, monkeypatch)
