"""k_train_fs2's plain forms form the loss head's seven statistics sums only on a step that may be read -- the epoch's last minibatch, the one max_batches ends on, every step
while KL stopping is on, every step of the launch's first epoch (a suspect step there reports its own loss) -- and total / update a wave's two W2 tiles one after the other
(csrc/train_fs2_kernel.h: STAT_SKIP, W2_TILED). Buffers of 328 rows (128 + 128 + 72: two steps that report nothing and a ragged one that does, per epoch), minibatches of
128, three epochs, Adam(0.01), explicit permutations:
  (a) target_kl = None against target_kl = 1e30 (statistics on every step, never stops: the every-step path inside the same kernel): the same BITS in parameters, Adam state,
      the info and the epoch rows; the values themselves against the sample-split learner (CRUX_FS=0) and the oracle under the bars of test_gpu_fs2_misc_lanes.py.
      4-64-64-2 categorical (misc map, 2 gradient words), 4-64-64-1 value (1; KL stopping does not exist for a value head: its twin pins the dispatch only), 3-64-64-1 Gaussian
      (dealt map, 2 words), 17-64-64-6 Gaussian (12 words: the reduce-scatter on every step, the path unchanged);
  (b) max_batches = 4: the report falls on the first step of epoch 1, mid-epoch; info and rows are the sample-split learner's;
  (c) a row that makes a step suspect, placed by the order in minibatch 1 of epoch 0: CRUX_ENAN, parameters and Adam state the bits of a run stopped one minibatch earlier,
      the info, the epoch row and the code those of the sample-split learner. The NaN sits in the row's OBSERVATION (as in test_a_suspect_step_puts_b3_and_logsigma_back): a
      NaN ADVANTAGE never makes a step of these learners suspect -- gsel = (u <= cl) ? A : 0 drops the sample's gradient, only a reported loss turns NaN. That case runs
      too: the orders put the row in minibatch 1 of epochs 0 and 1 (no report, from epoch 1 on no statistics) and in the reporting minibatch of epoch 2; code, NaN pattern
      and values are the sample-split learner's. A suspect step in epoch 1 cannot be built from the data: every row is visited in every epoch, so a row that poisons a step
      ends the launch in epoch 0;
  (d) the tile order of the W2 update on 200 rows (128 + 72), five epochs, against CRUX_FS=0 and the oracle."""
import ctypes as C

import numpy as np
import pytest

import parity
from parity import L, O, crux

pytestmark = pytest.mark.gpu

BS = 128
LR = 0.01
EXTRAS = ["return", "logprob", "advantage"]
INFO_COLS = ("loss", "grad_norm", "entropy", "kl", "clip_fraction", "avg_advantage", "avg_return")

# name: (obs, act, discrete, dims, policy kind, head, oracle env kind, loss)
SHAPES = {
    "4-64-64-2-categorical": (4, 2, True, [4, 64, 64, 2], "discrete", "categorical", "cartpole", "ppo"),
    "4-64-64-1-value": (4, 2, True, [4, 64, 64, 1], "continuous", "deterministic", "cartpole", "value_mse"),
    "3-64-64-1-gaussian": (3, 1, False, [3, 64, 64, 1], "gaussian", "gaussian", "synth", "ppo"),
    "17-64-64-6-gaussian": (17, 6, False, [17, 64, 64, 6], "gaussian", "gaussian", "synth", "ppo"),
}
GLOSS = {"ppo": crux.ppo_loss, "value_mse": crux.value_mse_loss}
P_PPO = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}

_shards = {}


def _shard(shape, n_rows, seed=941):
    """n_rows of an oracle rollout of the shape's policy (GAE, returns, whitened advantage), computed once and left unchanged"""
    if (shape, n_rows, seed) in _shards:
        return _shards[(shape, n_rows, seed)]
    od, ad, disc, dims, kind, head, okind, loss = SHAPES[shape]
    adims = dims if loss != "value_mse" else [od, 64, 64, ad]
    _, oa = parity.make_pair(adims, parity.ACTS, 50, 0, "discrete" if disc else "gaussian", n_extra=0 if disc else ad, extra_init=-0.5)
    _, oc = parity.make_pair([od, 64, 64, 1], parity.ACTS, 50, 1)
    E, T = 4, n_rows // 4
    assert E * T == n_rows
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, n_rows, EXTRAS)
    env = O.OEnv("cartpole", E, 60, 0.99, seed) if okind == "cartpole" else O.OEnv(okind, E, 60, 0.99, seed, so=od, sa=ad)
    env.rollout(oa, parity.rollout_cfg(head="categorical" if disc else "gaussian"), ob, T)
    ol = O.lib()
    O.chk(ol.orc_fill_gae(ob.h, oc.h, 0.95, 0.99)); O.chk(ol.orc_fill_returns(ob.h, 0.99)); O.chk(ol.orc_whiten(ob.h, L.COL["advantage"]))
    data = {k: ob[k].copy() for k in ob.keys()}
    _shards[(shape, n_rows, seed)] = data
    return data


def _pair(shape, seed=31):
    od, ad, disc, dims, kind, head, okind, loss = SHAPES[shape]
    return parity.make_pair(dims, parity.ACTS, seed, 0, kind, n_extra=ad if kind == "gaussian" else 0, extra_init=-0.5)


def _gbuf(shape, data, n_rows):
    od, ad, disc = SHAPES[shape][:3]
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad), n_rows, EXTRAS); gb.push_(data)
    return gb


def _obuf(shape, data, n_rows):
    od, ad, disc = SHAPES[shape][:3]
    ob = O.OBuffer(od, ad, L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS, n_rows, EXTRAS); ob.push(data)
    return ob


def _perms(n_rows, epochs, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n_rows) for _ in range(epochs)])


def _perms_for_orders(orders):
    """the per-epoch permutations whose composition (order_e[j] = order_{e-1}[perm_e[j]], order_{-1} = identity: experience_buffer.jl:118-124) visits the rows in `orders`"""
    out, prev = [], np.arange(orders[0].size)
    for o in orders:
        inv = np.empty_like(prev); inv[prev] = np.arange(prev.size)
        out.append(inv[o]); prev = o
    return np.stack(out)


def _state(net):
    m, v, bp = net.adam_state()
    return [net.get_params(), m, v, bp]


def _launch(shape, data, n_rows, epochs, perms, fs, monkeypatch, target_kl=None, max_batches=None):
    """one batch_train! launch through the library, so that the code, the info and the epoch rows are there after a failure too: (code, state, info, epoch rows)"""
    from crux_jl_amd import core
    monkeypatch.setenv("CRUX_FS", "1" if fs else "0")
    loss = SHAPES[shape][7]
    g, _ = _pair(shape); gb = _gbuf(shape, data, n_rows)
    kw = {} if max_batches is None else {"max_batches": max_batches}
    opt = crux.TrainingParams(loss=GLOSS[loss], optimizer=crux.Adam(LR), batch_size=BS, epochs=epochs, target_kl=target_kl, name="n_", **kw)
    core._ensure_opt(g, opt)
    cfg = core._train_cfg(g, opt, P_PPO)
    pp = np.ascontiguousarray(np.asarray(perms, np.int64)); assert pp.shape == (epochs, n_rows)
    raw = np.zeros(L.INFO_N, np.float32); ep = np.zeros((epochs, L.INFO_N), np.float32)
    rc = g.ctx.lib.crux_batch_train(g.h, gb.h, C.byref(cfg), core._vp(pp), core._vp(raw), core._vp(ep))
    return int(rc), _state(g), raw, ep


def _oracle(shape, data, n_rows, epochs, perms):
    od, ad, disc, dims, kind, head, okind, loss = SHAPES[shape]
    _, o = _pair(shape); ob = _obuf(shape, data, n_rows)
    o.adam_init(float(np.float32(LR)))
    cfg = parity.train_cfg(loss, head, BS, epochs, -1.0, 0); oi = np.zeros(L.INFO_N, np.float32); oep = np.zeros((epochs, L.INFO_N), np.float32)
    O.chk(O.lib().orc_batch_train(o.h, ob.h, C.byref(cfg), O.vpz(np.ascontiguousarray(perms, np.int64)), O.vpz(oi), O.vpz(oep)))
    om, ov, obp = o.adam_state()
    return [np.array(o.params, copy=True), om, ov, obp], oi, oep      # (a copy: the oracle network does not outlive this call)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _close(a, b, what):
    """the info bar of test_gpu_fs2_misc_lanes.py: 2e-4 relative (absolute below 1); NaN where the reference has NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, a, b)
    f = ~np.isnan(b)
    print(what, "max |d| = %.3g" % (float(np.abs(a[f] - b[f]).max()) if f.any() else 0.0))
    assert np.all(np.abs(a[f] - b[f]) <= 2e-4 * np.maximum(1.0, np.abs(b[f]))), (what, a, b)


def _check_state(got, ref, what, exact_bp):
    """the parameter / moment bars of test_gpu_fs2_misc_lanes.py"""
    d = [float(np.abs(got[i] - ref[i]).max()) for i in range(3)]
    print(what, "max |dtheta| = %.3g, |dm| = %.3g, |dv| = %.3g" % tuple(d))
    assert d[0] < 2e-5 and d[1] <= 2e-5 and d[2] <= 2e-5, (what, d)
    assert np.array_equal(got[3], ref[3]) if exact_bp else np.allclose(got[3], ref[3], rtol=1e-12), what


def _cols(shape):
    return [L.INFO[k] for k in (INFO_COLS if SHAPES[shape][7] != "value_mse" else ("loss", "grad_norm"))]


def _against_split_and_oracle(shape, n_rows, epochs, monkeypatch, kl_twin):
    data = _shard(shape, n_rows); perms = _perms(n_rows, epochs)
    steps = epochs * ((n_rows + BS - 1) // BS)
    rc2, s2, i2, e2 = _launch(shape, data, n_rows, epochs, perms, True, monkeypatch)
    assert rc2 == L.OK and int(i2[L.INFO["batches_trained"]]) == steps and int(i2[L.INFO["epochs_run"]]) == epochs
    if kl_twin:      # statistics on every step, never stops: the same bits everywhere
        rck, sk, ik, ek = _launch(shape, data, n_rows, epochs, perms, True, monkeypatch, target_kl=1e30)
        assert rck == L.OK
        for x, y, what in zip(s2 + [i2, e2], sk + [ik, ek], ("theta", "m", "v", "beta powers", "info", "epoch rows")):
            assert _bits(x, y), (shape, what)
    rc1, s1, i1, e1 = _launch(shape, data, n_rows, epochs, perms, False, monkeypatch)
    assert rc1 == L.OK and int(i1[L.INFO["batches_trained"]]) == steps
    so, oi, oep = _oracle(shape, data, n_rows, epochs, perms)
    assert int(oi[L.INFO["batches_trained"]]) == steps
    _check_state(s2, s1, shape + " vs split:", True)
    _check_state(s2, so, shape + " vs oracle:", False)
    cols = _cols(shape)
    _close(e2[:, cols], e1[:, cols], shape + " epoch rows vs split:")
    _close(e2[:, cols], oep[:, cols], shape + " epoch rows vs oracle:")
    _close(i2[cols], i1[cols], shape + " info vs split:")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_report_only_statistics_have_the_bits_of_every_step_statistics(gpu_ctx, monkeypatch, shape):
    _against_split_and_oracle(shape, 328, 3, monkeypatch, True)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_mid_epoch_report_at_max_batches(gpu_ctx, monkeypatch, shape):
    """max_batches = 4: three steps of epoch 0, then the first step of epoch 1 -- a full minibatch in the middle of an epoch whose statistics are read because the loop ends on it"""
    data = _shard(shape, 328); perms = _perms(328, 3)
    rc2, s2, i2, e2 = _launch(shape, data, 328, 3, perms, True, monkeypatch, max_batches=4)
    rc1, s1, i1, e1 = _launch(shape, data, 328, 3, perms, False, monkeypatch, max_batches=4)
    assert rc2 == rc1 == L.OK
    assert int(i2[L.INFO["batches_trained"]]) == int(i1[L.INFO["batches_trained"]]) == 4
    assert int(i2[L.INFO["epochs_run"]]) == int(i1[L.INFO["epochs_run"]]) == 2
    _check_state(s2, s1, shape + " vs split:", True)
    cols = _cols(shape)
    _close(i2[cols], i1[cols], shape + " info at max_batches vs split:")
    _close(e2[:2, cols], e1[:2, cols], shape + " epoch rows at max_batches vs split:")


@pytest.mark.parametrize("shape", ["4-64-64-2-categorical", "4-64-64-1-value", "3-64-64-1-gaussian"])
def test_a_suspect_step_in_minibatch_1_of_epoch_0(gpu_ctx, monkeypatch, shape):
    clean = _shard(shape, 328); perms = _perms(328, 3, seed=7)
    data = dict(clean); data["s"] = clean["s"].copy(); data["s"][0, perms[0][BS + 5]] = np.nan
    rc2, s2, i2, e2 = _launch(shape, data, 328, 3, perms, True, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, data, 328, 3, perms, False, monkeypatch)
    assert rc2 == rc1 == L.ENAN
    # every parameter and moment: the bits of a run stopped after minibatch 0
    rcr, sr, _, _ = _launch(shape, clean, 328, 1, perms[:1], True, monkeypatch, max_batches=1)
    assert rcr == L.OK
    for x, y in zip(s2[:3], sr[:3]):
        assert _bits(x, y)
    before = _pair(shape)[0].get_params()
    assert np.any(s2[0] != before)
    assert np.isnan(i2[L.INFO["grad_norm"]]) == np.isnan(i1[L.INFO["grad_norm"]])
    _close(i2, i1, shape + " info of the failed launch vs split:")
    _close(e2, e1, shape + " epoch rows of the failed launch vs split:")


@pytest.mark.parametrize("shape", ["4-64-64-2-categorical", "3-64-64-1-gaussian"])
def test_a_nan_advantage_is_what_the_sample_split_learner_makes_of_it(gpu_ctx, monkeypatch, shape):
    clean = _shard(shape, 328)
    rng = np.random.default_rng(11)
    row = 17
    orders = []
    for e, pos in enumerate((BS + 5, BS + 9, 2 * BS + 3)):      # minibatch 1, minibatch 1, the reporting minibatch
        o = rng.permutation(328); j = int(np.where(o == row)[0][0]); o[j], o[pos] = o[pos], o[j]
        orders.append(o)
    perms = _perms_for_orders(orders)
    data = dict(clean); data["advantage"] = clean["advantage"].copy(); data["advantage"].reshape(-1)[row] = np.nan
    rc2, s2, i2, e2 = _launch(shape, data, 328, 3, perms, True, monkeypatch)
    rc1, s1, i1, e1 = _launch(shape, data, 328, 3, perms, False, monkeypatch)
    print(shape, "NaN advantage: codes", rc2, rc1, "batches", i2[L.INFO["batches_trained"]], i1[L.INFO["batches_trained"]])
    assert rc2 == rc1
    assert int(i2[L.INFO["batches_trained"]]) == int(i1[L.INFO["batches_trained"]]) and int(i2[L.INFO["epochs_run"]]) == int(i1[L.INFO["epochs_run"]])
    _check_state(s2, s1, shape + " vs split:", True)
    cols = _cols(shape)
    _close(i2[cols], i1[cols], shape + " info vs split:")
    _close(e2[:, cols], e1[:, cols], shape + " epoch rows vs split:")
    if rc2 == L.OK:      # the row was reported once, in epoch 2: that row's loss is NaN, the others are numbers
        assert np.isnan(e2[2, L.INFO["loss"]]) and not np.isnan(e2[:2, L.INFO["loss"]]).any()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_tile_order_of_the_w2_update(gpu_ctx, monkeypatch, shape):
    _against_split_and_oracle(shape, 200, 5, monkeypatch, False)
