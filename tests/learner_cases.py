"""Cases of the register-resident on-policy learners (csrc/train_fs2.hip, train_mfma_x2.hip, train_mfma8.hip) at the edges of their row masks, with LIVE gradients.

Host only: nothing here needs a device until Case.gpu_net() / whole_epoch_windows(g=...) are called (tests/test_learner_cases.py uses the oracle alone).

  FS2_ROWS / MFX_ROWS / MF8_ROWS   the closed shape lists of the three dispatchers as data: (in, out, kind, act1, h2, act2); test_learner_cases.py parses the one table
                                    they instantiate from (csrc/learner_shapes.h: the LF_FS2 / LF_X2 / LF_ONE8 flags of its rows) and requires equality -- FS2_ROWS in the
                                    table's order, which the (bs, r) schedule counts in --, so a row added without a case fails without a GPU
  make_case(row, bs, r, seed)       oracle network + buffer data of N = 3 bs + r rows whose :logprob column is CONSISTENT with the network: the float64 log-density of the freshly
                                    initialised policy at the stored action plus N(0, LOGPROB_SIGMA). The older window tests draw logprob ~ N(-1.2, 0.05) whatever the action
                                    dimension; at 4..8 Gaussian actions the true density is near -10, every ratio is e^-9, every row is clipped and the surrogate contributes
                                    nothing to W1..W3 (clip_fraction 1.00, |g| = lambda_e sqrt(out): the entropy term on logSigma alone)
  FS2_EDGES / fs2_pairs(i)          twelve (bs, r) pairs: a ragged tail of 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97 rows (k_train_fs2 places sample 32 wg + 16 tile + lane:
                                    whole tiles / whole workgroups empty) under minibatches of 65 .. 128 rows; table row i takes pairs (3 i + j) % 12 (plus FS2_EXTRA_PAIRS)
  SINGLE_NS / SMALL_BS / SMALL_RS   the edges of the sample-split kernels below 65 rows
  whole_epoch_windows               parity.learner_window_parity with a whole epoch as the window (its last minibatch is the ragged one), returning Adam's m beside theta
  oracle_run                        the oracle's own trajectory of the same schedule: per-step infos, m at the window ends, optionally with one row dropped from one minibatch
"""
import ctypes as C

import numpy as np

import dense_reference as R
import oracle as O
from crux_jl_amd import _lib as L

CAT, GAU, VAL, RELU, TANH, IDENT = "categorical", "gaussian", "value", "relu", "tanh", "identity"


def _r(i, o, k, a, h2=64, a2=None):
    return (i, o, k, a, h2, a if a2 is None else a2)


# learner_shapes.h: every row (all carry LF_FS2), in the order of the file
FS2_ROWS = [_r(4, 2, CAT, RELU), _r(4, 1, VAL, RELU), _r(17, 6, GAU, TANH), _r(17, 1, VAL, TANH),
            _r(3, 1, GAU, RELU), _r(3, 1, VAL, RELU), _r(17, 6, GAU, RELU), _r(17, 1, VAL, RELU), _r(8, 4, CAT, RELU), _r(8, 1, VAL, RELU), _r(2, 1, GAU, RELU), _r(2, 1, VAL, RELU),
            _r(6, 3, CAT, RELU), _r(6, 1, VAL, RELU), _r(2, 3, CAT, RELU),
            _r(8, 2, GAU, RELU), _r(8, 2, GAU, TANH), _r(8, 1, VAL, TANH),
            _r(11, 3, GAU, RELU), _r(11, 3, GAU, TANH), _r(11, 1, VAL, RELU), _r(11, 1, VAL, TANH),
            _r(24, 4, GAU, RELU), _r(24, 4, GAU, TANH), _r(24, 1, VAL, RELU), _r(24, 1, VAL, TANH),
            _r(27, 8, GAU, RELU), _r(27, 8, GAU, TANH), _r(27, 1, VAL, RELU), _r(27, 1, VAL, TANH),
            _r(17, 6, GAU, TANH, 32, TANH), _r(17, 1, VAL, TANH, 32, IDENT), _r(17, 1, VAL, TANH, 32, TANH)]
# the LF_X2 rows: the two-CU form, 64-64 hidden (this order feeds case ids)
MFX_ROWS = [_r(4, 2, CAT, RELU), _r(4, 1, VAL, RELU), _r(3, 1, GAU, RELU), _r(3, 1, VAL, RELU), _r(17, 6, GAU, RELU), _r(17, 6, GAU, TANH), _r(17, 1, VAL, RELU), _r(17, 1, VAL, TANH),
            _r(8, 4, CAT, RELU), _r(8, 1, VAL, RELU)]
# the LF_ONE8 rows: the one-CU form
MF8_ROWS = [_r(4, 2, CAT, RELU), _r(4, 1, VAL, RELU), _r(3, 1, GAU, RELU), _r(3, 1, VAL, RELU)]
# small minibatches and single steps: the one-CU kernel where it has the shape, the two-CU kernel's any-mode path for the 17- and 8-wide rows
SMALL_ROWS = MF8_ROWS + [r for r in MFX_ROWS if r not in MF8_ROWS]

FS2_EDGES = [(128, 1), (128, 17), (128, 33), (128, 97), (127, 16), (113, 32), (112, 15), (97, 96), (96, 31), (81, 65), (80, 64), (65, 63)]
SINGLE_NS = [1, 15, 16, 17, 33, 63, 64, 65, 127, 128]
SMALL_BS, SMALL_RS = [16, 33, 64], [1, 15, 17]

LOGSIGMA0 = -0.5
LOGPROB_SIGMA = 0.1       # chosen once: every fs2 case keeps a mean clip_fraction inside [0.02, 0.6] over five epochs (test_learner_cases.py asserts it)
EXTRAS = ["return", "logprob", "advantage"]
PPO_P = {"eps": 0.2, "lambda_p": 1.0, "lambda_e": 0.1}
LR = 3e-4
M_SHIFT_MIN = 5e-5        # sensitivity: dropping ONE row must move Adam's m by five times the bound the GPU tests assert on it (1e-5)
# (row index, bs, r) -> data seed, for a case whose default draw misses M_SHIFT_MIN (a case that misses gets another seed; none may be dropped)
SEED_OVERRIDES = {(12, 128, 1): 7707}      # 6-3 categorical at a tail of one row: the default draw moved m by 4.4e-5


# The rule "row i takes pairs (3 i + j) % 12" gives a row the offset 3 (i % 4), and the order of the table alternates policies and critics: every row with
# i % 4 == 1 is a critic, the four categorical rows sit at i % 4 in {0, 0, 0, 2}, no Gaussian row at i % 4 == 1 and no critic at i % 4 == 2. The rule alone therefore cannot
# meet "every pair under every head"; these rows take the missing pairs IN ADDITION to their own three (nothing of the rule is dropped): 99 + 12 = 111 cases.
FS2_EXTRA_PAIRS = {8: [3, 4, 5], 12: [9, 10, 11],      # categorical 8-4 and 6-3
                   27: [3, 4, 5],                      # Gaussian 27-8 tanh
                   3: [6, 7, 8]}                       # critic 17-1 tanh


def fs2_pairs(i):
    return [FS2_EDGES[(3 * i + j) % 12] for j in range(3)] + [FS2_EDGES[q] for q in FS2_EXTRA_PAIRS.get(i, [])]


def fs2_cases():
    """[(row index, row, bs, r)]: 33 rows x 3 pairs, and the twelve of FS2_EXTRA_PAIRS"""
    return [(i, row, bs, r) for i, row in enumerate(FS2_ROWS) for bs, r in fs2_pairs(i)]


def case_seed(i, bs, r):
    return SEED_OVERRIDES.get((i, bs, r), 5000 + 131 * i + bs + 7 * r)


def row_id(row):
    i, o, k, a, h2, a2 = row
    return "%d-64-%d-%d_%s_%s%s" % (i, h2, o, k, a, "" if a2 == a else "-" + a2)


def action_space_of(row):
    """(action dimension, discrete) of the buffer a row trains on: a policy's own; a critic's is the one of the policy it is paired with (the first policy row of the lists
    with its input width, its activation preferred), since a critic reads no action"""
    i, o, k, a = row[:4]
    if k != VAL:
        return o, k == CAT
    pol = [p for p in FS2_ROWS if p[0] == i and p[2] != VAL]
    pol = [p for p in pol if p[3] == a] or pol
    return pol[0][1], pol[0][2] == CAT


def policy_logprob64(params, dims, acts, kind, s, a, logsigma=LOGSIGMA0):
    """float64 log-density of the action columns under the network: log-softmax at the one-hot action, or sum_d -(a - mu)^2 / (2 sigma^2) - log sqrt(2 pi) - logSigma"""
    y = R._np_mlp(np.asarray(params), dims, acts, np.asarray(s))[-1]
    if kind == CAT:
        z = y - y.max(axis=0, keepdims=True); ls = z - np.log(np.exp(z).sum(axis=0, keepdims=True))
        return (ls * np.asarray(a, np.float64)).sum(axis=0, keepdims=True)
    sg2 = np.exp(2.0 * logsigma)
    return (-(np.asarray(a, np.float64) - y) ** 2 / (2.0 * sg2) - 0.5 * np.log(2.0 * np.pi) - logsigma).sum(axis=0, keepdims=True)


class Case:
    """one learner case: the oracle network `o` (freshly initialised), the buffer columns `data` (N rows), and what the drivers need to train on them"""

    def __init__(self, row, N, seed):
        i, out, kind, a1, h2, a2 = row
        self.row, self.N, self.seed, self.kind = row, N, seed, kind
        self.dims, self.acts = [i, 64, h2, out], [a1, a2, IDENT]
        self.od = i; self.ad, self.disc = action_space_of(row)
        self.n_extra = out if kind == GAU else 0
        self.loss, self.head = ("value_mse", "deterministic") if kind == VAL else ("ppo", kind)
        self.net_seed = 400 + seed % 97
        self.o = O.OMlp(self.dims, self.acts, self.n_extra).init_glorot(self.net_seed, 0, LOGSIGMA0)
        rng = np.random.default_rng(seed); od, ad = self.od, self.ad
        if RELU in self.acts:
            s = np.ascontiguousarray(R.kink_free_inputs(self.o.params, self.dims, self.acts, N, rng, 1e-4))
        else:
            s = rng.normal(0, 1, (od, N)).astype(np.float32)
        act = np.eye(ad, dtype=bool)[:, rng.integers(0, ad, N)] if self.disc else rng.normal(0, 0.7, (ad, N)).astype(np.float32)
        d = {"s": s, "a": act, "sp": rng.normal(0, 1, (od, N)).astype(np.float32), "r": np.ones((1, N), np.float32),
             "done": np.zeros((1, N), bool), "episode_end": np.zeros((1, N), bool), "return": rng.normal(0, 1, (1, N)).astype(np.float32),
             "advantage": rng.normal(0, 1, (1, N)).astype(np.float32)}
        noise = rng.normal(0, LOGPROB_SIGMA, (1, N))
        if kind == VAL:       # a critic does not read :logprob
            d["logprob"] = (-1.2 + noise).astype(np.float32)
        else:
            d["logprob"] = (policy_logprob64(self.o.params, self.dims, self.acts, kind, s, act) + noise).astype(np.float32)
        self.data = d

    def gpu_net(self):
        """the same network on the device (identical Philox draws: parity.make_pair)"""
        import parity
        pk = "discrete" if self.kind == CAT else "gaussian" if self.kind == GAU else "continuous"
        g, o = parity.make_pair(self.dims, self.acts, self.net_seed, 0, pk, n_extra=self.n_extra, extra_init=LOGSIGMA0)
        assert np.array_equal(o.params, self.o.params)
        return g

    def fresh_oracle(self):
        return O.OMlp(self.dims, self.acts, self.n_extra).init_glorot(self.net_seed, 0, LOGSIGMA0)

    def oracle_buffer(self):
        ob = O.OBuffer(self.od, self.ad, L.ACTION_DISCRETE if self.disc else L.ACTION_CONTINUOUS, self.N, EXTRAS); ob.push(self.data)
        return ob


def make_case(row, bs, r, seed):
    """the case of N = 3 bs + r rows: three full minibatches of bs rows and a ragged one of r"""
    return Case(row, 3 * bs + r, seed)


def train_cfg(loss, head, bs, seed, P=None):
    P = P or PPO_P
    cfg = L.TrainCfg()
    cfg.loss, cfg.head, cfg.batch_size, cfg.epochs, cfg.max_batches = L.LOSS[loss], L.HEAD[head], bs, 1, 0
    cfg.eps_clip, cfg.lambda_p, cfg.lambda_e, cfg.target_kl = P["eps"], P["lambda_p"], P["lambda_e"], -1.0
    cfg.shuffle_seed, cfg.shuffle_counter = seed, 0
    return cfg


def oracle_run(case, bs, loss=None, epochs=5, at=(2, 4), seed=900, drop=None, lr=LR):
    """The oracle's trajectory of whole_epoch_windows without a device: batch_train! spelled out (shuffle!, then train! per minibatch) for `epochs` epochs.
    drop = (epoch, k): minibatch k of that epoch trains on ids[:-1]. Returns (infos [steps x INFO_N], {epoch: m after that epoch} for the epochs in `at`)."""
    o, ob = case.fresh_oracle(), case.oracle_buffer()
    N = case.N; nmb = -(-N // bs)
    o.adam_init(float(np.float32(lr)))
    cfg = train_cfg(loss or case.loss, case.head, bs, seed)
    perm = np.empty(N, np.int64); infos, ms = [], {}
    for e in range(epochs):
        O.lib().orc_perm(seed, e, N, O.vpz(perm)); ob.permute(perm + 1)
        for k in range(nmb):
            ids = np.arange(k * bs, min((k + 1) * bs, N), dtype=np.int64)
            if drop == (e, k):
                ids = np.ascontiguousarray(ids[:-1])
            info = np.zeros(L.INFO_N, np.float32)
            O.chk(O.lib().orc_train_step(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(info)))
            infos.append(info)
        if e in at:
            ms[e] = o.adam_state()[0]
    return np.array(infos), ms


def whole_epoch_windows(g, o, data0, od, ad, disc, loss, head, bs, epochs=5, at=(2, 4), seed=900, lr=LR, P=None):
    """parity.learner_window_parity with starts = [e * nmb for e in at] and W = nmb: at the start of each epoch in `at` the GPU learner `g` gets the oracle's state (theta, m, v,
    beta powers) and the row order of that moment and runs the WHOLE epoch -- its ragged last minibatch included -- in one persistent launch (explicit permutation). Returns one
    dict per window: start (the global step), dtheta = max |theta - theta_o|, dm = max |m - m_o|, m_scale = max |m_o|, bp / bp_o (the beta powers), batches (w_batches_trained),
    nmb, and the GPU's theta / m / v themselves (for bit comparisons between switch forms)."""
    import crux_jl_amd as crux
    P = P or PPO_P
    N = np.asarray(data0["s"]).shape[-1]; nmb = -(-N // bs)
    kind = L.ACTION_DISCRETE if disc else L.ACTION_CONTINUOUS
    ob = O.OBuffer(od, ad, kind, N, EXTRAS); ob.push(data0)
    gb = crux.ExperienceBuffer(crux.ContinuousSpace(od), crux.DiscreteSpace(ad) if disc else crux.ContinuousSpace(ad), N, EXTRAS)
    o.adam_init(float(np.float32(lr)))
    gloss = {"ppo": crux.ppo_loss, "value_mse": crux.value_mse_loss, "a2c": crux.a2c_loss}[loss]
    opt = crux.TrainingParams(loss=gloss, batch_size=bs, epochs=1, max_batches=nmb, name="w_", shuffle_seed=seed)
    g.attach_optimizer(opt.optimizer)
    cfg = train_cfg(loss, head, bs, seed, P)
    info = np.zeros(L.INFO_N, np.float32); perm = np.empty(N, np.int64); out = []
    for e in range(epochs):
        D_e = {k: ob[k] for k in ob.keys()}                                  # row order before this epoch's shuffle!
        O.lib().orc_perm(seed, e, N, O.vpz(perm)); ob.permute(perm + 1)
        got = None
        if e in at:
            m, v, bp = o.adam_state()
            g.set_params(o.params.copy()); g.set_adam_state(m, v, bp)
            gb.clear_(); gb.push_(D_e)
            gi = crux.batch_train_(g, opt, P, gb, perms=perm[None, :] + 1)
            gm, gv, gbp = g.adam_state()
            got = {"start": e * nmb, "nmb": nmb, "batches": int(gi["w_batches_trained"]), "theta": g.get_params(), "m": gm, "v": gv, "bp": np.asarray(gbp, np.float64).copy()}
        for k in range(nmb):
            ids = np.arange(k * bs, min((k + 1) * bs, N), dtype=np.int64)
            O.chk(O.lib().orc_train_step(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(info)))
        if got is not None:
            om, ov, obp = o.adam_state()
            got.update(dtheta=float(np.abs(got["theta"] - o.params).max()), dm=float(np.abs(got["m"] - om).max()), m_scale=float(np.abs(om).max()),
                       bp_o=np.asarray(obp, np.float64).copy())
            out.append(got)
    return out
