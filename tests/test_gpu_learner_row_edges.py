"""The register-resident learners -- k_train_fs2, the two-CU k_train_mfma<4,2> and the one-CU k_train_mfma<8,1> -- against the oracle at the edges of their row masks, on
LIVE PPO gradients (tests/learner_cases.py: :logprob is the policy's own float64 log-density plus N(0, 0.1); tests/test_learner_cases.py proves on the CPU that every fs2
case has a clip fraction of 0.03 .. 0.52 and moves Adam's m by >= 5e-5 when ONE row is dropped).

k_train_fs2 places sample sidx = 32 workgroup + 16 tile + lane, masks sidx < nb and scales by 1 / nb; it takes minibatches of 65 .. 128 rows and any ragged last minibatch.
Before this module the suite met it (against another implementation) at bs = 128, one bs = 100, and one tail of 104 rows. Here: every row of its dispatch table under three or
six of twelve (bs, r) pairs -- tails of 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97 rows (a whole tile, or three whole workgroups, empty), bs of 65, 80, 81, 96, 97, 112,
113, 127, 128 --, the sample-split kernels at the same edges, and both of those at the small sizes they alone serve (1 .. 128 single-step rows, bs 16 / 33 / 64 loops).

Every bound is one the suite already asserts: |dtheta| < parity.window_tol(start) (5e-5 this early in training) for a whole-epoch teacher-forced window, 2e-5 after the three
single steps; |m - m_o| <= 1e-5 max(1, |m_o|max) (the bound that discriminates: see the sensitivity test); beta powers rtol 1e-12; batches trained exact; gradients
1e-4 max(1, |g_o|max); the seven infos 1e-4. Each module prints its measured worst (ROW_EDGES lines) and ends with the not-the-generic-learner hook.

Not here: lagrange_ppo_loss (a minibatch without an episode end is a NaN step by definition), the replica-group forms, the _multi population launchers, the dense engine.

Measured on an MI355X (bounds: |dtheta| 5e-5 windows / 2e-5 single steps, |dm| 1e-5 max(1, |m_o|max)):
  A (k_train_fs2, 111 + 6 + 12 cases)            worst |dtheta| 5.96e-08, worst |dm| / max(1, |m_o|max) 6.56e-07
  B (two-CU and one-CU kernels, 20 + 12 cases)   worst |dtheta| 2.98e-08, worst |dm| 1.64e-07
  C (single steps and small loops, 100 + 90)     worst |dtheta| 5.1e-06 (after three single steps), worst |dm| 4.01e-06; gradients <= 6.6e-06 of scale 2.2
No case failed; no kernel or oracle change was needed.
Mutation runs (scratch builds, each run once: this module, then test_gpu_fs2*.py, test_gpu_round3.py, test_gpu_components.py, test_gpu_ppo_parity.py, test_gpu_dense_learner.py,
test_gpu_switches.py):
  1 k_train_fs2: invB = 1 / bs instead of 1 / nb              this module 39 of 73 ids fail (every id of A); the older modules 27 of 260 (their 104-row tail against the sample-split kernels)
  2 k_train_fs2: mask sidx < (nb & ~15)                       this module 39 fail (every id of A); the older modules the same 27
  3 k_train_fs2: Gaussian dz[1] = 0                           this module 14 fail: all eleven Gaussian rows with two or more actions, both a2c ids, the 27-8 gather id; the older
                                                              modules 18, on six of those eleven instantiations (17-6 tanh, 17-64-32-6, 8-2 tanh, 11-3 tanh, 24-4 relu, 27-8 tanh: the
                                                              N(-1.2, 0.05) windows are not quite dead -- rows with A > 0 keep a gradient of A e^-9, which Adam's normalisation lifts past
                                                              2e-6 --) and on none of 17-6 relu, 8-2 relu, 11-3 relu, 24-4 tanh, 27-8 relu
  4 k_train_mfma: mask sidx < (nb & ~15)                      this module 34 fail (every id of B and C); the older modules 30
So the older suite does notice a mask or scale that is wrong at EVERY ragged size; what it cannot see is an instantiation it never meets against a reference (mutation 3) or an
error confined to sizes it never runs (tails that leave a tile or a workgroup empty, bs below 100).
"""
import ctypes as C

import numpy as np
import pytest

import crux_jl_amd as crux
from crux_jl_amd import _lib as L
import learner_cases as LC
import oracle as O
import parity
from test_gpu_dense_learner import _not_generic

pytestmark = pytest.mark.gpu
E = LC.FS2_EDGES
WORST = {}      # module letter -> [max |dtheta|, max |dm| / max(1, |m_o|max)]
LINES = []


def _say(msg):
    LINES.append(msg)


@pytest.fixture(autouse=True)
def _report(capfd):
    """the measured figures of a test, printed after it whether it passed or not (_not_generic reads, and thereby empties, what the test itself printed)"""
    LINES.clear()
    yield
    print("\n".join(LINES))


def _note(mod, dtheta, dm_rel):
    w = WORST.setdefault(mod, [0.0, 0.0]); w[0] = max(w[0], dtheta); w[1] = max(w[1], dm_rel)
    _say("ROW_EDGES module %s worst so far: |dtheta| %.3g, |dm| / max(1, |m_o|max) %.3g" % (mod, w[0], w[1]))


def _windows(mod, row, bs, r, seed, loss=None):
    """one case through whole_epoch_windows (five oracle epochs, the GPU replays epochs 2 and 4 whole), with every bound of the module's table"""
    case = LC.make_case(row, bs, r, seed)
    res = LC.whole_epoch_windows(case.gpu_net(), case.fresh_oracle(), case.data, case.od, case.ad, case.disc, loss or case.loss, case.head, bs)
    assert len(res) == 2, res
    for w in res:
        rel = w["dm"] / max(1.0, w["m_scale"])
        _say("ROW_EDGES %s %s %s bs %d r %d start %d: |dtheta| %.3g |dm| %.3g (|m_o|max %.3g)" % (mod, LC.row_id(row), loss or case.loss, bs, r, w["start"], w["dtheta"], w["dm"], w["m_scale"]))
        _note(mod, w["dtheta"], rel)
    for w in res:
        tag = (LC.row_id(row), bs, r, w["start"])
        assert w["batches"] == w["nmb"] == -(-case.N // bs), tag
        assert np.allclose(w["bp"], w["bp_o"], rtol=1e-12, atol=0), (tag, w["bp"], w["bp_o"])
        assert w["dtheta"] < parity.window_tol(w["start"]), (tag, w["dtheta"])
        assert w["dm"] <= 1e-5 * max(1.0, w["m_scale"]), (tag, w["dm"], w["m_scale"])
    return res


# ---- A. k_train_fs2 ---------------------------------------------------------------------------------------------------------------------------------------
FS2_IDS = ["%02d_%s" % (i, LC.row_id(row)) for i, row in enumerate(LC.FS2_ROWS)]


@pytest.mark.parametrize("i", range(len(LC.FS2_ROWS)), ids=FS2_IDS)
def test_fs2_every_row_at_its_row_edges(gpu_ctx, capfd, i):
    """every row of train_fs2.hip's table under its (bs, r) pairs: PPO for the policy heads, value_mse for the critics"""
    for bs, r in LC.fs2_pairs(i):
        _windows("A", LC.FS2_ROWS[i], bs, r, LC.case_seed(i, bs, r))
    _not_generic(capfd)


A2C_ROWS = [0, 2, 30]      # 4-2 categorical, 17-6 Gaussian tanh, and the 64-32 Gaussian of the reference's HalfCheetah example


@pytest.mark.parametrize("i", A2C_ROWS, ids=[FS2_IDS[i] for i in A2C_ROWS])
def test_fs2_a2c_at_row_edges(gpu_ctx, capfd, i):
    """the same kernel under a2c_loss (no ratio, no clip: the head's other branch) at a tail of one tile and at the smallest minibatch"""
    for bs, r in [(127, 16), (65, 63)]:
        _windows("A", LC.FS2_ROWS[i], bs, r, LC.case_seed(i, bs, r) + 1, loss="a2c")
    _not_generic(capfd)


GATHER_ROWS = [0, 27, 7]      # 4-2 categorical, 27-8 Gaussian tanh, 17-1 critic


@pytest.mark.parametrize("i", GATHER_ROWS, ids=[FS2_IDS[i] for i in GATHER_ROWS])
def test_fs2_column_gather_form_is_bit_identical_at_row_edges(gpu_ctx, capfd, monkeypatch, i):
    """CRUX_PACK_ROWS=0 (the helper waves gather the columns instead of the packed 128-byte rows): theta, m and v of both windows are the bits of the packed form --
    test_on_policy_switch_forms_are_bit_identical makes this claim at bs = 128 without a tail"""
    for bs, r in [(128, 1), (113, 32)]:
        seed = LC.case_seed(i, bs, r) + 2
        monkeypatch.setenv("CRUX_PACK_ROWS", "0"); got = _windows("A", LC.FS2_ROWS[i], bs, r, seed)
        monkeypatch.delenv("CRUX_PACK_ROWS"); ref = _windows("A", LC.FS2_ROWS[i], bs, r, seed)
        for a, b in zip(got, ref):
            for k in ("theta", "m", "v"):
                assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (LC.row_id(LC.FS2_ROWS[i]), bs, r, a["start"], k)
    _not_generic(capfd)


# ---- B. the sample-split forms at the same edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(LC.MFX_ROWS)), ids=[LC.row_id(r) for r in LC.MFX_ROWS])
def test_two_cu_kernel_at_row_edges(gpu_ctx, capfd, monkeypatch, k):
    """CRUX_FS=0: the rows of train_mfma_x2.hip's table on k_train_mfma<4,2>; row k takes pairs 5 k and 5 k + 6 (mod 12), which meets all twelve over the ten rows"""
    monkeypatch.setenv("CRUX_FS", "0")
    for bs, r in (E[(5 * k) % 12], E[(5 * k + 6) % 12]):
        _windows("B", LC.MFX_ROWS[k], bs, r, LC.case_seed(100 + k, bs, r))
    _not_generic(capfd)


@pytest.mark.parametrize("k", range(len(LC.MF8_ROWS)), ids=[LC.row_id(r) for r in LC.MF8_ROWS])
def test_one_cu_kernel_at_row_edges(gpu_ctx, capfd, k):
    """Context.set_learner_cus(1): the rows of train_mfma8.hip's table on k_train_mfma<8,1> (a 16-sample tile per wave); row k takes pairs k and k + 4, k + 8"""
    gpu_ctx.set_learner_cus(1)
    try:
        for bs, r in (E[k], E[k + 4], E[k + 8]):
            _windows("B", LC.MF8_ROWS[k], bs, r, LC.case_seed(200 + k, bs, r))
    finally:
        gpu_ctx.set_learner_cus(0)
    _not_generic(capfd)


# ---- C. small minibatches and single steps ----------------------------------------------------------------------------------------------------------------
SMALL_IDS = [LC.row_id(r) for r in LC.SMALL_ROWS]


@pytest.mark.parametrize("k", range(len(LC.SMALL_ROWS)), ids=SMALL_IDS)
def test_gradient_only_and_single_steps_at_row_edges(gpu_ctx, capfd, k):
    """the body of test_gpu_components.py::test_train_step_and_loss_grad_match_oracle with its tolerances, at n = 1 .. 128 ids out of 128 rows: crux_loss_grad against
    orc_loss_grad (gradient, the seven infos, parameters untouched), then three train_ steps (parameters 2e-5, m, beta powers). The one-CU kernel for the four narrow rows,
    the two-CU kernel's any-mode path (workgroup 1 idles on empty tiles below 65 rows) for the 17- and 8-wide ones."""
    row = LC.SMALL_ROWS[k]
    for n in LC.SINGLE_NS:
        case = LC.Case(row, 128, LC.case_seed(300 + k, n, 0)); g, o, ob = case.gpu_net(), case.fresh_oracle(), case.oracle_buffer()
        gb = crux.ExperienceBuffer(crux.ContinuousSpace(case.od), crux.DiscreteSpace(case.ad) if case.disc else crux.ContinuousSpace(case.ad), case.N, LC.EXTRAS); gb.push_(case.data)
        rng = np.random.default_rng(1000 * k + n)
        p = crux.TrainingParams(loss=crux.value_mse_loss if case.kind == LC.VAL else crux.ppo_loss, batch_size=n, epochs=1, name="x_")
        o.adam_init(float(np.float32(LC.LR))); cfg = LC.train_cfg(case.loss, case.head, n, 11)
        ids = rng.permutation(case.N)[:n].astype(np.int64)
        g.attach_optimizer(p.optimizer); g.optimizer = p.optimizer
        raw = np.zeros(L.INFO_N, np.float32); tc = crux.api._train_cfg(g, p, LC.PPO_P)
        g.ctx.check(g.ctx.lib.crux_loss_grad(g.h, gb.h, C.byref(tc), O.vpz(ids), ids.size, O.vpz(raw)))
        oinfo = np.zeros(L.INFO_N, np.float32); O.chk(O.lib().orc_loss_grad(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(oinfo)))
        gg = np.empty(o.n, np.float32); g.ctx.d2h(g.ctx.lib.crux_mlp_grads_ptr(g.h), gg)
        scale = max(1.0, np.abs(o.grads).max()); dg = float(np.abs(gg - o.grads).max())
        dinfo = max(abs(float(raw[L.INFO[q]]) - float(oinfo[L.INFO[q]])) / max(1.0, abs(float(oinfo[L.INFO[q]]))) for q in ("loss", "grad_norm", "kl", "entropy", "clip_fraction", "avg_advantage", "avg_return"))
        _say("ROW_EDGES C %s n %d: gradient %.3g of scale %.3g, infos %.3g" % (LC.row_id(row), n, dg, scale, dinfo))
        assert dg < 1e-4 * scale, (row, n, dg)
        for q in ("loss", "grad_norm", "kl", "entropy", "clip_fraction", "avg_advantage", "avg_return"):
            assert abs(raw[L.INFO[q]] - oinfo[L.INFO[q]]) < 1e-4 * max(1.0, abs(oinfo[L.INFO[q]])), (row, n, q, raw[L.INFO[q]], oinfo[L.INFO[q]])
        assert np.array_equal(g.get_params(), o.params)                                   # gradient-only: parameters untouched
        for s in range(3):
            ids = rng.permutation(case.N)[:n].astype(np.int64)
            info = crux.train_(g, p, LC.PPO_P, gb, ids + 1)
            O.chk(O.lib().orc_train_step(o.h, ob.h, C.byref(cfg), O.vpz(ids), ids.size, O.vpz(oinfo)))
            assert abs(info["x_loss"] - oinfo[0]) < 1e-4 * max(1, abs(oinfo[0])), (row, n, s)
        m, v, bp = g.adam_state(); om, ov, obp = o.adam_state()
        dth, dm, ms = float(np.abs(g.get_params() - o.params).max()), float(np.abs(m - om).max()), float(np.abs(om).max())
        _say("ROW_EDGES C %s n %d after three steps: |dtheta| %.3g |dm| %.3g (|m_o|max %.3g)" % (LC.row_id(row), n, dth, dm, ms)); _note("C", dth, dm / max(1.0, ms))
        assert dth < 2e-5, (row, n, dth)
        assert dm <= 1e-5 * max(1.0, ms) and np.allclose(bp, obp, rtol=1e-12, atol=0), (row, n, dm, ms)
    _not_generic(capfd)


@pytest.mark.parametrize("k", range(len(LC.SMALL_ROWS)), ids=SMALL_IDS)
def test_small_minibatch_loops_at_row_edges(gpu_ctx, capfd, k):
    """full batch_train! loops of 16-, 33- and 64-row minibatches with tails of 1, 15 and 17 rows, as whole-epoch windows"""
    for bs in LC.SMALL_BS:
        for r in LC.SMALL_RS:
            _windows("C", LC.SMALL_ROWS[k], bs, r, LC.case_seed(400 + k, bs, r))      # (bs 16, r 17: four full minibatches and a tail of one)
    _not_generic(capfd)
