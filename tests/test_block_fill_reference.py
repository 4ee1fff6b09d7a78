"""CPU: tests/block_fill_reference.py (the yardstick of tests/test_gpu_block_fills.py) on hand-worked blocks, against the oracle's whole-buffer fills where the two
must agree, and -- the teeth -- on the GPU tests' own inputs: the rows of every grid case tell a scan that forgot the segments, one that closes every trailing
episode and one that reads V(s) at the physical row from the truth, wherever that mistake can be made at all.

Hand-worked numbers use gamma = lambda = 0.5 and dyadic inputs, so every intermediate is exact in Float32."""
import numpy as np
import pytest

import block_fill_reference as R

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. hand-worked blocks ------------------------------------------------------------------------------------------------------------------------------------------
def test_block_rows_are_the_ring_rows():
    assert R.block_rows(3, 4, 5).tolist() == [3, 4, 0, 1] and R.block_rows(0, 3, 3).tolist() == [0, 1, 2] and R.block_rows(4, 1, 5).tolist() == [4]


def test_episodes_by_hand():
    ee = [1, 0, 1, 0, 0]
    assert R.episodes(ee, 0, 1) == [(0, 0, True), (1, 2, True), (3, 4, True)] and R.episodes(ee, 0, 0) == [(0, 0, True), (1, 2, True), (3, 4, False)]
    # two rows per environment: row 1 trails its segment, row 4 is a segment of its own (n is no multiple of seg)
    assert R.episodes(ee, 2, 0) == [(0, 0, True), (1, 1, False), (2, 2, True), (3, 3, False), (4, 4, False)]


def test_returns_by_hand():
    r = [1, 2, 3, 4]
    # rows 0-1 end on :episode_end: R1 = 2, R0 = 1 + 2/2 = 2; rows 2-3 trail: R3 = 4, R2 = 3 + 4/2 = 5 when closed, the fresh block's zeros otherwise
    assert R.returns_block(r, [0, 1, 0, 0], 0.5, 0, 1).tolist() == [2.0, 2.0, 5.0, 4.0]
    assert R.returns_block(r, [0, 1, 0, 0], 0.5, 0, 0).tolist() == [2.0, 2.0, 0.0, 0.0]
    # two environments of two rows: the first one's rows trail ITS segment
    assert R.returns_block(r, [0, 0, 0, 1], 0.5, 2, 1).tolist() == [2.0, 2.0, 5.0, 4.0]
    assert R.returns_block(r, [0, 0, 0, 1], 0.5, 2, 0).tolist() == [0.0, 0.0, 5.0, 4.0]
    # one segment: the four rows are one episode: 4, 3 + 2, 2 + 2.5, 1 + 2.25
    assert R.returns_block(r, [0, 0, 0, 1], 0.5, 0, 0).tolist() == [3.25, 4.5, 5.0, 4.0]


def test_gae_by_hand():
    # c = 1/4. k = 2 (done): (0 + 4) + 0 - 3 = 1; k = 1: (1/4 + 2) + 3/2 - 2 = 1.75; k = 0: (1.75/4 + 1) + 2/2 - 1 = 1.4375
    assert R.gae_block([1, 2, 4], [0, 0, 1], [0, 0, 1], [1, 2, 3], [2, 3, 5], 0.5, 0.5, 0, 0).tolist() == [1.4375, 1.75, 1.0]
    # a one-row episode cut by the time limit (done = 0: it bootstraps, 1 + 2/2 - 1 = 1); rows 1-2 end in a terminal state: 4 - 1 = 3, (3/4 + 2) + 1 - 1 = 2.75;
    # rows 3-4 trail: (16 + 1) - 1 = 16, (16/4 + 8) + 1 - 1 = 12 when closed
    args = ([1, 2, 4, 8, 16], [0, 0, 1, 0, 0], [1, 0, 1, 0, 0], [1] * 5, [2] * 5, 0.5, 0.5)
    assert R.gae_block(*args, 0, 1).tolist() == [1.0, 2.75, 3.0, 12.0, 16.0]
    assert R.gae_block(*args, 0, 0).tolist() == [1.0, 2.75, 3.0, 0.0, 0.0]
    # three rows per environment: row 3 opens the second environment's only run
    assert R.gae_block(*args, 3, 1).tolist() == [1.0, 2.75, 3.0, 12.0, 16.0] and R.gae_block(*args, 4, 1).tolist() == [1.0, 2.75, 3.0, 8.0, 16.0]


def test_gae_association_is_the_references():
    """with inexact inputs the order of the roundings shows: ((c A + r) + ((1 - done) gamma) Vsp) - Vs, c = Float32(lam) Float32(gamma)"""
    lam, g = F(0.95), F(0.99); c = F(lam * g); r, Vs, Vsp = F(0.3), F(0.7), F(1.1)
    a1 = F(F(r + F(F(F(1) * g) * Vsp)) - Vs)
    a0 = F(F(F(F(c * a1) + r) + F(F(F(1) * g) * Vsp)) - Vs)
    got = R.gae_block([r, r], [0, 0], [0, 1], [Vs, Vs], [Vsp, Vsp], 0.95, 0.99, 0, 0)
    assert np.array_equal(_bits(got), _bits([a0, a1]))


def test_weight_products_by_hand():
    iw = [2, 0.25, 4, 0.5, 3]
    fwd, cum, rev = R.weight_products_block(iw, [0, 1, 0, 0, 0], 0, 1)
    assert fwd.tolist() == [2.0, 0.5, 4.0, 2.0, 6.0] and cum.tolist() == [0.5, 0.5, 6.0, 6.0, 6.0] and rev.tolist() == [0.5, 0.25, 6.0, 1.5, 3.0]
    fwd, cum, rev = R.weight_products_block(iw, [0, 1, 0, 0, 0], 0, 0)          # the open rows keep the fresh block's ones
    assert fwd.tolist() == [2.0, 0.5, 1.0, 1.0, 1.0] and cum.tolist() == [0.5, 0.5, 1.0, 1.0, 1.0] and rev.tolist() == [0.5, 0.25, 1.0, 1.0, 1.0]
    fwd, cum, rev = R.weight_products_block(iw, [0, 0, 0, 0, 1], 2, 1)          # environments of two rows: (2, 1/4), (4, 1/2), (3)
    assert fwd.tolist() == [2.0, 0.5, 4.0, 2.0, 3.0] and cum.tolist() == [0.5, 0.5, 2.0, 2.0, 3.0] and rev.tolist() == [0.5, 0.25, 2.0, 0.5, 3.0]


def test_importance_ratios_by_hand():
    h = R.LOG_SQRT_2PI
    assert R.gaussian_iw([[0.0]], [0.0], [[0.0]], [-h])[0] == 1.0
    assert abs(R.gaussian_iw([[1.0]], [0.0], [[2.0]], [-h])[0] - 0.6065306597126334) < 1e-15                       # exp(-1/2)
    # two dimensions, sigma = (1, 2): -(1)^2/2 - h - 0  and  -(2)^2/(2 4) - h - log 2; against logprob = -2 h: exp(-1 - log 2) = 1/(2 e)
    assert abs(R.gaussian_iw([[0.0], [1.0]], [0.0, np.log(2.0)], [[1.0], [3.0]], [-2 * h])[0] - 0.5 / np.e) < 1e-15
    assert abs(R.categorical_iw([[0.0], [np.log(3.0)]], [[0], [1]], [np.log(0.5)])[0] - 1.5) < 1e-15               # softmax = (1/4, 3/4)
    assert abs(R.categorical_iw([[5.0], [5.0], [5.0]], [[1], [0], [0]], [0.0])[0] - 1 / 3) < 1e-15
    got = R.gaussian_iw_f32([[0.0], [1.0]], [0.0, np.log(2.0)], [[1.0], [3.0]], [-2 * h])
    assert got.dtype == F and abs(float(got[0]) - 0.5 / np.e) < 1e-6


def test_mlp_by_hand():
    p = np.array([1, 2, 3, 4, 0.5, -20, 1, 1, 0.25], F)      # W1 = [[1, 3], [2, 4]] column-major, b1 = (0.5, -20); W2 = [1, 1], b2 = 0.25
    assert R.mlp(p, [2, 2, 1], ["relu", "identity"], [[1.0], [2.0]]).tolist() == [[7.75]]      # relu(7.5, -10) -> 7.5 + 0.25


# ---- 2. one segment, close_last = 1: the whole-buffer fills of the oracle --------------------------------------------------------------------------------------------
def test_one_closed_segment_is_the_oracles_whole_buffer_fill():
    """fill_returns!(b, gamma) / fill_gae!(b, V, lambda, gamma) over episodes(b) (sampler.jl:255-281, experience_buffer.jl:194-212: a trailing episode is closed at
    length(b)) as the oracle restates them: the block scans with one segment and close_last = 1, bit for bit"""
    import oracle as O
    L = O.L
    c = R.block_case(3); n = c["n"]
    ob = O.OBuffer(R.OBS_DIM, 1, L.ACTION_CONTINUOUS, n, ["return", "advantage"])
    ob.push({k: c[k] for k in ("s", "a", "sp", "r", "done", "episode_end")})
    net = O.OMlp(c["dims"], c["acts"]); net.params[:] = c["pV"]
    O.chk(O.lib().orc_fill_returns(ob.h, R.GAMMA)); O.chk(O.lib().orc_fill_gae(ob.h, net.h, R.LAM, R.GAMMA))
    assert np.array_equal(_bits(ob["return"][0]), _bits(R.returns_block(c["r"], c["episode_end"], R.GAMMA, 0, 1)))
    Vs, Vsp = net.forward(c["s"])[0], net.forward(c["sp"])[0]
    assert np.array_equal(_bits(ob["advantage"][0]), _bits(R.gae_block(c["r"], c["done"], c["episode_end"], Vs, Vsp, R.LAM, R.GAMMA, 0, 1)))


# ---- 3. the GPU tests' inputs ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(R.GRID))
def test_grid_case_has_the_engineered_rows(cid):
    c = R.block_case(cid); E, T, n, cap, first = c["E"], c["T"], c["n"], c["cap"], c["first"]
    ee, done = c["episode_end"], c["done"]; phys = R.block_rows(first, n, cap)
    assert n == E * T and n > 256 and T % 64 != 0 and n <= cap and len(set(phys.tolist())) == n
    if c["rows_per_env"] > 0:
        segs = [ee[e * T:(e + 1) * T] for e in range(E)]
        assert any(s[-1] for s in segs) and any(s[0] for s in segs) and not segs[c["empty_segment"]].any()
        assert any(not s[-1] for s in segs[:-1])                                  # an episode still open where the next environment's rows begin
    else:                                                                         # one segment: its first row is an episode, its last row is open, a run crosses row 2 T
        assert c["seg"] == n and ee[0] and not ee[-1] and not ee[2 * T - 1] and ee[2 * T:].any()
    for q in (cap - 1, 0):
        assert q not in phys or ee[phys == q][0], "physical row %d lies in the block without an :episode_end" % q
    assert (done & ee).any() and (ee & ~done).any() and not (done & ~ee).any()   # terminal states and time-limit cuts
    assert 0.015 < ee.mean() < 0.06                                              # about 4 % on two of three segments
    if cid == 8:
        assert min(cap - first, n - (cap - first)) >= 1024 and c["dims"] == [4, 64, 64, 1]
    else:
        assert c["dims"] == [4, 32, 32, 1]
    assert {2: first + n == cap, 3: first + n == cap + 1, 6: n == cap}.get(cid, True)


def _scans(c, close_last):
    """[(name, scan, columns, extra keywords)] of a case; V(s), V(sp) from numpy"""
    Vs, Vsp = R.case_values(c); ee = c["episode_end"]
    return [("gae", R.gae_block, (c["r"], c["done"], ee, Vs, Vsp, R.LAM, R.GAMMA)), ("cost_gae", R.gae_block, (c["cost"], c["done"], ee, *R.case_values(c, "pVc"), R.LAM, R.GAMMA)),
            ("returns", R.returns_block, (c["r"], ee, R.GAMMA)), ("cost_returns", R.returns_block, (c["cost"], ee, R.GAMMA)),
            ("products", lambda *a, **k: np.stack(R.weight_products_block(*a, **k)), (c["importance_weight"], ee))]


def _differs(a, b):
    return bool((_bits(a) != _bits(b)).any())


@pytest.mark.parametrize("close_last", [0, 1])
@pytest.mark.parametrize("cid", sorted(R.GRID))
def test_grid_case_tells_the_wrong_scans_apart(cid, close_last):
    """Every scan of every grid case, against the three wrong scans. A mistake that cannot be made leaves nothing to tell apart, and only then is nothing asked:
      ignore_segments   needs more than one segment: not case 7 (rows_per_env = 0 IS one segment; there the opposite mistake, a scan split every T rows, must differ).
                        With close_last = 0 it also needs an open run that a LATER closed episode would swallow: in case 4 the rows at physical cap-1 and 0 are the
                        last row of segment 0 and the first of segment 1, which leaves segment 2 as the one without an :episode_end -- segment 1's open tail
                        and all of segment 2 hold the fresh block's values either way (close_last = 1 tells them apart there).
      always_close      needs close_last = 0.
      physical_values   needs first != 0 (case 1: the physical row IS the block row); advantages only."""
    c = R.block_case(cid); kw = {"seg": c["rows_per_env"], "close_last": close_last}
    for name, scan, cols in _scans(c, close_last):
        truth = scan(*cols, **kw)
        assert np.isfinite(truth).all() and np.abs(truth).max() < 1e6, name            # no product over- or underflows
        if c["rows_per_env"] > 0:
            if close_last or c["empty_segment"] != c["E"] - 1:
                assert _differs(R.ignore_segments(scan, *cols, **kw), truth), (name, "ignore_segments")
        else:
            assert _differs(scan(*cols, seg=c["T"], close_last=close_last), truth), (name, "split where one segment is meant")
        if not close_last:
            assert _differs(R.always_close(scan, *cols, **kw), truth), (name, "always_close")
            still_open = [k for a, b, closed in R.episodes(c["episode_end"], kw["seg"], 0) if not closed for k in range(a, b + 1)]
            assert len(still_open) > 1 and (truth[..., still_open] == (1.0 if name == "products" else 0.0)).all()
        if c["first"] and name.endswith("gae"):
            assert _differs(R.physical_values(*cols, **kw, first=c["first"], cap=c["cap"]), truth), (name, "physical_values")
    assert cid in (4, 7) or c["empty_segment"] != c["E"] - 1      # the exception above is case 4's alone (case 7 has one segment and no empty one)


@pytest.mark.parametrize("cid", [1, 6])
def test_whole_buffer_cases_tell_the_wrong_whole_buffer_scans_apart(cid):
    """The whole-buffer fills scan the PHYSICAL rows 0 .. length(b)-1 as one closed segment. On the rings of cases 1 and 6 (test_gpu_block_fills.py) that differs from
    a scan that leaves the trailing run open (case 1: the last physical row is no :episode_end), from one cut every T rows, and -- case 6, next_ind at 200 -- from the
    ring's rows scanned in push order."""
    c = R.block_case(cid); p, m = R.ring_columns(c); ee = p["episode_end"]; T = c["T"]
    assert m == 390 and (c["first"] + c["n"]) % c["cap"] == {1: 390, 6: 200}[cid]
    Vs, Vsp = (R.mlp(c["pV"], c["dims"], c["acts"], p[k], F)[0] for k in ("s", "sp"))
    scans = [("returns", R.returns_block, (p["r"], ee, R.GAMMA)), ("gae", R.gae_block, (p["r"], p["done"], ee, Vs, Vsp, R.LAM, R.GAMMA))]
    rows = R.block_rows(c["first"], c["n"], c["cap"])            # push order IS block order: block row k lies at physical row rows[k]
    block_order = [(c["r"], c["episode_end"], R.GAMMA), (c["r"], c["done"], c["episode_end"], *R.case_values(c), R.LAM, R.GAMMA)]
    for (name, scan, cols), pushed in zip(scans, block_order):
        truth = scan(*cols, seg=0, close_last=1)
        assert _differs(scan(*cols, seg=T, close_last=1), truth), (name, "T-row segments")
        if cid == 1:
            assert not ee[m - 1] and _differs(scan(*cols, seg=0, close_last=0), truth), (name, "trailing run left open")
        else:
            in_push_order = np.empty(m, F); in_push_order[rows] = scan(*pushed, seg=0, close_last=1)
            assert _differs(in_push_order, truth), (name, "push order")


def test_nan_rows_of_the_gpu_test_sit_where_they_must():
    """the NaN-reward rows of test_gpu_block_fills.py: a wrapped block row inside a CLOSED episode (whatever close_last), and a ring row outside the block"""
    for cid in (3, 4):
        c = R.block_case(cid); k = R.nan_row(c); phys = R.block_rows(c["first"], c["n"], c["cap"])
        assert phys[k] < c["first"] and k >= c["cap"] - c["first"]
        assert any(a <= k <= b and closed for a, b, closed in R.episodes(c["episode_end"], c["rows_per_env"], 0))
        assert R.outside_row(c) not in phys


# ---- 4. the per-step ratio's inputs and its tolerance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.IW_HEADS))
def test_weight_case_keeps_the_ratios_moderate(name):
    c = R.weight_case(name); ref = R.iw_reference(c)
    assert np.abs(c["nominal_logpdf"] - c["logprob"].astype(np.float64)).max() <= 3.0
    assert np.exp(-3.0) <= ref.min() and ref.max() <= np.exp(3.0)
    assert R.IW_FIRST > 0 and R.IW_ROWS > 256 and R.IW_FIRST + R.IW_ROWS < R.IW_CAP
    if c["disc"]:
        assert (c["a"].sum(axis=0) == 1).all() and c["a"].any(axis=1).all()          # one-hot columns, every action taken
    else:
        assert np.array_equal(c["p"][-c["ad"]:], R.LOG_SIGMA[:c["ad"]])


@pytest.mark.parametrize("name", ["gaussian1", "gaussian3"])
def test_gaussian_ratio_tolerance_is_sized_by_the_float32_replica(name):
    """How far a Float32 evaluation in the kernel's association strays from float64 on these very inputs: 9.9e-7 (act_dim 1) and 1.05e-6 (act_dim 3) of the column's
    maximum. Four times that stays under the categorical head's 5e-6, so 5e-6 is the bound of the GPU test."""
    dev = R.iw_f32_deviation(R.weight_case(name))
    print("%s: Float32 replica against float64: %.3g of the column's maximum (recorded %.3g)" % (name, dev, R.IW_MEASURED[name]))
    assert 0 < dev <= R.IW_MEASURED[name]
    assert R.iw_tolerance(name) == max(5e-6, 4 * R.IW_MEASURED[name]) == 5e-6 and R.iw_tolerance("categorical3") == 5e-6
