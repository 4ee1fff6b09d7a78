"""GPU: what every steps! call leaves on the ring rows [first, first + n) mod capacity of the block it produced (csrc/advantage.hip: k_gae_returns,
k_importance_weight, k_importance_fills behind crux_fill_gae_rows[_keys], crux_fill_returns_rows[_keys], crux_importance_weight_rows and
crux_fill_importance_weights_rows) against the plain scans of tests/block_fill_reference.py.

The scans are sequential Float32 recurrences, so :return, :cost_return, :advantage, :cost_advantage (given the library's own V(s), V(sp) of the block's rows) and the
fwd_ / cum_ / rev_ products are compared BIT FOR BIT; the per-step ratio is compared with float64 to 5e-6 of the column's maximum (block_fill_reference.iw_tolerance:
the Float32 replica strays 9.9e-7 / 1.05e-6 from float64 on these inputs, four times that stays under the categorical head's bound). Every target column is pre-set to
a sentinel bit pattern over the whole ring: rows outside the block must keep it. The inputs (block_fill_reference.GRID) are shown on the CPU to tell a scan that forgets
the segments, closes every trailing episode or reads V at the physical row from the truth (tests/test_block_fill_reference.py).

Reference: src/sampler.jl:53-66,108-111,139-155,255-308, src/policies.jl:128-135,333-336, src/experience_buffer.jl:4-35,194-259."""
import numpy as np
import pytest

import block_fill_reference as R
import parity
from crux_jl_amd.api import _np_dtype
from parity import crux, L

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = np.array([0x7FC5A5A5], np.uint32).view(F)[0]      # a quiet NaN with a payload no scan produces
EXTRAS = ["return", "advantage", "cost", "cost_advantage", "cost_return", "logprob", "importance_weight", "fwd_importance_weight", "cum_importance_weight", "rev_importance_weight"]
PUSHED = ("s", "a", "sp", "r", "done", "episode_end", "cost", "importance_weight")
GRID_IDS = sorted(R.GRID)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _get(buf, key):
    """a column over the WHOLE ring (b[key] stops at length(b)): [rows x capacity]"""
    out = np.empty(buf._shape(key, buf.capacity), _np_dtype(key, buf.act_kind), order="F")
    return buf.ctx.d2h(buf.column_ptr(key), out)


def _put(buf, key, v):
    v = np.asfortranarray(np.broadcast_to(np.asarray(v, _np_dtype(key, buf.act_kind)), buf._shape(key, buf.capacity)))
    buf.ctx.h2d(buf.column_ptr(key), v)


def _net(ctx, dims, acts, p):
    n = crux.ContinuousNetwork(parity.chain(dims, acts), ctx=ctx); n.set_params(p); return n


class Ring:
    """a grid case on the device: junk over the whole ring, `first` junk rows pushed to place next_ind, then the block; the two critics and their values of the block"""

    def __init__(self, ctx, cid):
        c = self.c = R.block_case(cid); cap, first, n = c["cap"], c["first"], c["n"]
        b = self.buf = crux.ExperienceBuffer(crux.ContinuousSpace(R.OBS_DIM), crux.ContinuousSpace(1), cap, EXTRAS, ctx=ctx)
        for k in PUSHED:
            _put(b, k, c["junk"][k])
        if first:
            b.push_({k: c["junk"][k][..., :first] for k in PUSHED})
        assert b.next_ind - 1 == first
        b.push_({k: c[k] for k in PUSHED})
        assert b.next_ind - 1 == (first + n) % cap and len(b) == min(cap, first + n)
        self.rows = R.block_rows(first, n, cap); self.outside = np.setdiff1d(np.arange(cap), self.rows)
        assert np.array_equal(_get(b, "episode_end")[0, self.rows], c["episode_end"]) and np.array_equal(_bits(_get(b, "r")[0, self.rows]), _bits(c["r"]))
        self.V, self.Vc = _net(ctx, c["dims"], c["acts"], c["pV"]), _net(ctx, c["dims"], c["acts"], c["pVc"])
        # V(s), V(sp) of the block's rows in block order from the library's own forward (the generic and the matrix-pipe kernel agree bit for bit: test_gpu_components.py)
        self.values = {id(q): (q.forward(c["s"])[0], q.forward(c["sp"])[0]) for q in (self.V, self.Vc)}
        self.args = (first, n, c["rows_per_env"])

    def check(self, key, want, what):
        col = _get(self.buf, key)[0]
        bad = np.flatnonzero(_bits(col[self.rows]) != _bits(want))
        assert bad.size == 0, "%s: %d of %d block rows differ, first at block row %d (physical %d): %r, expected %r" % (
            what, bad.size, want.size, bad[0], self.rows[bad[0]], col[self.rows[bad[0]]], want[bad[0]])
        assert (_bits(col[self.outside]) == _bits(SENTINEL)).all(), "%s: rows outside the block were written: physical %s" % (
            what, self.outside[_bits(col[self.outside]) != _bits(SENTINEL)][:8])


_RINGS = {}


def _ring(ctx, cid):
    if cid not in _RINGS:
        _RINGS[cid] = Ring(ctx, cid)
    return _RINGS[cid]


# ---- 1. returns and advantages on the grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("close_last", [0, 1])
@pytest.mark.parametrize("cid", GRID_IDS)
def test_returns_and_advantages_of_a_ring_block_equal_the_plain_scan(gpu_ctx, cid, close_last):
    g = _ring(gpu_ctx, cid); c, b, lib = g.c, g.buf, gpu_ctx.lib; ee = c["episode_end"]; kw = {"seg": c["rows_per_env"], "close_last": close_last}
    for k in ("return", "cost_return", "advantage", "cost_advantage"):
        _put(b, k, SENTINEL)
    gpu_ctx.check(lib.crux_fill_returns_rows(b.h, R.GAMMA, *g.args, close_last))
    g.check("return", R.returns_block(c["r"], ee, R.GAMMA, **kw), "crux_fill_returns_rows")
    gpu_ctx.check(lib.crux_fill_returns_rows_keys(b.h, R.GAMMA, *g.args, close_last, L.COL["cost"], L.COL["cost_return"]))
    g.check("cost_return", R.returns_block(c["cost"], ee, R.GAMMA, **kw), "crux_fill_returns_rows_keys(:cost -> :cost_return)")
    gpu_ctx.check(lib.crux_fill_gae_rows(b.h, g.V.h, R.LAM, R.GAMMA, *g.args, close_last))
    g.check("advantage", R.gae_block(c["r"], c["done"], ee, *g.values[id(g.V)], R.LAM, R.GAMMA, **kw), "crux_fill_gae_rows")
    gpu_ctx.check(lib.crux_fill_gae_rows_keys(b.h, g.Vc.h, R.LAM, R.GAMMA, *g.args, close_last, L.COL["cost"], L.COL["cost_advantage"]))
    g.check("cost_advantage", R.gae_block(c["cost"], c["done"], ee, *g.values[id(g.Vc)], R.LAM, R.GAMMA, **kw), "crux_fill_gae_rows_keys(:cost -> :cost_advantage)")
    g.check("return", R.returns_block(c["r"], ee, R.GAMMA, **kw), ":return after the other three fills")      # (each fill writes its own target only)


@pytest.mark.parametrize("close_last", [0, 1])
@pytest.mark.parametrize("cid", [3, 4])
def test_nan_reward_is_reported_from_a_wrapped_row_and_ignored_outside_the_block(gpu_ctx, cid, close_last):
    """@assert !isnan(A) (sampler.jl:270) looks at the block's rows, wherever the ring put them, and at no other row"""
    g = _ring(gpu_ctx, cid); c, b, lib = g.c, g.buf, gpu_ctx.lib
    r0 = _get(b, "r")
    try:
        r = r0.copy(); r[0, R.outside_row(c)] = np.nan; _put(b, "r", r); _put(b, "advantage", SENTINEL)
        assert lib.crux_fill_gae_rows(b.h, g.V.h, R.LAM, R.GAMMA, *g.args, close_last) == L.OK
        g.check("advantage", R.gae_block(c["r"], c["done"], c["episode_end"], *g.values[id(g.V)], R.LAM, R.GAMMA, seg=c["rows_per_env"], close_last=close_last), "NaN outside the block")
        r = r0.copy(); r[0, g.rows[R.nan_row(c)]] = np.nan; _put(b, "r", r)
        assert g.rows[R.nan_row(c)] < c["first"]                                  # past the wrap
        assert lib.crux_fill_gae_rows(b.h, g.V.h, R.LAM, R.GAMMA, *g.args, close_last) == L.ENAN
        assert "NaN advantage" in (lib.crux_last_error(gpu_ctx.h) or b"").decode()
    finally:
        _put(b, "r", r0)


# ---- 1b. the whole-buffer forms: the physical rows 0 .. length(b)-1 as one closed segment, wherever next_ind stands ----------------------------------------------------
WHOLE_KEYS = ("return", "cost_return", "advantage", "cost_advantage")


def _whole_fills(lib, ctx, b, V, Vc, rows=None):
    """the four fills through the whole-buffer entry points, or through the _rows forms on `rows` = (first_row, n_rows, rows_per_env, close_last)"""
    cost = (L.COL["cost"], L.COL["cost_return"]), (L.COL["cost"], L.COL["cost_advantage"])
    if rows is None:
        rcs = [lib.crux_fill_returns(b.h, R.GAMMA), lib.crux_fill_returns_keys(b.h, R.GAMMA, *cost[0]),
               lib.crux_fill_gae(b.h, V.h, R.LAM, R.GAMMA), lib.crux_fill_gae_keys(b.h, Vc.h, R.LAM, R.GAMMA, *cost[1])]
    else:
        rcs = [lib.crux_fill_returns_rows(b.h, R.GAMMA, *rows), lib.crux_fill_returns_rows_keys(b.h, R.GAMMA, *rows, *cost[0]),
               lib.crux_fill_gae_rows(b.h, V.h, R.LAM, R.GAMMA, *rows), lib.crux_fill_gae_rows_keys(b.h, Vc.h, R.LAM, R.GAMMA, *rows, *cost[1])]
    for rc in rcs:
        ctx.check(rc)


@pytest.mark.parametrize("cid", [1, 6])
def test_whole_buffer_fills_scan_the_physical_rows_as_one_closed_segment(gpu_ctx, cid):
    """crux_fill_returns[_keys] / crux_fill_gae[_keys] on case 1 (390 rows in a ring of 500, next_ind at 390) and case 6 (a full ring of 390 that wrapped, next_ind at
    200) against the plain scans of the PHYSICAL columns with seg = 0, close_last = 1; the _rows forms on (0, length(b), 0, 1) write the same bits. What makes the
    wrong scans (push order, T-row segments, an open trailing run) show on these rows: tests/test_block_fill_reference.py."""
    g = _ring(gpu_ctx, cid); b, lib = g.buf, gpu_ctx.lib; n = len(b); cap = b.capacity
    assert (n, cap, b.next_ind - 1) == {1: (390, 500, 390), 6: (390, 390, 200)}[cid]
    phys = {k: _get(b, k)[..., :n] for k in ("s", "sp", "r", "cost", "done", "episode_end")}
    r, cost, done, ee = (phys[k][0] for k in ("r", "cost", "done", "episode_end"))
    want = {"return": R.returns_block(r, ee, R.GAMMA, seg=0, close_last=1), "cost_return": R.returns_block(cost, ee, R.GAMMA, seg=0, close_last=1),
            "advantage": R.gae_block(r, done, ee, g.V.forward(phys["s"])[0], g.V.forward(phys["sp"])[0], R.LAM, R.GAMMA, seg=0, close_last=1),
            "cost_advantage": R.gae_block(cost, done, ee, g.Vc.forward(phys["s"])[0], g.Vc.forward(phys["sp"])[0], R.LAM, R.GAMMA, seg=0, close_last=1)}
    for k in WHOLE_KEYS:
        _put(b, k, SENTINEL)
    _whole_fills(lib, gpu_ctx, b, g.V, g.Vc)
    whole = {k: _get(b, k)[0] for k in WHOLE_KEYS}
    for k in WHOLE_KEYS:
        bad = np.flatnonzero(_bits(whole[k][:n]) != _bits(want[k]))
        assert bad.size == 0, "whole-buffer :%s: %d of %d rows differ, first at physical row %d: %r, expected %r" % (k, bad.size, n, bad[0], whole[k][bad[0]], want[k][bad[0]])
        assert (_bits(whole[k][n:]) == _bits(SENTINEL)).all(), "whole-buffer :%s: rows past length(b) were written" % k
    for k in WHOLE_KEYS:
        _put(b, k, SENTINEL)
    _whole_fills(lib, gpu_ctx, b, g.V, g.Vc, rows=(0, n, 0, 1))
    for k in WHOLE_KEYS:
        assert np.array_equal(_bits(_get(b, k)[0]), _bits(whole[k])), "the _rows form on (0, length(b), 0, 1) and the whole-buffer form differ in :" + k


def test_whole_buffer_fills_of_an_empty_buffer_write_nothing(gpu_ctx):
    b = crux.ExperienceBuffer(crux.ContinuousSpace(R.OBS_DIM), crux.ContinuousSpace(1), 8, EXTRAS, ctx=gpu_ctx)
    c = R.block_case(1); V = _net(gpu_ctx, c["dims"], c["acts"], c["pV"])
    assert len(b) == 0
    for k in WHOLE_KEYS:
        _put(b, k, SENTINEL)
    _whole_fills(gpu_ctx.lib, gpu_ctx, b, V, V)                     # every call returns CRUX_OK
    for k in WHOLE_KEYS:
        assert (_bits(_get(b, k)) == _bits(SENTINEL)).all(), k


def _unequal_pair(ctx, nan_at=None):
    """two buffers of 96 rows (capacity 128) and 130 rows (full) with critics 4-32-32-1 and 4-16-16-1; :advantage and :return pre-set to the sentinel"""
    out = []
    for j, (n, cap, hidden) in enumerate(((96, 128, 32), (130, 130, 16))):
        rng = np.random.default_rng(3000 + j); dims = [R.OBS_DIM, hidden, hidden, 1]
        ee = rng.random(n) < 0.05; done = ee & (rng.random(n) < 0.5)
        r = rng.normal(0, 1, n).astype(F)
        if nan_at is not None and j == 1:
            r[nan_at] = np.nan
        b = crux.ExperienceBuffer(crux.ContinuousSpace(R.OBS_DIM), crux.ContinuousSpace(1), cap, ["return", "advantage"], ctx=ctx)
        b.push_({"s": rng.normal(0, 1, (R.OBS_DIM, n)).astype(F), "a": rng.uniform(-1, 1, (1, n)).astype(F), "sp": rng.normal(0, 1, (R.OBS_DIM, n)).astype(F),
                 "r": r, "done": done, "episode_end": ee})
        assert len(b) == n and ee.sum() >= 2 and not ee[-1]
        for k in ("return", "advantage"):
            _put(b, k, SENTINEL)
        out.append((b, _net(ctx, dims, R.ACTS, R.init_params(dims, rng))))
    return out


def _fill_multi(lib, pairs, with_returns=1):
    import ctypes as C
    hb = (C.c_void_p * len(pairs))(*[b.h for b, _ in pairs]); hc = (C.c_void_p * len(pairs))(*[V.h for _, V in pairs])
    return lib.crux_fill_gae_multi(len(pairs), hb, hc, R.LAM, R.GAMMA, with_returns)


def test_fill_gae_multi_of_unequal_buffers_equals_the_single_fills(gpu_ctx):
    """buffers of different lengths and critics of different widths take crux_fill_gae_multi's one-buffer-after-the-other branch: bit for bit what crux_fill_gae +
    crux_fill_returns leave on twin buffers (rows past length(b) untouched); a NaN reward in the second buffer is reported as buffer 1's"""
    lib = gpu_ctx.lib; multi, single = _unequal_pair(gpu_ctx), _unequal_pair(gpu_ctx)
    gpu_ctx.check(_fill_multi(lib, multi))
    for j, ((bm, _), (bs, V)) in enumerate(zip(multi, single)):
        gpu_ctx.check(lib.crux_fill_gae(bs.h, V.h, R.LAM, R.GAMMA)); gpu_ctx.check(lib.crux_fill_returns(bs.h, R.GAMMA))
        for k in ("advantage", "return"):
            got, want = _get(bm, k)[0], _get(bs, k)[0]
            assert np.isfinite(want[:len(bs)]).all() and (_bits(want[len(bs):]) == _bits(SENTINEL)).all()
            assert np.array_equal(_bits(got), _bits(want)), "buffer %d :%s" % (j, k)
    assert _fill_multi(lib, _unequal_pair(gpu_ctx, nan_at=57)) == L.ENAN
    msg = (lib.crux_last_error(gpu_ctx.h) or b"").decode()
    assert "NaN advantage" in msg and "buffer 1" in msg, msg


# ---- 2. the running products ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("close_last", [0, 1])
@pytest.mark.parametrize("cid", R.WEIGHT_CASES)
def test_importance_weight_products_of_a_ring_block_equal_the_plain_scan(gpu_ctx, cid, close_last):
    g = _ring(gpu_ctx, cid); c, b, lib = g.c, g.buf, gpu_ctx.lib
    keys = ("fwd_importance_weight", "cum_importance_weight", "rev_importance_weight")
    for k in keys:
        _put(b, k, SENTINEL)
    iw0 = _get(b, "importance_weight")
    assert 0.7 <= c["importance_weight"].min() and c["importance_weight"].max() <= 1.4
    gpu_ctx.check(lib.crux_fill_importance_weights_rows(b.h, *g.args, close_last))
    want = R.weight_products_block(c["importance_weight"], c["episode_end"], c["rows_per_env"], close_last)
    for k, w in zip(keys, want):
        g.check(k, w, "crux_fill_importance_weights_rows :" + k)
    assert np.array_equal(_bits(_get(b, "importance_weight")), _bits(iw0))
    still_open = [k for a, z, closed in R.episodes(c["episode_end"], c["rows_per_env"], close_last) if not closed for k in range(a, z + 1)]
    assert (len(still_open) > 0) == (close_last == 0)
    for k in keys:
        assert (_get(b, k)[0, g.rows[still_open]] == 1.0).all(), k               # the fresh block's ones (experience_buffer.jl:17-19)


# ---- 3. the per-step ratio ------------------------------------------------------------------------------------------------------------------------------------------
def _nominal(ctx, c, squashed=False):
    ch = parity.chain(c["dims"], c["acts"])
    if c["disc"]:
        pa = crux.DiscreteNetwork(ch, list(range(1, c["ad"] + 1)), ctx=ctx)
    elif squashed:
        pa = crux.SquashedGaussianPolicy(ch, c["log_sigma"], ascale=1.0, ctx=ctx)
    else:
        pa = crux.GaussianPolicy(ch, c["log_sigma"], ctx=ctx)
    pa.set_params(c["p"]); return pa


def _weight_ring(ctx, c):
    A = crux.DiscreteSpace(c["ad"]) if c["disc"] else crux.ContinuousSpace(c["ad"])
    b = crux.ExperienceBuffer(crux.ContinuousSpace(R.OBS_DIM), A, R.IW_CAP, ["logprob", "importance_weight"], ctx=ctx)
    n = R.IW_CAP
    b.push_({"s": c["s"], "a": c["a"], "sp": c["s"], "r": np.zeros(n, F), "done": np.zeros(n, bool), "episode_end": np.zeros(n, bool), "logprob": c["logprob"]})
    assert len(b) == n
    return b


@pytest.mark.parametrize("name", sorted(R.IW_HEADS))
def test_importance_weight_rows_match_float64(gpu_ctx, name):
    """exp.(logpdf(pa, s, a) .- logprob) (sampler.jl:108-111) on the rows [37, 337) of a ring of 700: Gaussian nominal policies of 1 and 3 action dimensions, a categorical
    one of 3 actions. Bound: 5e-6 of the column's maximum (see the module docstring)."""
    c = R.weight_case(name); b = _weight_ring(gpu_ctx, c); pa = _nominal(gpu_ctx, c)
    head = L.HEAD["categorical" if c["disc"] else "gaussian"]; lo, hi = R.IW_FIRST, R.IW_FIRST + R.IW_ROWS
    _put(b, "importance_weight", SENTINEL)
    gpu_ctx.check(gpu_ctx.lib.crux_importance_weight_rows(b.h, pa.h, head, lo, R.IW_ROWS))
    col = _get(b, "importance_weight")[0]; ref = R.iw_reference(c)[lo:hi]
    inside = np.zeros(R.IW_CAP, bool); inside[lo:hi] = True
    assert (_bits(col[~inside]) == _bits(SENTINEL)).all(), "rows outside [%d, %d) were written" % (lo, hi)
    dev = float(np.abs(col[lo:hi].astype(np.float64) - ref).max() / np.abs(ref).max())
    print("importance_weight %s: max deviation from float64 %.3g of the column's maximum %.3g (bound %.3g)" % (name, dev, np.abs(ref).max(), R.iw_tolerance(name)))
    assert np.isfinite(col[lo:hi]).all() and dev <= R.iw_tolerance(name), dev
    # the first range of a wrapped block ends exactly at the capacity
    _put(b, "importance_weight", SENTINEL)
    gpu_ctx.check(gpu_ctx.lib.crux_importance_weight_rows(b.h, pa.h, head, R.IW_CAP - 3, 3))
    col = _get(b, "importance_weight")[0]; ref = R.iw_reference(c)
    assert (_bits(col[:-3]) == _bits(SENTINEL)).all() and np.abs(col[-3:] - ref[-3:]).max() <= R.iw_tolerance(name) * np.abs(ref).max()


def test_importance_weight_rows_refuses_what_it_cannot_do(gpu_ctx):
    lib = gpu_ctx.lib; G, K = L.HEAD["gaussian"], L.HEAD["categorical"]
    cg, cc = R.weight_case("gaussian3"), R.weight_case("categorical3")
    bg, bc = _weight_ring(gpu_ctx, cg), _weight_ring(gpu_ctx, cc); pg, pc = _nominal(gpu_ctx, cg), _nominal(gpu_ctx, cc)
    _put(bg, "importance_weight", SENTINEL); _put(bc, "importance_weight", SENTINEL)

    def refused(rc, code, word):
        msg = (lib.crux_last_error(gpu_ctx.h) or b"").decode()
        assert rc == code and word in msg, (rc, msg)
    refused(lib.crux_importance_weight_rows(bg.h, pg.h, G, R.IW_CAP - 10, 11), L.EINVAL, "outside the buffer")               # a range past capacity (a wrapped block takes two calls)
    refused(lib.crux_importance_weight_rows(bg.h, pg.h, G, -1, 5), L.EINVAL, "outside the buffer")
    refused(lib.crux_importance_weight_rows(bg.h, pg.h, K, 0, 5), L.EINVAL, "Gaussian")                                       # the wrong head, both ways
    refused(lib.crux_importance_weight_rows(bc.h, pc.h, G, 0, 5), L.EINVAL, "categorical")
    plain = _net(gpu_ctx, cg["dims"], cg["acts"], cg["p"][:-cg["ad"]])                                                         # the same mu network without logSigma
    refused(lib.crux_importance_weight_rows(bg.h, plain.h, G, 0, 5), L.EINVAL, "logSigma")
    narrow, squashed = _nominal(gpu_ctx, R.weight_case("gaussian1")), _nominal(gpu_ctx, cg, squashed=True)      # (named: the handles must outlive the calls)
    refused(lib.crux_importance_weight_rows(bg.h, narrow.h, G, 0, 5), L.EINVAL, "obs(")                                       # act_dim 1 for a buffer of 3
    refused(lib.crux_importance_weight_rows(bg.h, squashed.h, G, 0, 5), L.EUNSUP, "Squashed")
    for b in (bg, bc):                                                                                                          # and nothing was written
        assert (_bits(_get(b, "importance_weight")) == _bits(SENTINEL)).all()


# ---- 4. end to end: steps! ------------------------------------------------------------------------------------------------------------------------------------------
E2E_EXTRAS = ["return", "advantage", "logprob", "importance_weight", "fwd_importance_weight", "cum_importance_weight", "rev_importance_weight"]
E2E_FILLED = E2E_EXTRAS[:2] + E2E_EXTRAS[3:]
E2E_DIMS, E2E_ACTS, E2E_LS = [3, 32, 32, 1], ["tanh", "tanh", "identity"], np.array([-0.4], F)


def _host_pendulum(E, seed):
    """a pendulum stepped on the host (float64 state (theta, omega)); leaving |omega| < 4 is terminal, so that some episodes end with :done"""
    def initialstate(e, n_resets):
        rng = np.random.default_rng([seed, e, n_resets]); return np.array([rng.uniform(-np.pi, np.pi), rng.uniform(-1.0, 1.0)])

    def gen(e, s, a, n_steps):
        th, om = s; u = float(np.clip(a[0], -2.0, 2.0))
        om2 = om + 0.05 * (15.0 * np.sin(th) + 3.0 * u); th2 = th + 0.05 * om2
        return np.array([th2, om2]), -(((th + np.pi) % (2 * np.pi) - np.pi) ** 2 + 0.1 * om * om + 0.001 * u * u)
    return crux.HostMDP(initialstate, gen, lambda sp: bool(abs(sp[1]) >= 4.0), lambda s: np.array([np.cos(s[0]), np.sin(s[0]), s[1] / 8.0], F), 3, 1, False,
                        n_envs=E, seed=seed, discount=0.99)


@pytest.mark.parametrize("where", ["device", "host"])
def test_steps_fills_every_block_where_the_ring_put_it(gpu_ctx, where):
    """crux.steps_ four times (reset = True, False, False, True; the third block wraps) with a Gaussian policy and a Gaussian nominal `pa`: after each call the block's
    rows, read in block order, hold the plain scans of their own :r / :episode_end / :done / V / ratios, with rows_per_env = Nsteps / n_envs and close_last = reset, and
    no other row of the ring changed. device: PendulumMDP through _fill_block; host: a HostMDP through crux_steps_push."""
    E, T, max_steps, cap, seed = 4, 40, 17, 400, 77; n = E * T
    mk = lambda s, st: crux.GaussianPolicy(parity.chain(E2E_DIMS, E2E_ACTS), E2E_LS, seed=s, stream=st, ctx=gpu_ctx)
    V = crux.ContinuousNetwork(parity.chain(E2E_DIMS, E2E_ACTS), seed=seed, stream=1, ctx=gpu_ctx)
    pi, pa = crux.ActorCritic(mk(seed, 0), V), mk(seed + 1, 2)
    mdp = crux.PendulumMDP(n_envs=E, seed=seed, discount=0.99) if where == "device" else _host_pendulum(E, seed)
    buf = crux.ExperienceBuffer(mdp.state_space(), mdp.action_space(), cap, E2E_EXTRAS, ctx=gpu_ctx)
    smp = crux.Sampler(mdp, crux.PolicyParams(pi, pa=pa), max_steps=max_steps, required_columns=E2E_EXTRAS, lam=0.95, ctx=gpu_ctx)
    p_pa = pa.get_params(); gamma, lam = F(0.99), F(0.95); i = 0; wrapped = open_rows = 0
    for call, reset in enumerate((True, False, False, True)):
        first = buf.next_ind - 1; rows = R.block_rows(first, n, cap); outside = np.setdiff1d(np.arange(cap), rows); wrapped += first + n > cap
        before = {k: _get(buf, k) for k in E2E_FILLED}
        crux.steps_(smp, buf, Nsteps=n, explore=True, i=i, reset=reset); i += n
        assert buf.next_ind - 1 == (first + n) % cap
        d = buf.minibatch(rows + 1); ee = d["episode_end"][0]; kw = {"seg": T, "close_last": int(reset)}; tag = "%s, call %d (first %d, reset %s): " % (where, call, first, reset)
        assert ee.sum() >= 2 * E and np.isfinite(d["logprob"]).all()
        open_rows += sum(z - a + 1 for a, z, closed in R.episodes(ee, **kw) if not closed)
        assert np.array_equal(_bits(d["return"][0]), _bits(R.returns_block(d["r"][0], ee, gamma, **kw))), tag + ":return"
        Vs, Vsp = V.forward(d["s"])[0], V.forward(d["sp"])[0]
        assert np.array_equal(_bits(d["advantage"][0]), _bits(R.gae_block(d["r"][0], d["done"][0], ee, Vs, Vsp, lam, gamma, **kw))), tag + ":advantage"
        ref = R.gaussian_iw(R.mlp(p_pa[:-1], E2E_DIMS, E2E_ACTS, d["s"]), p_pa[-1:], d["a"], d["logprob"][0])
        dev = float(np.abs(d["importance_weight"][0].astype(np.float64) - ref).max() / np.abs(ref).max())
        print(tag + ":importance_weight deviates %.3g of the column's maximum %.3g from float64" % (dev, np.abs(ref).max()))
        assert dev <= R.iw_tolerance("gaussian1"), tag + ":importance_weight %g" % dev
        for k, w in zip(("fwd_importance_weight", "cum_importance_weight", "rev_importance_weight"), R.weight_products_block(d["importance_weight"][0], ee, **kw)):
            assert np.array_equal(_bits(d[k][0]), _bits(w)), tag + ":" + k
        for k in E2E_FILLED:
            assert np.array_equal(_bits(_get(buf, k)[0, outside]), _bits(before[k][0, outside])), tag + "rows outside the block changed in :" + k
    assert wrapped == 1 and open_rows > 0                          # the third block wrapped; the reset = False blocks left episodes open
    if where == "host":
        assert buf["done"].any()
