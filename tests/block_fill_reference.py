"""Plain numpy restatement of what every steps! call leaves on the block it produced (src/sampler.jl:53-66,108-111,255-308): the yardstick of
tests/test_gpu_block_fills.py, checked on the CPU by tests/test_block_fill_reference.py. Nothing here shares code with csrc/advantage.hip, and nothing of the
library is imported.

Everything works in BLOCK order: block row k of a block of n rows pushed at ring row `first` of a ring of `cap` rows lives at physical row (first + k) % cap
(block_rows). seg = rows_per_env (seg <= 0: seg = n); segment e owns the block rows [e seg, min((e + 1) seg, n)). Inside a segment the episodes are the maximal
runs that end on an :episode_end row, the first one starting at the segment's first row; a trailing run without :episode_end is closed when close_last is set
(steps!(reset=true): terminate_episode! at the end of the block, sampler.jl:148) and is otherwise left with what mdp_data put into the fresh block
(experience_buffer.jl:4-35): 0 for :advantage / :return, 1 for the importance-weight products.

  gae_block              A = ((c A + r) + ((1 - done) gamma) Vsp) - Vs backwards from A = 0, c = Float32(lam) Float32(gamma): np.float32 scalars, sampler.jl:269
  returns_block          R = r + gamma R                                                                                            sampler.jl:278
  weight_products_block  (fwd, cum, rev): w = iw[k] w from w = 1, forwards / backwards; cum = the episode's last forward product      sampler.jl:283-308
  gaussian_iw            exp(sum_d(-(a - mu)^2 / (2 exp(ls)^2) - 0.9189385332046727 - ls) - logprob) in float64                      policies.jl:333-336
  gaussian_iw_f32        the same with np.float32 scalars in the kernel's association: used ONLY to size the tolerance of the float64 comparison
  categorical_iw         exp(log(sum(softmax(z) onehot)) - logprob) in float64                                                       policies.jl:128-135
  ignore_segments / always_close / physical_values
                         three deliberately WRONG scans (one segment where several are meant; every trailing run closed; V(s), V(sp) read at the physical
                         row): the CPU test shows that the inputs of every grid case tell each of them from the truth wherever the mistake can be made at all
  GRID / block_case / weight_case
                         the inputs of the GPU tests, from numpy alone, so that the CPU test sees the same rows
"""
import functools

import numpy as np

F = np.float32
LOG_SQRT_2PI = 0.9189385332046727


def block_rows(first, n, cap):
    """the physical ring rows of block rows 0 .. n-1"""
    return (int(first) + np.arange(int(n), dtype=np.int64)) % int(cap)


def episodes(ee, seg, close_last):
    """[(start, stop, closed)] in block order, stop inclusive: the runs of every segment; closed = the run ends on :episode_end, or trails and close_last is set"""
    ee = np.asarray(ee).reshape(-1).astype(bool); n = ee.size
    seg = int(seg) if int(seg) > 0 else n
    out = []
    for lo in range(0, n, seg):
        hi = min(lo + seg, n); start = lo
        for k in range(lo, hi):
            if ee[k]:
                out.append((start, k, True)); start = k + 1
        if start < hi:
            out.append((start, hi - 1, bool(close_last)))
    return out


def gae_block(r, done, ee, Vs, Vsp, lam, gamma, seg, close_last):
    r, Vs, Vsp = (np.asarray(x, F).reshape(-1) for x in (r, Vs, Vsp)); done = np.asarray(done).reshape(-1).astype(bool)
    lam, gamma = F(lam), F(gamma); c = F(lam * gamma); one = F(1)
    adv = np.zeros(r.size, F)
    for a, b, closed in episodes(ee, seg, close_last):
        if not closed:
            continue                                    # the fresh block's zeros
        A = F(0)
        for k in range(b, a - 1, -1):
            t2 = F(F(c * A) + r[k])
            t3 = F(F(F(one - (one if done[k] else F(0))) * gamma) * Vsp[k])
            A = F(F(t2 + t3) - Vs[k]); adv[k] = A
    return adv


def returns_block(r, ee, gamma, seg, close_last):
    r = np.asarray(r, F).reshape(-1); gamma = F(gamma)
    ret = np.zeros(r.size, F)
    for a, b, closed in episodes(ee, seg, close_last):
        if not closed:
            continue
        R = F(0)
        for k in range(b, a - 1, -1):
            R = F(r[k] + F(gamma * R)); ret[k] = R
    return ret


def weight_products_block(iw, ee, seg, close_last):
    iw = np.asarray(iw, F).reshape(-1)
    fwd, cum, rev = (np.ones(iw.size, F) for _ in range(3))
    for a, b, closed in episodes(ee, seg, close_last):
        if not closed:
            continue                                    # the fresh block's ones
        w = F(1)
        for k in range(a, b + 1):
            w = F(iw[k] * w); fwd[k] = w
        cum[a:b + 1] = w
        w = F(1)
        for k in range(b, a - 1, -1):
            w = F(iw[k] * w); rev[k] = w
    return fwd, cum, rev


# ---- the per-step ratio -------------------------------------------------------------------------------------------------------------------------------------------
def gaussian_iw(mu, log_sigma, a, logprob):
    """mu, a: [act_dim x n]; log_sigma: [act_dim]; logprob: [n]. float64 throughout."""
    mu, a = np.asarray(mu, np.float64), np.asarray(a, np.float64); ls = np.asarray(log_sigma, np.float64).reshape(-1, 1)
    nom = (-(a - mu) ** 2 / (2.0 * np.exp(ls) ** 2) - LOG_SQRT_2PI - ls).sum(axis=0)
    return np.exp(nom - np.asarray(logprob, np.float64).reshape(-1))


def gaussian_iw_f32(mu, log_sigma, a, logprob):
    """np.float32 scalars, one operation at a time, summed over the action dimensions in order: how a Float32 implementation associates the same formula"""
    mu, a = np.asarray(mu, F), np.asarray(a, F); ls = np.asarray(log_sigma, F).reshape(-1); lp = np.asarray(logprob, F).reshape(-1)
    out = np.empty(lp.size, F)
    for j in range(lp.size):
        nom = F(0)
        for d in range(ls.size):
            sg = F(np.exp(ls[d])); s2 = F(sg * sg); df = F(a[d, j] - mu[d, j])
            nom = F(nom + F(F(F(-F(df * df)) / F(F(2) * s2) - F(LOG_SQRT_2PI)) - ls[d]))
        out[j] = F(np.exp(F(nom - lp[j])))
    return out


def categorical_iw(z, onehot, logprob):
    """z: logits [n_actions x n]; onehot: [n_actions x n]; logprob: [n]. float64 throughout."""
    z = np.asarray(z, np.float64); e = np.exp(z - z.max(axis=0, keepdims=True)); p = e / e.sum(axis=0, keepdims=True)
    return np.exp(np.log((p * np.asarray(onehot, np.float64)).sum(axis=0)) - np.asarray(logprob, np.float64).reshape(-1))


# ---- a dense chain from its flat parameter vector (W1 column-major [out x in], b1, W2, b2, ..., extras) ----------------------------------------------------------------
_ACT = {"identity": lambda x: x, "relu": lambda x: np.maximum(x, 0), "tanh": np.tanh}


def init_params(dims, rng, n_extra=0):
    """Glorot-uniform weights and small biases in the flat order, n_extra trailing zeros"""
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o)); out += [rng.uniform(-lim, lim, i * o), rng.normal(0, 0.2, o)]
    return np.concatenate(out + [np.zeros(n_extra)]).astype(F)


def mlp(params, dims, acts, x, dtype=np.float64):
    """x: [dims[0] x n] -> [dims[-1] x n], every operation in `dtype`"""
    h = np.asarray(x, dtype); off = 0; p = np.asarray(params)
    for i, o, act in zip(dims[:-1], dims[1:], acts):
        W = p[off:off + i * o].reshape((o, i), order="F").astype(dtype); off += i * o
        b = p[off:off + o].astype(dtype); off += o
        h = _ACT[act]((W @ h + b[:, None]).astype(dtype))
    return h


# ---- the three wrong scans ------------------------------------------------------------------------------------------------------------------------------------------
def ignore_segments(scan, *cols, seg, close_last, **kw):
    """`scan` (gae_block / returns_block / weight_products_block) as a kernel that forgot the environments: one segment, episodes run across the boundaries"""
    return scan(*cols, seg=0, close_last=close_last, **kw)


def always_close(scan, *cols, seg, close_last, **kw):
    """`scan` as a kernel that closes every trailing run whatever close_last says"""
    return scan(*cols, seg=seg, close_last=1, **kw)


def physical_values(r, done, ee, Vs, Vsp, lam, gamma, seg, close_last, first, cap):
    """gae_block as a kernel that reads V(s), V(sp) at the PHYSICAL row of block row k (the value arrays have n entries: the index is taken mod n)"""
    n = np.asarray(r).size; q = block_rows(first, n, cap) % n
    return gae_block(r, done, ee, np.asarray(Vs, F).reshape(-1)[q], np.asarray(Vsp, F).reshape(-1)[q], lam, gamma, seg, close_last)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------------------------------
LAM, GAMMA = 0.95, 0.99
OBS_DIM = 4
ACTS = ["tanh", "tanh", "identity"]
# id: (E, T, cap, first, rows_per_env given to the entry point (0: one segment), hidden width of the critics)
GRID = {
    1: (3, 130, 500, 0, 130, 32),
    2: (3, 130, 500, 110, 130, 32),       # the block ends exactly at cap
    3: (3, 130, 500, 111, 130, 32),       # wraps by one row
    4: (3, 130, 500, 370, 130, 32),       # wraps where the second segment begins
    5: (3, 130, 500, 499, 130, 32),       # one row before the wrap
    6: (3, 130, 390, 200, 130, 32),       # n == capacity
    7: (3, 130, 500, 370, 0, 32),         # rows_per_env = 0: the whole block is one segment
    8: (4, 550, 2400, 1300, 550, 64),     # 2200 rows, 1100 before the wrap and 1100 after: value ranges of >= 1024 rows, a 4-64-64-1 critic
}
WEIGHT_CASES = (3, 4, 7)


@functools.lru_cache(maxsize=None)
def block_case(cid):
    """The rows of grid case `cid` in block order, the junk that lies in the ring around them, and the two critics' parameters.

    :episode_end is random at about 4 % (never on a segment's last row), plus: physical rows cap-1 and 0 where the block holds them; one segment with none at all
    (`empty_segment`: the first one free of those two rows); of the other segments (in order) the first gets one on its LAST row and the next one on its FIRST
    row (a one-row episode). Case 7 (rows_per_env = 0) is ONE segment: see below. :done is set on about half of the :episode_end rows (the others are time-limit cuts) and on no other row."""
    E, T, cap, first, rpe, hidden = GRID[cid]
    n = E * T; rng = np.random.default_rng(1000 + cid)
    ee = rng.random(n) < 0.04
    ee[T - 1::T] = False
    k_wrap = [k for k in ((cap - 1 - first) % cap, (cap - first) % cap) if k < n]      # the block rows at physical rows cap-1 and 0
    for k in k_wrap:
        ee[k] = True
    if rpe > 0:
        empty = next(e for e in range(E) if not any(e * T <= k < (e + 1) * T for k in k_wrap))
        ee[empty * T:(empty + 1) * T] = False
        others = [e for e in range(E) if e != empty]
        ee[others[0] * T + T - 1] = True; ee[others[1] * T] = True
    else:               # one segment of n rows: a one-row episode on its first row, its last row open (close_last decides), no run ends where a T-row split would cut
        empty = None; ee[0] = True
    done = ee & (rng.random(n) < 0.5)
    dims = [OBS_DIM, hidden, hidden, 1]
    c = {"id": cid, "E": E, "T": T, "n": n, "cap": cap, "first": first, "rows_per_env": rpe, "seg": rpe if rpe > 0 else n, "dims": dims, "acts": ACTS,
         "empty_segment": empty, "k_wrap": k_wrap,
         "s": rng.normal(0, 1, (OBS_DIM, n)).astype(F), "sp": rng.normal(0, 1, (OBS_DIM, n)).astype(F), "a": rng.uniform(-1, 1, (1, n)).astype(F),
         "r": rng.normal(0, 1, n).astype(F), "cost": rng.uniform(0, 2, n).astype(F), "done": done, "episode_end": ee,
         "importance_weight": rng.uniform(0.7, 1.4, n).astype(F),
         "pV": init_params(dims, rng), "pVc": init_params(dims, rng)}
    # what lies in the ring outside the block: rows of the same kind (a scan that leaves the block reads episode ends and rewards, not zeros)
    c["junk"] = {"s": rng.normal(0, 1, (OBS_DIM, cap)).astype(F), "sp": rng.normal(0, 1, (OBS_DIM, cap)).astype(F), "a": rng.uniform(-1, 1, (1, cap)).astype(F),
                 "r": rng.normal(0, 1, cap).astype(F), "cost": rng.uniform(0, 2, cap).astype(F), "done": rng.random(cap) < 0.05, "episode_end": rng.random(cap) < 0.1,
                 "importance_weight": rng.uniform(0.7, 1.4, cap).astype(F)}
    for v in list(c.values()) + list(c["junk"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def ring_columns(c):
    """({key: the physical column over rows 0 .. length(b)-1}, length(b)) of the ring once the GPU test has filled it: junk everywhere, the block at block_rows"""
    rows = block_rows(c["first"], c["n"], c["cap"]); m = min(c["cap"], c["first"] + c["n"]); out = {}
    for k, junk in c["junk"].items():
        col = junk.copy(); col[..., rows] = c[k]; out[k] = col[..., :m]
    return out, m


def nan_row(c):
    """a block row that lies past the wrap and inside an episode that ends on :episode_end (closed whatever close_last): a NaN reward there must reach the advantage"""
    k_first_wrapped = c["cap"] - c["first"]
    return next(k for a, b, closed in episodes(c["episode_end"], c["rows_per_env"], 0) if closed for k in range(a, b + 1) if k >= k_first_wrapped)


def outside_row(c):
    """a physical ring row right behind the block"""
    assert c["n"] < c["cap"]
    return (c["first"] + c["n"]) % c["cap"]


def case_values(c, which="pV", dtype=F):
    """V(s), V(sp) of a case's block from numpy (the CPU test; the GPU test takes them from the library's own forward)"""
    return mlp(c[which], c["dims"], c["acts"], c["s"], dtype)[0].astype(F), mlp(c[which], c["dims"], c["acts"], c["sp"], dtype)[0].astype(F)


# the per-step ratio: (name, act_dim or number of actions, discrete)
IW_HEADS = {"gaussian1": (1, False), "gaussian3": (3, False), "categorical3": (3, True)}
IW_CAP, IW_FIRST, IW_ROWS = 700, 37, 300          # rows [37, 337): first_row is not 0 and the range crosses a 256-thread block
IW_DIMS, IW_ACTS = [OBS_DIM, 32, 32], ["tanh", "tanh", "identity"]
LOG_SIGMA = np.array([-0.4, 0.1, -1.0], F)


@functools.lru_cache(maxsize=None)
def weight_case(name):
    """A full ring of IW_CAP rows for crux_importance_weight_rows: the nominal policy's parameters, states, actions and a :logprob column chosen so that
    |logpdf(pa, s, a) - logprob| <= 2.9 on every row (the ratios lie in [0.055, 18.2]: nothing under- or overflows)."""
    ad, disc = IW_HEADS[name]; rng = np.random.default_rng(2000 + ad + 10 * disc)
    dims = IW_DIMS + [ad]; n = IW_CAP
    p = init_params(dims, rng, n_extra=0 if disc else ad)
    s = rng.normal(0, 1, (OBS_DIM, n)).astype(F)
    z = mlp(p, dims, IW_ACTS, s)                                       # float64
    if disc:
        a = np.eye(ad, dtype=bool)[:, rng.integers(0, ad, n)]
        nom = np.log(categorical_iw(z, a, np.zeros(n))); ls = None
    else:
        ls = LOG_SIGMA[:ad].copy(); p[-ad:] = ls
        a = (z + np.exp(ls.astype(np.float64))[:, None] * rng.normal(0, 1, (ad, n))).astype(F)
        nom = np.log(gaussian_iw(z, ls, a, np.zeros(n)))
    lp = (nom - rng.uniform(-2.9, 2.9, n)).astype(F)
    c = {"name": name, "ad": ad, "disc": disc, "dims": dims, "acts": IW_ACTS, "p": p, "log_sigma": ls, "s": s, "a": a, "logprob": lp, "z64": z, "nominal_logpdf": nom}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def iw_reference(c):
    """float64 ratios of every row of a weight_case"""
    return categorical_iw(c["z64"], c["a"], c["logprob"]) if c["disc"] else gaussian_iw(c["z64"], c["log_sigma"], c["a"], c["logprob"])


def iw_f32_deviation(c):
    """max |Float32 replica - float64| / max |float64| of a Gaussian weight_case (mu from a Float32 forward): the rounding a Float32 implementation cannot avoid"""
    mu32 = mlp(c["p"], c["dims"], c["acts"], c["s"], F)
    ref = iw_reference(c)
    return float(np.abs(gaussian_iw_f32(mu32, c["log_sigma"], c["a"], c["logprob"]).astype(np.float64) - ref).max() / np.abs(ref).max())


IW_FLOOR = 5e-6                                   # the project's bound for the categorical head (tests/test_gpu_round4.py), of the column's maximum
IW_MEASURED = {"gaussian1": 1.0e-6, "gaussian3": 1.1e-6}      # iw_f32_deviation of the two Gaussian cases, rounded up (measured 9.9e-7 and 1.05e-6; test_block_fill_reference.py holds them to it)


def iw_tolerance(name):
    """of the column's maximum: the larger of IW_FLOOR and four times the Float32 replica's own deviation (the factor covers expf / logf of the device against the
    host's). 4 x 1.1e-6 = 4.4e-6 < 5e-6: the floor is the bound for every head."""
    return max(IW_FLOOR, 4.0 * IW_MEASURED.get(name, 0.0))
