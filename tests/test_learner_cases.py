"""The case lists of tests/learner_cases.py, checked without a GPU: the dispatch tables are the flags of csrc/learner_shapes.h, the (bs, r) schedule covers every head at every edge, the
gradients of every case are live (the surrogate is not clipped away) and every case is sensitive to ONE dropped row by five times the bound the GPU module asserts on Adam's m.
Nothing here runs a kernel: the reference alone."""
import os
import re

import numpy as np
import pytest

import learner_cases as LC
from crux_jl_amd import _lib as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "crux.jl_amd", "csrc")
KIND = {"MFK_CATEGORICAL": LC.CAT, "MFK_GAUSSIAN": LC.GAU, "MFK_VALUE": LC.VAL}
ACT = {"CRUX_ACT_RELU": LC.RELU, "CRUX_ACT_TANH": LC.TANH, "CRUX_ACT_IDENTITY": LC.IDENT}


def _parse():
    """the rows of CRUX_LEARNER_SHAPES in csrc/learner_shapes.h, in file order: [(row, {flag names})]"""
    rows = []
    with open(os.path.join(CSRC, "learner_shapes.h")) as f:
        for line in f:
            m = re.match(r"\s*X\(([^()]*)\)", line)
            if not m:
                continue
            a = [x.strip() for x in m.group(1).split(",")]
            assert len(a) == 7, line
            flags = {x.strip() for x in a[6].split("|")}
            assert all(re.fullmatch(r"LF_[A-Z0-9_]+", x) for x in flags), line
            rows.append(((int(a[0]), int(a[1]), KIND[a[2]], ACT[a[3]], int(a[4]), ACT[a[5]]), flags))
    return rows


def _with(table, flag):
    return [row for row, flags in table if flag in flags]


# the lists the flags replace, written out from the dispatchers they stood in (train_fs2.hip: FS2_HAS_LAG and HAS_TIMING, the CRUX_FS2_MINIMAL rows; train_mfma_x2.hip:
# MFXL_CASE, MFXM_CASE and the timing pair; train_mfma8.hip: MF8M_CASE and the timing shape)
_C2A, _C2C, _C5A, _C5C = LC._r(4, 2, LC.CAT, LC.RELU), LC._r(4, 1, LC.VAL, LC.RELU), LC._r(17, 6, LC.GAU, LC.TANH), LC._r(17, 1, LC.VAL, LC.TANH)
_LAG = [_C2A, LC._r(8, 4, LC.CAT, LC.RELU), LC._r(3, 1, LC.GAU, LC.RELU), _C5A]
SUBSETS = {"LF_FS2_MIN": [_C2A, _C2C, _C5A, _C5C], "LF_FS2_LAG": _LAG, "LF_FS2_TIMING": [_C2A, _C2C, _C5A, _C5C],
           "LF_X2_LAG": _LAG, "LF_X2_MULTI": [_C2A, _C2C, _C5A, _C5C], "LF_X2_TIMING": [_C2A, _C5A],
           "LF_ONE8_MULTI": [_C2A, _C2C, LC._r(3, 1, LC.GAU, LC.RELU), LC._r(3, 1, LC.VAL, LC.RELU)], "LF_ONE8_TIMING": [_C2A]}


def test_the_dispatch_tables_are_the_ones_of_the_shape_table():
    table = _parse()
    fs2, mfx, mf8 = _with(table, "LF_FS2"), _with(table, "LF_X2"), _with(table, "LF_ONE8")
    assert (len(fs2), len(mfx), len(mf8)) == (33, 10, 4)
    assert len(table) == 33 and fs2 == LC.FS2_ROWS      # every row is a k_train_fs2 row, in the order the (bs, r) schedule counts in
    assert set(mfx) == set(LC.MFX_ROWS) and set(mf8) == set(LC.MF8_ROWS)      # (their dispatchers match disjoint rows: no order to keep)
    for rows in (fs2, mfx, mf8, LC.MFX_ROWS, LC.MF8_ROWS):
        assert len(set(rows)) == len(rows)
    assert set(LC.MF8_ROWS) <= set(LC.MFX_ROWS) and sorted(LC.SMALL_ROWS) == sorted(LC.MFX_ROWS)


@pytest.mark.parametrize("flag", sorted(SUBSETS))
def test_the_flag_subsets_are_the_lists_they_replace(flag):
    table = _parse()
    assert {f for _, flags in table for f in flags} == set(SUBSETS) | {"LF_FS2", "LF_X2", "LF_ONE8"}
    got = _with(table, flag)
    assert len(got) == len(set(got)) and set(got) == set(SUBSETS[flag]), (flag, got)


def test_the_edge_schedule_covers_every_head_at_every_pair():
    assert len(LC.FS2_EDGES) == len(set(LC.FS2_EDGES)) == 12
    for bs, r in LC.FS2_EDGES:
        assert 65 <= bs <= 128 and 1 <= r < bs
    assert {r for _, r in LC.FS2_EDGES} >= {1, 15, 16, 17, 32, 33} and {bs for bs, _ in LC.FS2_EDGES} >= {65, 127, 128}
    met = {p: set() for p in LC.FS2_EDGES}
    for i, row, bs, r in LC.fs2_cases():
        met[(bs, r)].add(row[2])
    assert len(LC.fs2_cases()) == 99 + 12 and len(set(LC.fs2_cases())) == 111
    for i in range(len(LC.FS2_ROWS)):
        assert LC.fs2_pairs(i)[:3] == [LC.FS2_EDGES[(3 * i + j) % 12] for j in range(3)]      # the rule itself stays; FS2_EXTRA_PAIRS only adds
    for p, kinds in met.items():
        assert kinds == {LC.CAT, LC.GAU, LC.VAL}, (p, kinds)


FS2_IDS = ["%02d_%s" % (i, LC.row_id(row)) for i, row in enumerate(LC.FS2_ROWS)]


@pytest.mark.parametrize("i", range(len(LC.FS2_ROWS)), ids=FS2_IDS)
def test_fs2_cases_are_live_and_feel_one_dropped_row(i):
    """Liveness: the oracle's own five-epoch trajectory has finite infos and, for the policy heads, a mean clip_fraction in [0.02, 0.6] (with logprob ~ N(-1.2, 0.05) the
    Gaussian rows of 4..8 actions sit at 1.00). Sensitivity: one row removed from the ragged minibatch of the first window (from minibatch 1 where the ragged one has a single
    row) moves Adam's m at the window's end by at least M_SHIFT_MIN = 5e-5 -- a kernel that drops or mis-weights a single row cannot stay inside the 1e-5 the GPU module allows."""
    row = LC.FS2_ROWS[i]
    for bs, r in LC.fs2_pairs(i):
        case = LC.make_case(row, bs, r, LC.case_seed(i, bs, r)); nmb = 4
        assert case.N == 3 * bs + r and -(-case.N // bs) == nmb
        infos, ms = LC.oracle_run(case, bs)
        assert infos.shape == (5 * nmb, L.INFO_N) and np.isfinite(infos).all()
        cf = float(infos[:, L.INFO["clip_fraction"]].mean()); gn = float(infos[:, L.INFO["grad_norm"]].min())
        if row[2] != LC.VAL:
            assert 0.02 <= cf <= 0.6, (row, bs, r, cf)
        _, ms2 = LC.oracle_run(case, bs, drop=(2, 1 if r == 1 else nmb - 1), epochs=3)
        shift = float(np.abs(ms2[2] - ms[2]).max())
        print("CASE %s bs %d r %d: clip %.3f min |g| %.3g m shift %.3g" % (LC.row_id(row), bs, r, cf, gn, shift))
        assert shift >= LC.M_SHIFT_MIN, (row, bs, r, shift)


def test_logprob_is_the_networks_own_density():
    """the float64 density of make_case against the oracle's float32 head: at the initial parameters every ratio is exp(-noise), so kl and clip_fraction of the first step are
    those of the noise alone (|noise| > log 1.2 = 0.18 for about 7 % of N(0, 0.1) draws)"""
    for row in (LC.FS2_ROWS[0], LC.FS2_ROWS[2], LC.FS2_ROWS[27]):
        case = LC.make_case(row, 128, 97, 3)
        infos, _ = LC.oracle_run(case, 128, epochs=1, at=())
        assert 0.01 < infos[0, L.INFO["clip_fraction"]] < 0.2, (row, infos[0])
        assert abs(infos[0, L.INFO["kl"]]) < 0.03, (row, infos[0])
