"""The case lists of tests/learner_cases.py, checked without a GPU: the dispatch tables are the ones of the .hip files, the (bs, r) schedule covers every head at every edge, the
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


def _parse(fname, macros):
    """the uses of `macros` in a dispatcher, in file order, as table rows; #define lines are skipped, and \\b keeps MFXL_ / MFXM_ / MF8M_CASE out"""
    rows = []
    with open(os.path.join(CSRC, fname)) as f:
        for line in f:
            if line.lstrip().startswith("#"):
                continue
            for name, args in re.findall(r"\b(%s)\(([^()]*)\)" % "|".join(macros), line):
                a = [x.strip() for x in args.split(",")]
                assert len(a) == (6 if name == "FS2_CASE2" else 4), (fname, line)
                row = (int(a[0]), int(a[1]), KIND[a[2]], ACT[a[3]]) + ((int(a[4]), ACT[a[5]]) if name == "FS2_CASE2" else (64, ACT[a[3]]))
                rows.append(row)
    return rows


def test_the_dispatch_tables_are_the_ones_of_the_hip_files():
    fs2, mfx, mf8 = _parse("train_fs2.hip", ["FS2_CASE2", "FS2_CASE"]), _parse("train_mfma_x2.hip", ["MFX_CASE"]), _parse("train_mfma8.hip", ["MF8_CASE"])
    assert (len(fs2), len(mfx), len(mf8)) == (33, 10, 4)
    assert fs2 == LC.FS2_ROWS and mfx == LC.MFX_ROWS and mf8 == LC.MF8_ROWS
    for rows in (fs2, mfx, mf8):
        assert len(set(rows)) == len(rows)
    assert set(LC.MF8_ROWS) <= set(LC.MFX_ROWS) and sorted(LC.SMALL_ROWS) == sorted(LC.MFX_ROWS)


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
