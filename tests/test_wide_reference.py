"""CPU: the wide grid (tests/wide_cases.py) through dense_reference.chain_reference in the engine's defined summation order (gemm16_order_f32 / rowsum16_order_f32).
Every tensor's emulated ratio to max(e32, u) must stay at or below dense_reference.M_EMULATED_WORST, the figure the existing margin M_MARGIN = 2 x 5.55 was derived from, so
that tests/test_gpu_wide.py can use M_MARGIN unchanged: reductions up to 4096 long do not ask for a wider bound. The kink-free draw must end within its 32 rounds on
every relu member. No GPU, no library."""
import numpy as np
import pytest

import dense_reference as R
from wide_cases import WIDE_CASES


def test_grid_reaches_every_place_wide_can_break():
    dims = [c[0] for c in WIDE_CASES]
    assert all(max(d) > 1024 for d in dims) and max(max(d) for d in dims) == 4096
    assert any(d[0] % 4 for d in dims) and any(d[0] > 1024 and d[1] > 1024 for d in dims if len(d) > 2)                  # K no multiple of 4; both dimensions wide
    assert any(d[0] <= 1024 and d[1] > 1024 for d in dims) and any(d[0] > 1024 and d[1] <= 1024 for d in dims)          # wide as M and as K
    tiles = lambda d: ((d[1] + 15) // 16) * ((d[0] + 15) // 16)      # noqa: E731  (dW of layer 0: M = out, N = in)
    assert sum(1 for d in dims if tiles(d) > 4096) >= 2
    assert ([2048, 256, 6], ["relu", "identity"], 32) in WIDE_CASES and ([3136, 512, 6], ["relu", "identity"], 16) in WIDE_CASES


@pytest.mark.parametrize("case", WIDE_CASES, ids=R.case_id)
def test_emulated_engine_order_stays_inside_the_measured_worst(case):
    dims, acts, B = case
    rng = np.random.default_rng(3)
    p = R.perturbed_params(R.glorot_params(dims, rng), rng); st = {"rounds": 0}
    x = R.kink_free_inputs(p, dims, acts, B, rng, stats=st) if "relu" in acts else np.asfortranarray(rng.normal(0, 1, (dims[0], B)).astype(np.float32))
    assert st["rounds"] <= 32
    dy = rng.normal(0, 1, (dims[-1], B)).astype(np.float32)
    r64 = R.chain_reference(p, dims, acts, x, dy, np.float64); r32 = R.chain_reference(p, dims, acts, x, dy, np.float32)
    rem = R.chain_reference(p, dims, acts, x, dy, np.float32, mm=R.gemm16_order_f32, rowsum=R.rowsum16_order_f32)
    for name, get in [("y", lambda r: r["y"]), ("dx", lambda r: r["dx"])] + [("dW%d" % l, lambda r, l=l: r["dW"][l]) for l in range(len(acts))] + [("db%d" % l, lambda r, l=l: r["db"][l]) for l in range(len(acts))]:
        e32, eem = R.rel_err(get(r32), get(r64)), R.rel_err(get(rem), get(r64))
        ratio = eem / max(e32, R.U32)
        print("%-24s %-4s e32 %7.2f u  emulated %7.2f u  ratio %.2f" % (R.case_id(case), name, e32 / R.U32, eem / R.U32, ratio))
        assert ratio <= R.M_EMULATED_WORST, (name, e32 / R.U32, eem / R.U32)
