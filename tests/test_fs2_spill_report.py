"""tools/fs2_spill_report.py on the kernels of -DCRUX_FS2_MINIMAL (the C2 / C5 learners: plain, PX, PXK, LAG, TIMING): what the compiler spills from the scalar file of
k_train_fs2 into VGPR lanes -- invisible in the scratch column of the resource tables. One compile of train_fs2.hip to device assembly (about half a minute,
no GPU), shared by the tests; skipped where hipcc is absent."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)), reason="hipcc is not installed")

# .sgpr_spill_count of the four plain bench kernels before the kernel arguments were read at their use (the same compile of the commit before that change)
BEFORE = {(4, 2, "categorical"): 157, (4, 1, "value"): 71, (17, 6, "gaussian"): 147, (17, 1, "value"): 79}


@pytest.fixture(scope="module")
def kernels():
    import fs2_spill_report
    ks = fs2_spill_report.report(all_forms=False)
    print(fs2_spill_report.table(ks))
    return ks


def _plain(kernels, i, o, kind):
    got = [k for k in kernels if k["template"]["form"] == "plain" and (k["template"]["in"], k["template"]["out"], k["template"]["kind"]) == (i, o, kind)]
    assert len(got) == 1, (i, o, kind, [k["label"] for k in kernels])
    return got[0]


def test_the_minimal_build_has_its_kernels_without_scratch_or_vgpr_spills(kernels):
    forms = sorted(k["template"]["form"] for k in kernels)
    assert len(kernels) == 18 and forms.count("plain") == 4 and forms.count("TIMING") == 4 and forms.count("PX") == 4 and forms.count("PXK") == 4 and forms.count("LAG") == 2, forms
    # (the plain, PX, PXK and TIMING forms of the four bench learners, and the two lagrange actors)
    for k in kernels:
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (k["label"], k["scratch"], k["vgpr_spill_count"])
        assert k["vgprs"] <= 256 and k["sgprs"] <= 106 and k["code_bytes"] > 0


@pytest.mark.parametrize("shape", sorted(BEFORE))
def test_the_plain_bench_kernels_spill_fewer_scalar_registers_than_before(kernels, shape):
    k = _plain(kernels, *shape)
    print(k["label"], "sgpr_spill_count", k["sgpr_spill_count"], "before", BEFORE[shape])
    assert k["sgpr_spill_count"] < BEFORE[shape]


@pytest.mark.parametrize("shape", [(4, 2, "categorical"), (4, 1, "value")])
def test_the_c2_minibatch_loops_hold_no_lane_spill_traffic(kernels, shape):
    k = _plain(kernels, *shape)
    assert len(k["minibatch_loops"]) == 2, k["minibatch_loops"]          # the helper role's and the compute role's
    for loop in k["minibatch_loops"]:
        print(k["label"], loop)
        assert loop["instructions"] > 500
        assert loop["v_readlane_b32"] == 0 and loop["v_writelane_b32"] == 0, (k["label"], loop)


def test_the_c5_loops_are_reported(kernels):
    for shape in ((17, 6, "gaussian"), (17, 1, "value")):
        k = _plain(kernels, *shape)
        assert len(k["minibatch_loops"]) == 2
        print(k["label"], k["minibatch_loops"])
