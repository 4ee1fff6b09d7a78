"""Which learner a train! / batch_train! call gets (csrc/learner_route.h), asked without a GPU: tests/host/learner_route_check.cpp builds the argument blocks by hand, asks
learner_route and prints one line per case; the expectations are here. A dispatch slip that drops a bench learner onto the generic kernel changes no result -- only this
test (and the benchmark) sees it. One compile of about two seconds, shared by the tests; skipped where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

from crux_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not (os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)), reason="hipcc is not installed")

# name -> route, or (route, need_px, px_every), or a refusal's code
EXPECT = {
    # batch size, ids and shape edges
    "c2_bs128": "FS2", "c2_bs65": "FS2", "c2_bs64": "ONE8", "c5_bs64": "X2", "c2_bs129": "DENSE", "c2_bs128_len100": "ONE8", "c2_ids100": "ONE8", "c2_ids129": "GENERIC",
    "hopper_bs64": "DENSE", "hopper_ids64": "GENERIC", "hc32_bs128": "FS2", "hc32_bs128_fs0": "DENSE", "tiny_bs32": "GENERIC", "w256_bs256": "DENSE", "w256_ids": "GENERIC",
    "w512_ids": "DENSE",      # the generic learner's LDS carve would exceed 160 KB - 64
    # switches, learner_cus and placement
    "c2_bs128_fs0": "X2", "c2_cus1": "ONE8", "c2_cus2": "X2", "c5_bs64_x2off": "DENSE", "c2_force_generic": "GENERIC", "w512_force_generic": "DENSE",
    "c2_bs128_unplaced": "ONE8", "c5_bs128_unplaced": "DENSE", "tiny_bs128": "GENERIC", "tiny_ids": "GENERIC",
    # losses
    "c2_td_internal": "GENERIC", "c5_mse_action_bs128": "DENSE",
    # replica groups
    "group_c2_bs128": ("FS2", 1, 1), "group_c2_cus1": ("FS2", 1, 1), "group_c2_fs0": ("DENSE", 1, 1), "group_tiny": L.EUNSUP,
    "every4_c2_16mb": ("FS2", 1, 4), "every4_tiny": L.EUNSUP, "every4_c2_kl": L.EINVAL, "every4_c2_18mb": L.EINVAL,
    # lagrange, two-headed and regularised handles
    "lagrange_c2_bs128": "FS2", "lagrange_c2_fs0": "X2", "lagrange_acrobot": "DENSE", "lagrange_c2_group": ("DENSE", 1, 1),
    "two_headed_bs128": "DENSE", "two_headed_ids": "DENSE", "regularised_c2": "DENSE", "regularised_td_internal": L.EUNSUP,
}
MESSAGES = {"group_tiny": "would run un-synchronised", "every4_tiny": "the periodic exchange lives in the register-resident learner kernels",
            "every4_c2_kl": "no KL early stopping / max_batches", "every4_c2_18mb": "must divide the 18 minibatches", "regularised_td_internal": "DiagonalFisherRegularizer"}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "learner_route_check")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "crux.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "learner_route_check.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    got = {}
    for line in out.splitlines():
        head, _, msg = line.partition(" | ")
        f = head.rstrip(" |").split()
        if f[0] == "family":
            got["family"] = line[len("family "):]
        elif f[1] == "REFUSED":
            got[f[0]] = {"code": int(f[2]), "asked": int(f[5]), "msg": msg}
        else:
            got[f[0]] = {"route": f[1], "need_px": int(f[2]), "px_every": int(f[3]), "asked": int(f[4])}
    return got


def test_every_case_was_asked(lines):
    assert set(lines) == set(EXPECT) | {"family"}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_route(lines, name):
    want, got = EXPECT[name], lines[name]
    if isinstance(want, int):
        assert got.get("code") == want and MESSAGES[name] in got["msg"], got
    else:
        route, need_px, px_every = want if isinstance(want, tuple) else (want, 0, 1)
        assert (got.get("route"), got.get("need_px"), got.get("px_every")) == (route, need_px, px_every), got
    assert got["asked"] <= 1, got      # the placement probe: at most once per decision


def test_the_placement_probe_is_never_asked_for_a_network_outside_the_family(lines):
    for name in ("tiny_bs32", "tiny_bs128", "tiny_ids", "group_tiny", "every4_tiny", "w256_bs256", "c2_force_generic", "two_headed_bs128", "regularised_c2"):
        assert lines[name]["asked"] == 0, (name, lines[name])
    for name in ("c2_bs128", "c5_bs64", "c2_bs128_unplaced", "c5_bs128_unplaced"):      # ... and asked where a multi-CU form is about to be chosen
        assert lines[name]["asked"] == 1, (name, lines[name])


def test_the_fallback_warning_names_the_family_from_the_table(lines):
    assert lines["family"] == "IN-64-{64,32}-OUT with IN in {2,3,4,6,8,11,17,24,27}"
