"""The C ABI of CQL's entries for a two-headed actor: include/cruxhip.h declares crux_cql_{critic_step, alpha_step, conservative}_sigma with the parameter lists of their plain
twins, crux.jl_amd/_lib.py binds them with the twins' ctypes signatures, and julia/CruxHIP.jl calls them. No GPU."""
import pytest

import test_julia_shim as TJ

NAMES = ["crux_cql_critic_step", "crux_cql_alpha_step", "crux_cql_conservative"]


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_sigma_entry_with_its_twins_parameters(name):
    protos = TJ.header_prototypes()
    assert name + "_sigma" in protos, "%s_sigma is not declared in include/cruxhip.h" % name
    assert protos[name + "_sigma"] == protos[name]


@pytest.mark.parametrize("name", NAMES)
def test_python_binds_the_sigma_entry(name):
    from crux_jl_amd import _lib as L
    assert name + "_sigma" in L.SIGNATURES, "%s_sigma is not in _lib.SIGNATURES" % name
    ret, args = L.SIGNATURES[name + "_sigma"]; ret0, args0 = L.SIGNATURES[name]
    assert ret is ret0 and list(args) == list(args0) and len(args) == len(TJ.header_prototypes()[name][1])


@pytest.mark.parametrize("name", NAMES)
def test_julia_shim_calls_the_sigma_entry(name):
    calls = {c[0]: c for c in TJ.shim_ccalls()}
    assert name + "_sigma" in calls, "julia/CruxHIP.jl has no ccall of %s_sigma" % name
    assert calls[name + "_sigma"][1:3] == calls[name][1:3] and len(calls[name + "_sigma"][3]) == len(calls[name][3])
