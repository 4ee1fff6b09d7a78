"""The C ABI of the wide-handle constructor and the ClipValue setter: include/cruxhip.h declares crux_mlp_create_wide with crux_mlp_create's parameter list and
crux_adam_set_clip_value / crux_adam_get_clip_value, and crux.jl_amd/_lib.py binds them with matching ctypes signatures. (The Julia shim does not bind them, as it does not
bind the conv entries they serve.) No GPU."""
import ctypes as C

import pytest

import test_julia_shim as TJ

NEW = ["crux_mlp_create_wide", "crux_adam_set_clip_value", "crux_adam_get_clip_value"]


@pytest.mark.parametrize("name", NEW)
def test_header_declares_the_entry(name):
    assert name in TJ.header_prototypes(), "%s is not declared in include/cruxhip.h" % name


def test_header_prototypes_are_the_intended_ones():
    protos = TJ.header_prototypes()
    assert protos["crux_mlp_create_wide"] == protos["crux_mlp_create"]
    assert protos["crux_adam_set_clip_value"] == (("int32_t", 0), [("crux_mlp", 1), ("float", 0)])
    assert protos["crux_adam_get_clip_value"] == (("float", 0), [("crux_mlp", 1)])


@pytest.mark.parametrize("name", NEW)
def test_python_binds_the_entry(name):
    from crux_jl_amd import _lib as L
    assert name in L.SIGNATURES, "%s is not in _lib.SIGNATURES" % name
    ret, args = L.SIGNATURES[name]
    assert len(args) == len(TJ.header_prototypes()[name][1])
    if name == "crux_mlp_create_wide":
        ret0, args0 = L.SIGNATURES["crux_mlp_create"]
        assert ret is ret0 and list(args) == list(args0)
    elif name == "crux_adam_set_clip_value":
        assert ret is C.c_int32 and list(args) == [C.c_void_p, C.c_float]
    else:
        assert ret is C.c_float and list(args) == [C.c_void_p]


def test_julia_shim_leaves_them_unbound_with_the_conv_entries():
    calls = {c[0] for c in TJ.shim_ccalls()}
    assert not any(n in calls for n in NEW) and not any(n.startswith("crux_conv_") for n in calls)
