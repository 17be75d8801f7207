"""int8 IQ (sc8) output of the transmitters at the C ABI, on CPU: include/qrl_hip.h declares the nine entry points (process_sc8,
set_sc8_scale, set_sc8_clip_counts for qrl_mod, qrl_amod and qrl_synth), libqrl_hip.so exports them, a NULL handle is QRL_ERR_ARG before any
device work, and the Python binding has their argtypes and the Mod / AMod / Synth methods."""
import ctypes as C
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1


def _args(*parts):
    return r"\s*,\s*".join(parts)


def _ptr(t, const=False):
    return (r"const\s+" if const else "") + t + r"\s*\*\s*\w+"


SZ = r"size_t\s+\w+"
DECLS = {
    "qrl_mod_process_sc8": _args(_ptr("qrl_mod"), _ptr("uint8_t", True), SZ, SZ, _ptr("int8_t"), SZ),
    "qrl_amod_process_sc8": _args(_ptr("qrl_amod"), _ptr("float", True), SZ, SZ, _ptr("int8_t"), SZ),
    "qrl_synth_process_sc8": _args(_ptr("qrl_synth"), _ptr("int16_t", True), SZ, SZ, _ptr("int8_t"), SZ, _ptr("size_t")),
}
for _x in ("mod", "amod", "synth"):
    DECLS["qrl_%s_set_sc8_scale" % _x] = _args(_ptr("qrl_" + _x), r"float\s+\w+")
    DECLS["qrl_%s_set_sc8_clip_counts" % _x] = _args(_ptr("qrl_" + _x), _ptr("uint32_t"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrl_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_sc8_tx_entry_point(name):
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLS[name]), _header()), "%s is not declared as the issue states it" % name


def test_header_comment_states_the_contract():
    """the rule, the default, the alignment, the word-sharing rule, the counters"""
    text = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_mod_process_sc8\s*\(", text, flags=re.S)
    assert m, "no comment in front of qrl_mod_process_sc8"
    for word in ("rintf(x * scale)", "[-128, 127]", "127.0f", "NaN", "2-byte aligned", "QRL_ERR_ARG", "4-byte word", "qrl_mod_set_sc8_clip_counts", "-128 reached"):
        assert word in m.group(1), word


@pytest.mark.parametrize("name", sorted(DECLS))
def test_library_exports_sc8_tx_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    produced = C.c_size_t(7)
    assert lib.qrl_mod_process_sc8(None, None, 0, 0, None, 0) == QRL_ERR_ARG
    assert lib.qrl_amod_process_sc8(None, None, 0, 0, None, 0) == QRL_ERR_ARG
    assert lib.qrl_synth_process_sc8(None, None, 0, 0, None, 0, C.byref(produced)) == QRL_ERR_ARG
    for x in ("mod", "amod", "synth"):
        assert getattr(lib, "qrl_%s_set_sc8_scale" % x)(None, 1.0) == QRL_ERR_ARG
        assert getattr(lib, "qrl_%s_set_sc8_clip_counts" % x)(None, None) == QRL_ERR_ARG


def test_python_binding_has_the_argtypes_and_methods():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert list(lib.qrl_mod_process_sc8.argtypes) == [vp, vp, sz, sz, vp, sz]
    assert list(lib.qrl_amod_process_sc8.argtypes) == [vp, vp, sz, sz, vp, sz]
    assert list(lib.qrl_synth_process_sc8.argtypes) == [vp, vp, sz, sz, vp, sz, C.POINTER(sz)]
    for x in ("mod", "amod", "synth"):
        assert list(getattr(lib, "qrl_%s_set_sc8_scale" % x).argtypes) == [vp, C.c_float]
        assert list(getattr(lib, "qrl_%s_set_sc8_clip_counts" % x).argtypes) == [vp, vp]
    for cls, methods in ((q.Mod, ("process_sc8", "process_sc8_async")), (q.AMod, ("process_sc8",)), (q.Synth, ("process_sc8",))):
        for method in methods + ("set_sc8_scale", "set_sc8_clip_counts"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
