"""16-bit integer IQ at the C ABI, on CPU: include/qrl_hip.h declares qrl_demod_process_sc16, qrl_demod_set_sc16_scale and
qrl_demod_process_sc16_host, libqrl_hip.so exports them, a NULL handle is QRL_ERR_ARG before any device work, and the Python binding
has their argtypes and the Demod methods."""
import ctypes as C
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1
HOST_ARGS = r"qrl_demod\s*\*\s*\w+\s*,\s*const\s+int16_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+"
DECLS = {
    "qrl_demod_process_sc16": r"qrl_demod\s*\*\s*\w+\s*,\s*const\s+int16_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+\s*,\s*const\s+qrl_demod_out\s*\*\s*\w+",
    "qrl_demod_set_sc16_scale": r"qrl_demod\s*\*\s*\w+\s*,\s*float\s+\w+",
    "qrl_demod_process_sc16_host": HOST_ARGS,
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrl_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_sc16_entry_point(name):
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLS[name]), _header()), "%s is not declared as the issue states it" % name


def test_header_comment_names_the_later_change():
    """a 1 Msps handle is refused, and the header says which kernels a later change has to widen"""
    text = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_demod_process_sc16\s*\(", text, flags=re.S)
    assert m, "no comment in front of qrl_demod_process_sc16"
    for word in ("k_resamp", "k_dec2_fir", "QRL_ERR_ARG", "32768"):
        assert word in m.group(1), word


@pytest.mark.parametrize("name", sorted(DECLS))
def test_library_exports_sc16_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    assert lib.qrl_demod_process_sc16(None, None, 0, 0, None) == QRL_ERR_ARG
    assert lib.qrl_demod_set_sc16_scale(None, 1.0) == QRL_ERR_ARG
    cnt = (C.c_uint32 * 4)()
    assert lib.qrl_demod_process_sc16_host(None, None, 0, 0, None, None, 0, cnt) == QRL_ERR_ARG


def test_python_binding_has_the_argtypes():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert list(lib.qrl_demod_process_sc16.argtypes) == [vp, vp, sz, sz, C.POINTER(q._Out)]
    assert list(lib.qrl_demod_set_sc16_scale.argtypes) == [vp, C.c_float]
    assert list(lib.qrl_demod_process_sc16_host.argtypes) == [vp, vp, sz, sz, vp, vp, sz, vp]
    for method in ("process_sc16", "process_sc16_async", "set_sc16_scale"):
        assert callable(getattr(q.Demod, method))
