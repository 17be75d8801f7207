"""8-bit IQ (sc8, cu8) at the C ABI, on CPU: include/qrl_hip.h declares the ten entry points, libqrl_hip.so exports them, a NULL handle is
QRL_ERR_ARG before any device work, and the Python binding has their argtypes and the Demod / Fft methods."""
import ctypes as C
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1


def _process(handle, ctype):
    return r"%s\s*\*\s*\w+\s*,\s*const\s+%s\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+" % (handle, ctype)


def _host(ctype):
    return _process("qrl_demod", ctype) + r"\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+"


OUT = r"\s*,\s*const\s+qrl_demod_out\s*\*\s*\w+"
DECLS = {
    "qrl_demod_process_sc8": _process("qrl_demod", "int8_t") + OUT,
    "qrl_demod_process_cu8": _process("qrl_demod", "uint8_t") + OUT,
    "qrl_demod_process_sc8_host": _host("int8_t"),
    "qrl_demod_process_cu8_host": _host("uint8_t"),
    "qrl_demod_set_sc8_scale": r"qrl_demod\s*\*\s*\w+\s*,\s*float\s+\w+",
    "qrl_demod_set_cu8_scale": r"qrl_demod\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*float\s+\w+",
    "qrl_fft_process_sc8": _process("qrl_fft", "int8_t"),
    "qrl_fft_process_cu8": _process("qrl_fft", "uint8_t"),
    "qrl_fft_set_sc8_scale": r"qrl_fft\s*\*\s*\w+\s*,\s*float\s+\w+",
    "qrl_fft_set_cu8_scale": r"qrl_fft\s*\*\s*\w+\s*,\s*float\s+\w+\s*,\s*float\s+\w+",
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrl_hip.h")).read(), flags=re.S)


def test_there_are_ten_new_entry_points():
    assert len(DECLS) == 10


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_iq8_entry_point(name):
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLS[name]), _header()), "%s is not declared as the issue states it" % name


def test_header_comment_states_the_contract():
    text = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_demod_process_sc8\s*\(", text, flags=re.S)
    assert m, "no comment in front of qrl_demod_process_sc8"
    for word in ("127.5", "1.0f / 128", "QRL_ERR_ARG", "multiple of 8 samples", "1 Msps", "QRL_OPT_SC16_BASEBAND"):
        assert word in m.group(1), word


@pytest.mark.parametrize("name", sorted(DECLS))
def test_library_exports_iq8_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    cnt = (C.c_uint32 * 4)()
    for fmt in ("sc8", "cu8"):
        assert getattr(lib, "qrl_demod_process_" + fmt)(None, None, 0, 0, None) == QRL_ERR_ARG
        assert getattr(lib, "qrl_demod_process_%s_host" % fmt)(None, None, 0, 0, None, None, 0, cnt) == QRL_ERR_ARG
        assert getattr(lib, "qrl_fft_process_" + fmt)(None, None, 0, 0) == QRL_ERR_ARG
    assert lib.qrl_demod_set_sc8_scale(None, 1.0) == QRL_ERR_ARG
    assert lib.qrl_demod_set_cu8_scale(None, 1.0, 127.5) == QRL_ERR_ARG
    assert lib.qrl_fft_set_sc8_scale(None, 1.0) == QRL_ERR_ARG
    assert lib.qrl_fft_set_cu8_scale(None, 1.0, 127.5) == QRL_ERR_ARG


def test_python_binding_has_the_argtypes_and_the_wrappers():
    lib = q.load_library()
    vp, sz, fl = C.c_void_p, C.c_size_t, C.c_float
    for fmt in ("sc8", "cu8"):
        assert list(getattr(lib, "qrl_demod_process_" + fmt).argtypes) == [vp, vp, sz, sz, C.POINTER(q._Out)]
        assert list(getattr(lib, "qrl_demod_process_%s_host" % fmt).argtypes) == [vp, vp, sz, sz, vp, vp, sz, vp]
        assert list(getattr(lib, "qrl_fft_process_" + fmt).argtypes) == [vp, vp, sz, sz]
    assert list(lib.qrl_demod_set_sc8_scale.argtypes) == [vp, fl] and list(lib.qrl_fft_set_sc8_scale.argtypes) == [vp, fl]
    assert list(lib.qrl_demod_set_cu8_scale.argtypes) == [vp, fl, fl] and list(lib.qrl_fft_set_cu8_scale.argtypes) == [vp, fl, fl]
    for cls in (q.Demod, q.Fft):
        for method in ("process_sc8", "process_sc8_async", "process_cu8", "process_cu8_async", "set_sc8_scale", "set_cu8_scale"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
