"""16-bit integer IQ for the wideband receivers and the spectrum tap at the C ABI, on CPU: include/qrl_hip.h declares qrl_chan_process_sc16,
qrl_chan_channelize_sc16, qrl_chan_set_sc16_scale, qrl_fft_process_sc16 and qrl_fft_set_sc16_scale, libqrl_hip.so exports them, a NULL handle
is QRL_ERR_ARG before any device work, and the Python binding has their argtypes and the Channelizer / Fft methods."""
import ctypes as C
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRL_ERR_ARG = -1
SC16_IN = r"const\s+int16_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+"
DECLS = {
    "qrl_chan_process_sc16": r"qrl_chan\s*\*\s*\w+\s*,\s*" + SC16_IN + r"\s*,\s*int16_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+",
    "qrl_chan_channelize_sc16": r"qrl_chan\s*\*\s*\w+\s*,\s*" + SC16_IN + r"\s*,\s*float\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*int\s+\w+",
    "qrl_chan_set_sc16_scale": r"qrl_chan\s*\*\s*\w+\s*,\s*float\s+\w+",
    "qrl_fft_process_sc16": r"qrl_fft\s*\*\s*\w+\s*,\s*" + SC16_IN,
    "qrl_fft_set_sc16_scale": r"qrl_fft\s*\*\s*\w+\s*,\s*float\s+\w+",
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qrl_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(DECLS))
def test_header_declares_sc16_entry_point(name):
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, DECLS[name]), _header()), "%s is not declared as the issue states it" % name


def test_header_comment_states_the_rules():
    text = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+qrl_chan_process_sc16\s*\(", text, flags=re.S)
    assert m, "no comment in front of qrl_chan_process_sc16"
    for word in ("QRL_ERR_ARG", "32768", "16-byte", "form 3", "qrl_chan_process_channels"):
        assert word in m.group(1), word


@pytest.mark.parametrize("name", sorted(DECLS))
def test_library_exports_sc16_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_null_handle_is_an_arg_error():
    lib = q.load_library()
    buf = (C.c_int16 * 64)()
    assert lib.qrl_chan_process_sc16(None, None, 0, 0, None, 0, None) == QRL_ERR_ARG
    assert lib.qrl_chan_process_sc16(None, buf, 16, 16, None, 0, None) == QRL_ERR_ARG
    assert lib.qrl_chan_channelize_sc16(None, buf, 16, 16, buf, 16, 1) == QRL_ERR_ARG
    assert lib.qrl_chan_set_sc16_scale(None, 1.0) == QRL_ERR_ARG
    assert lib.qrl_fft_process_sc16(None, buf, 16, 16) == QRL_ERR_ARG
    assert lib.qrl_fft_set_sc16_scale(None, 1.0) == QRL_ERR_ARG


def test_python_binding_has_the_argtypes_and_methods():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert list(lib.qrl_chan_process_sc16.argtypes) == [vp, vp, sz, sz, vp, sz, vp]
    assert list(lib.qrl_chan_channelize_sc16.argtypes) == [vp, vp, sz, sz, vp, sz, C.c_int]
    assert list(lib.qrl_chan_set_sc16_scale.argtypes) == [vp, C.c_float]
    assert list(lib.qrl_fft_process_sc16.argtypes) == [vp, vp, sz, sz]
    assert list(lib.qrl_fft_set_sc16_scale.argtypes) == [vp, C.c_float]
    for method in ("process_sc16", "process_sc16_async", "channelize_sc16_async", "set_sc16_scale"):
        assert callable(getattr(q.Channelizer, method)), method
    for method in ("process_sc16", "set_sc16_scale"):
        assert callable(getattr(q.Fft, method)), method
