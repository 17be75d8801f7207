"""The C ABI and the Python surface of DMR layer 2 (qrl_dmr_l2_decode, qrl_dmr_trellis34_decode / _encode): header text, exports, the
refusals that need no device, the ctypes signatures and the package's wrappers."""
import ctypes as C
import inspect
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
QRL_OK, QRL_ERR_ARG = 0, -1
NAMES = ("qrl_dmr_l2_decode", "qrl_dmr_trellis34_decode", "qrl_dmr_trellis34_encode")


def _decl(name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, HEADER)
    assert m, "%s is not declared in qrl_hip.h" % name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_the_record_and_the_calls():
    assert re.search(r"#define\s+QRL_DMR_L2_RECORD_BYTES\s+80\b", HEADER)
    args = [a.strip() for a in _decl("qrl_dmr_l2_decode").split(",")]
    assert [re.sub(r"\s+", " ", a) for a in args] == ["qrl_ctx* ctx", "void* hip_stream", "const uint8_t* records", "const uint32_t* counts",
                                                       "size_t batch", "size_t cap_frames", "int audio_fec", "uint8_t* out"]
    assert len(_decl("qrl_dmr_trellis34_decode").split(",")) == 6
    assert len(_decl("qrl_dmr_trellis34_encode").split(",")) == 5


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_the_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_python_argtypes():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert lib.qrl_dmr_l2_decode.argtypes == [vp, vp, vp, vp, sz, sz, C.c_int, vp]
    assert lib.qrl_dmr_trellis34_decode.argtypes == [vp, vp, vp, sz, vp, vp]
    assert lib.qrl_dmr_trellis34_encode.argtypes == [vp, vp, vp, sz, vp]


def test_null_arguments_and_empty_mailboxes_are_arg_errors():
    lib = q.load_library()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    fake_ctx = p   # never dereferenced: every refusal below comes before the context is used
    assert lib.qrl_dmr_l2_decode(None, None, p, None, 1, 1, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_l2_decode(fake_ctx, None, None, None, 1, 1, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_l2_decode(fake_ctx, None, p, None, 1, 1, 1, None) == QRL_ERR_ARG
    assert lib.qrl_dmr_l2_decode(fake_ctx, None, p, None, 0, 1, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_l2_decode(fake_ctx, None, p, None, 1, 0, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_decode(None, None, p, 1, p, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_decode(fake_ctx, None, None, 1, p, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_decode(fake_ctx, None, p, 1, None, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_decode(fake_ctx, None, p, 1, p, None) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_encode(None, None, p, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_encode(fake_ctx, None, None, 1, p) == QRL_ERR_ARG
    assert lib.qrl_dmr_trellis34_encode(fake_ctx, None, p, 1, None) == QRL_ERR_ARG
    assert b"qrl_dmr_trellis34_encode" in lib.qrl_last_error()


def test_package_wrappers():
    assert list(inspect.signature(q.dmr_l2_decode).parameters) == ["ctx", "frames", "counts", "audio_fec"]
    assert inspect.signature(q.dmr_l2_decode).parameters["counts"].default is None
    assert inspect.signature(q.dmr_l2_decode).parameters["audio_fec"].default is True
    assert callable(q.dmr_trellis34_decode) and callable(q.dmr_trellis34_encode)
    assert inspect.signature(q.Demod.enable_dmo_l2).parameters["audio_fec"].default is True
