"""The C ABI and the Python surface of DMR layer 2 transmit (qrl_dmr_l2_encode, qrl_dmr_voice_call_encode): header text, exports, the
refusals that need no device, the ctypes signatures and the package's wrappers."""
import ctypes as C
import inspect
import os
import re

import pytest

import qradiolink_amd as q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
QRL_ERR_ARG = -1
NAMES = ("qrl_dmr_l2_encode", "qrl_dmr_voice_call_encode")


def _args(name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, HEADER)
    assert m, "%s is not declared in qrl_hip.h" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_header_declares_the_sizes_and_the_calls():
    assert re.search(r"#define\s+QRL_DMR_TX_RECORD_BYTES\s+48\b", HEADER) and re.search(r"#define\s+QRL_DMR_CALL_BYTES\s+40\b", HEADER)
    assert _args("qrl_dmr_l2_encode") == ["qrl_ctx* ctx", "void* hip_stream", "const uint8_t* records", "const uint32_t* counts", "size_t batch",
                                          "size_t cap_frames", "uint8_t* out", "size_t out_stride", "size_t slot_bytes"]
    assert _args("qrl_dmr_voice_call_encode") == ["qrl_ctx* ctx", "void* hip_stream", "const uint8_t* calls", "const uint8_t* voice",
                                                  "const uint32_t* first", "size_t batch", "size_t n", "uint8_t* out", "size_t out_stride",
                                                  "size_t slot_bytes"]
    assert (q.DMR_TX_RECORD_BYTES, q.DMR_CALL_BYTES, q.DMR_SLOT_BYTES) == (48, 40, 72)


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_the_entry_point(name):
    lib = q.load_library()
    assert hasattr(lib, name)
    assert name in q.EXPORTED_SYMBOLS


def test_python_argtypes():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    assert lib.qrl_dmr_l2_encode.argtypes == [vp, vp, vp, vp, sz, sz, vp, sz, sz]
    assert lib.qrl_dmr_voice_call_encode.argtypes == [vp, vp, vp, vp, vp, sz, sz, vp, sz, sz]


def test_null_arguments_and_bad_sizes_are_arg_errors():
    lib = q.load_library()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    fake_ctx = p   # never dereferenced: every refusal below comes before the context is used
    enc, call = lib.qrl_dmr_l2_encode, lib.qrl_dmr_voice_call_encode
    assert enc(None, None, p, None, 1, 1, p, 33, 33) == QRL_ERR_ARG
    assert enc(fake_ctx, None, None, None, 1, 1, p, 33, 33) == QRL_ERR_ARG
    assert enc(fake_ctx, None, p, None, 1, 1, None, 33, 33) == QRL_ERR_ARG
    assert enc(fake_ctx, None, p, None, 0, 1, p, 33, 33) == QRL_ERR_ARG
    assert enc(fake_ctx, None, p, None, 1, 0, p, 33, 33) == QRL_ERR_ARG
    assert enc(fake_ctx, None, p, None, 1, 1, p, 32, 32) == QRL_ERR_ARG            # a slot shorter than a burst
    assert enc(fake_ctx, None, p, None, 1, 2, p, 65, 33) == QRL_ERR_ARG            # a row shorter than its slots
    assert enc(fake_ctx, None, p, None, 1, 2, p, 143, 72) == QRL_ERR_ARG
    assert enc(fake_ctx, None, p, None, 1, 2, p, 1 << 40, (1 << 63) + 40) == QRL_ERR_ARG   # cap_frames * slot_bytes past size_t
    assert b"qrl_dmr_l2_encode" in lib.qrl_last_error()
    assert call(None, None, p, p, None, 1, 1, p, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, None, p, None, 1, 1, p, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, None, None, 1, 1, p, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, p, None, 1, 1, None, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, p, None, 0, 1, p, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, p, None, 1, 0, p, 33, 33) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, p, None, 1, 1, p, 32, 32) == QRL_ERR_ARG
    assert call(fake_ctx, None, p, p, None, 1, 3, p, 98, 33) == QRL_ERR_ARG
    assert b"qrl_dmr_voice_call_encode" in lib.qrl_last_error()


def test_package_wrappers():
    assert list(inspect.signature(q.dmr_l2_encode).parameters) == ["ctx", "records", "counts", "slot_bytes", "out"]
    assert list(inspect.signature(q.dmr_voice_call_encode).parameters) == ["ctx", "calls", "voice", "first", "slot_bytes", "out"]
    assert inspect.signature(q.dmr_voice_call_encode).parameters["first"].default is None
    assert list(inspect.signature(q.dmr_call_slots).parameters) == ["call", "voice", "repeater", "slot_bytes", "stream", "first_byte"]
    assert inspect.signature(q.dmr_call_slots).parameters["slot_bytes"].default == 72
    assert callable(q.dmr_call_descriptor) and callable(q.dmr_voice_call_records)
