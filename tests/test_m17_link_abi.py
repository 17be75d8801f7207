"""The C ABI and the Python surface of the M17 link layer on the CPU: what include/qrl_hip.h defines and declares, what libqrl_hip.so
exports, the ctypes signatures, the refusals that need no device, and the Python signatures and defaults."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import qradiolink_amd as q

import m17_link as M

ROOT = M.ROOT
HEADER = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
RX_NAMES = ["qrl_m17_rx_create", "qrl_m17_rx_destroy", "qrl_m17_rx_reset", "qrl_m17_rx_set_config", "qrl_m17_rx_process", "qrl_m17_rx_get_state"]
TX_NAMES = ["qrl_m17_call_start", "qrl_m17_call_encode", "qrl_m17_call_end"]
ERR_ARG = -1


def _define(name):
    m = re.search(r"^#define %s (\S+)" % name, CODE, flags=re.M)
    assert m, name
    return int(m.group(1), 0)


def test_header_defines():
    assert _define("QRL_M17_RX_RECORD_BYTES") == M.REC == q.M17_RX_RECORD_BYTES == 64
    assert _define("QRL_M17_RX_STATE_BYTES") == M.STATE_PUBLIC == q.M17_RX_STATE_BYTES == 16
    assert _define("QRL_M17_FRAMESYNC_RECORD_BYTES") == M.FS_REC == q.M17_FRAMESYNC_RECORD_BYTES == 56
    assert _define("QRL_M17_CALL_BYTES") == M.CALL_BYTES == q.M17_CALL_BYTES == 32
    assert _define("QRL_M17_CALL_START_BYTES") == M.START_BYTES == q.M17_CALL_START_BYTES == 96
    assert _define("QRL_M17_CALL_END_BYTES") == M.END_BYTES == q.M17_CALL_END_BYTES == 64
    flag_names = ["FRAME", "LSF_VALID", "INFO", "AUDIO", "END", "LICH_OK", "LSF_FROM_LICH", "LOCKED"]
    core = open(os.path.join(ROOT, "qradiolink_amd", "csrc", "m17_link_core.hpp")).read()
    for i, n in enumerate(flag_names):
        assert _define("QRL_M17_RX_" + n) == 1 << i == getattr(q, "M17_RX_" + n) == getattr(M, n)
        assert re.search(r"\bF_%s = 1 << %d\b" % (n, i), core), n
    assert "M17_FS_REC = 56, M17_DEC_REC = 40, M17_RX_REC = 64, M17_RX_STATE_SIZE = 64, M17_RX_STATE_PUBLIC = 16, M17_CALL_BYTES = 32" in core


def test_header_declarations_cite_the_reference():
    flat = " ".join(CODE.split())
    assert "typedef struct qrl_m17_rx qrl_m17_rx;" in flat
    assert "typedef struct { int can_rx; int decode_all_can; } qrl_m17_rx_config;" in flat
    for decl in ("int qrl_m17_rx_create(qrl_ctx* ctx, size_t batch, const qrl_m17_rx_config* config, qrl_m17_rx** out);",
                 "void qrl_m17_rx_destroy(qrl_m17_rx* h);",
                 "int qrl_m17_rx_reset(qrl_m17_rx* h, void* hip_stream);",
                 "int qrl_m17_rx_set_config(qrl_m17_rx* h, const qrl_m17_rx_config* config);",
                 "int qrl_m17_rx_process(qrl_m17_rx* h, void* hip_stream, const uint8_t* frames, size_t frame_stride, const uint32_t* counts, size_t cap_frames, uint8_t* out);",
                 "int qrl_m17_rx_get_state(qrl_m17_rx* h, void* hip_stream, uint8_t* out);",
                 "int qrl_m17_call_start(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, size_t batch, uint8_t* out, size_t out_stride);",
                 "int qrl_m17_call_encode(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint8_t* payloads, const uint32_t* first, size_t batch, size_t n, uint8_t* out, size_t out_stride, size_t slot_bytes);",
                 "int qrl_m17_call_end(qrl_ctx* ctx, void* hip_stream, const uint8_t* calls, const uint32_t* first, size_t batch, uint8_t* out, size_t out_stride);",
                 "void* qrl_framesync_stream(qrl_framesync* f);"):
        assert decl in flat, decl
    for cite in ("src/gr_modem.cpp:1370-1439", "src/M17/M17/M17FrameDecoder.cpp:37-43", "src/M17/M17/M17Transmitter.cpp:46-72", "src/gr_modem.cpp:687-697",
                 "src/gr_modem.cpp:868-884", "src/gr_modem.cpp:718-729", "src/M17/M17/M17LinkSetupFrame.cpp:83-97", "src/M17/M17/M17Callsign.cpp:26-68"):
        assert cite in HEADER, cite
    # the three comments that said the link layer is host work
    assert "the M17 frame decoder itself stays on the host" not in HEADER and "is host work: host/m17_frame_decoder_hip" not in HEADER
    assert "are per-stream state: host work" not in HEADER


def test_exports_and_argtypes():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    for n in RX_NAMES + TX_NAMES + ["qrl_framesync_stream"]:
        assert n in q.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.qrl_m17_rx_create.argtypes == [vp, sz, C.POINTER(q._M17RxConfig), C.POINTER(vp)]
    assert lib.qrl_m17_rx_destroy.argtypes == [vp] and lib.qrl_m17_rx_destroy.restype is None
    assert lib.qrl_m17_rx_reset.argtypes == [vp, vp] and lib.qrl_m17_rx_set_config.argtypes == [vp, C.POINTER(q._M17RxConfig)]
    assert lib.qrl_m17_rx_process.argtypes == [vp, vp, vp, sz, vp, sz, vp] and lib.qrl_m17_rx_get_state.argtypes == [vp, vp, vp]
    assert lib.qrl_m17_call_start.argtypes == [vp, vp, vp, sz, vp, sz]
    assert lib.qrl_m17_call_encode.argtypes == [vp, vp, vp, vp, vp, sz, sz, vp, sz, sz]
    assert lib.qrl_m17_call_end.argtypes == [vp, vp, vp, vp, sz, vp, sz]
    assert [f[0] for f in q._M17RxConfig._fields_] == ["can_rx", "decode_all_can"]


def test_refusals_that_need_no_device():
    lib = q.load_library()
    h = C.c_void_p()
    cfg = q._M17RxConfig(0, 1)
    assert lib.qrl_m17_rx_create(None, 4, C.byref(cfg), C.byref(h)) == ERR_ARG and not h.value
    assert lib.qrl_m17_rx_reset(None, None) == ERR_ARG and lib.qrl_m17_rx_set_config(None, C.byref(cfg)) == ERR_ARG
    assert lib.qrl_m17_rx_process(None, None, None, 0, None, 0, None) == ERR_ARG and lib.qrl_m17_rx_get_state(None, None, None) == ERR_ARG
    assert lib.qrl_m17_call_start(None, None, None, 0, None, 0) == ERR_ARG
    assert lib.qrl_m17_call_encode(None, None, None, None, None, 0, 0, None, 0, 0) == ERR_ARG
    assert lib.qrl_m17_call_end(None, None, None, None, 0, None, 0) == ERR_ARG
    assert lib.qrl_framesync_stream(None) is None
    lib.qrl_m17_rx_destroy(None)


def test_python_surface():
    sig = inspect.signature
    assert list(sig(q.M17Rx.__init__).parameters) == ["self", "ctx", "batch", "can_rx", "decode_all_can"]
    assert sig(q.M17Rx.__init__).parameters["can_rx"].default == 0 and sig(q.M17Rx.__init__).parameters["decode_all_can"].default is True
    assert {"process", "reset", "state", "set_config", "close"} <= set(dir(q.M17Rx))
    p = sig(q.FrameSync.enable_m17_link).parameters
    assert p["can_rx"].default == 0 and p["decode_all_can"].default is True
    for name in ("m17_call_descriptor", "m17_call_start", "m17_call_encode", "m17_call_end", "m17_call_bytes"):
        assert callable(getattr(q, name))


def test_call_descriptor():
    d = q.m17_call_descriptor("YO8RZZ", "AB1CDE", can=3, destination_type=0)
    assert d.dtype == np.uint8 and d.shape == (32,) and bytes(d[:6]) == b"YO8RZZ" and d[9] == 6 and bytes(d[10:16]) == b"AB1CDE" and d[19] == 6
    assert d[20] == 3 and d[21] == 0 and not d[22:].any() and not d[6:9].any()
    d = q.m17_call_descriptor("ABCDEFGHIJKL", "", can=15, destination_type=4)
    assert bytes(d[:9]) == b"ABCDEFGHI" and d[9] == 10 and d[19] == 0 and d[20] == 15 and d[21] == 4
    assert np.array_equal(G_DESC, np.stack([q.m17_call_descriptor(s, t, c, k) for _, s, t, c, k, _ in M.TX_CALLS]))


G_DESC = M.load_golden()["tx_desc"]
