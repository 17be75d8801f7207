"""The C ABI and the Python surface of the DMR receive call layer on the CPU: what include/qrl_hip.h defines and declares, what
libqrl_hip.so exports, the ctypes signatures, the refusals that need no device, and the Python signatures and defaults."""
import ctypes as C
import inspect
import os
import re

import qradiolink_amd as q

import dmr_rx

ROOT = dmr_rx.ROOT
HEADER = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
NAMES = ["qrl_dmr_rx_create", "qrl_dmr_rx_destroy", "qrl_dmr_rx_reset", "qrl_dmr_rx_set_config", "qrl_dmr_rx_process", "qrl_dmr_rx_get_state"]
ERR_ARG = -1


def _define(name):
    m = re.search(r"^#define %s (\S+)" % name, CODE, flags=re.M)
    assert m, name
    return int(m.group(1), 0)


def test_header_defines():
    assert _define("QRL_DMR_RX_RECORD_BYTES") == dmr_rx.REC == q.DMR_RX_RECORD_BYTES == 128
    assert _define("QRL_DMR_RX_STATE_BYTES") == dmr_rx.STATE_PUBLIC == q.DMR_RX_STATE_BYTES == 12
    flag_names = ["VALID", "PROCESSED", "HEADER_VOICE", "HEADER_DATA", "TERMINATOR", "END_BEEP", "AUDIO", "EMBEDDED", "TALKER_ALIAS", "GPS", "UNKNOWN_FLCO"]
    for i, n in enumerate(flag_names):
        assert _define("QRL_DMR_RX_" + n) == 1 << i == getattr(q, "DMR_RX_" + n) == getattr(dmr_rx, n)
    core = open(os.path.join(ROOT, "qradiolink_amd", "csrc", "dmr_rx_core.hpp")).read()
    for i, n in enumerate(flag_names):
        assert re.search(r"\bF_%s = 1 << %d\b" % (n, i), core), n
    assert "DMR_RX_REC = 128, DMR_RX_STATE_SIZE = 128, DMR_RX_STATE_PUBLIC = 12, TA_MAX = 68" in core


def test_header_declarations():
    flat = " ".join(CODE.split())
    assert "typedef struct qrl_dmr_rx qrl_dmr_rx;" in flat
    assert "typedef struct qrl_dmr_rx_config { int color_code; int promiscuous; } qrl_dmr_rx_config;" in flat
    for decl in ("int qrl_dmr_rx_create(qrl_ctx* ctx, size_t batch, const qrl_dmr_rx_config* config, qrl_dmr_rx** out);",
                 "void qrl_dmr_rx_destroy(qrl_dmr_rx* h);",
                 "int qrl_dmr_rx_reset(qrl_dmr_rx* h, void* hip_stream);",
                 "int qrl_dmr_rx_set_config(qrl_dmr_rx* h, const qrl_dmr_rx_config* config);",
                 "int qrl_dmr_rx_process(qrl_dmr_rx* h, void* hip_stream, const uint8_t* l2_records , const uint32_t* counts , size_t cap_frames, uint8_t* out );",
                 "int qrl_dmr_rx_get_state(qrl_dmr_rx* h, void* hip_stream, uint8_t* out );"):
        assert decl in flat, decl
    assert "stays host work. */\n#define QRL_DMR_L2_RECORD_BYTES" not in HEADER        # the layer-2 comment points at the call layer now


def test_exports_and_argtypes():
    lib = q.load_library()
    vp, sz = C.c_void_p, C.c_size_t
    for n in NAMES:
        assert n in q.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.qrl_dmr_rx_create.argtypes == [vp, sz, C.POINTER(q._DmrRxConfig), C.POINTER(vp)]
    assert lib.qrl_dmr_rx_destroy.argtypes == [vp] and lib.qrl_dmr_rx_destroy.restype is None
    assert lib.qrl_dmr_rx_reset.argtypes == [vp, vp]
    assert lib.qrl_dmr_rx_set_config.argtypes == [vp, C.POINTER(q._DmrRxConfig)]
    assert lib.qrl_dmr_rx_process.argtypes == [vp, vp, vp, vp, sz, vp]
    assert lib.qrl_dmr_rx_get_state.argtypes == [vp, vp, vp]
    assert [f[0] for f in q._DmrRxConfig._fields_] == ["color_code", "promiscuous"] and C.sizeof(q._DmrRxConfig) == 8


def test_refusals_that_need_no_device():
    lib = q.load_library()
    h = C.c_void_p(0x1234)
    good = q._DmrRxConfig(1, 0)
    fake_ctx = C.c_int(0)               # never read: every refusal below comes before the first device call
    ctx = C.addressof(fake_ctx)
    assert lib.qrl_dmr_rx_create(None, 4, C.byref(good), C.byref(h)) == ERR_ARG and not h.value
    assert lib.qrl_dmr_rx_create(ctx, 0, C.byref(good), C.byref(h)) == ERR_ARG
    assert lib.qrl_dmr_rx_create(ctx, 4, None, C.byref(h)) == ERR_ARG
    assert lib.qrl_dmr_rx_create(ctx, 4, C.byref(good), None) == ERR_ARG
    for cc, prom in ((-1, 0), (16, 0), (255, 1), (1, 2), (1, -1)):
        h = C.c_void_p(0x1234)
        assert lib.qrl_dmr_rx_create(ctx, 4, C.byref(q._DmrRxConfig(cc, prom)), C.byref(h)) == ERR_ARG and not h.value, (cc, prom)
        assert b"colour code" in lib.qrl_last_error()
    buf = (C.c_uint8 * 256)()
    assert lib.qrl_dmr_rx_process(None, None, buf, None, 1, buf) == ERR_ARG
    assert lib.qrl_dmr_rx_reset(None, None) == ERR_ARG
    assert lib.qrl_dmr_rx_set_config(None, C.byref(good)) == ERR_ARG
    assert lib.qrl_dmr_rx_get_state(None, None, buf) == ERR_ARG
    lib.qrl_dmr_rx_destroy(None)


def test_python_signatures_and_defaults():
    sig = inspect.signature(q.DmrRx.__init__)
    assert list(sig.parameters) == ["self", "ctx", "batch", "colour_code", "promiscuous"]
    assert sig.parameters["colour_code"].default == 1 and sig.parameters["promiscuous"].default is False
    assert list(inspect.signature(q.DmrRx.process).parameters) == ["self", "l2", "counts", "out", "stream"]
    assert list(inspect.signature(q.DmrRx.set_config).parameters) == ["self", "colour_code", "promiscuous"]
    for name in ("reset", "state"):
        assert list(inspect.signature(getattr(q.DmrRx, name)).parameters) == ["self", "stream"]
    sig = inspect.signature(q.Demod.enable_dmo_call)
    assert list(sig.parameters) == ["self", "colour_code", "promiscuous"]
    assert sig.parameters["colour_code"].default == 1 and sig.parameters["promiscuous"].default is False
    # off unless asked for: nothing in the constructor or in enable_dmo_l2 makes a tracker
    src = inspect.getsource(q.Demod)
    assert src.count("DmrRx(") == 1 and "DmrRx(" in inspect.getsource(q.Demod.enable_dmo_call)
    assert "dmo_call_rx.reset" in inspect.getsource(q.Demod.reset)
