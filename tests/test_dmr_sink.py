"""The repeater-mode DMR burst sink on the CPU: qradiolink_amd/csrc/dmr_sink_core.hpp, the code k_dmr_sink calls, against the recorded frame
and slot records of tests/golden/ref/dmr_sink.npz byte for byte, call by call under the recorded cuts, flushes and resets; the golden
against the live reference where it is present (its gr_dmr_sink, DMRFrame and DMRTiming, compiled unmodified: tests/host/dmr_sink_ref.cpp);
the slot-time helper of host/dmr_frame_hip.h against the values DMRTiming stored; the same core under the address and
undefined-behaviour sanitizers (tests/host/test_dmr_sink_core.cpp, a program of its own); and the argument errors of the C ABI."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dmr_rx
import dmr_sink
import dmr_tx
import qradiolink_amd as q

ROOT = dmr_sink.ROOT
G = dmr_sink.load_golden()
NAMES = [str(n) for n in G["names"]]
QRL_ERR_ARG = -1


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return dmr_sink.load_core(tmp_path_factory.mktemp("dmr_sink_core"))


def _same(got, exp, cap, what):
    wf, wi, wc = dmr_sink.written(exp, cap)
    assert got["counts"].tolist() == exp["counts"].tolist(), "%s: bursts found per call" % what
    assert np.array_equal(got["call_of"], wc), "%s: the calls the bursts were found in" % what
    bad = np.nonzero((got["frames"] != wf).any(axis=1) | (got["info"] != wi).any(axis=1))[0]
    assert not len(bad), "%s: bursts %s differ; first: %s / %s, reference %s / %s" % (what, bad[:8], got["frames"][bad[0]], got["info"][bad[0]],
                                                                                    wf[bad[0]], wi[bad[0]])


def test_the_golden_has_the_streams_the_device_test_needs():
    assert dmr_sink.NSTREAMS == 72 and len(set(NAMES)) == len(NAMES) == 75
    assert not any(dmr_sink.scenario(G, k)[0].ops for k in range(72)) and all(dmr_sink.scenario(G, k)[0].ops for k in range(72, 75))


@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_golden(core, name):
    x, exp = dmr_sink.scenario(G, name)
    _same(core.run(x), exp, x.cap, name)


def test_core_is_indifferent_to_the_cuts(core):
    """one call, one call per bit, and calls of 31 bits give the records of the recorded cuts (scenarios without flush or reset)"""
    for name in NAMES[:14] + NAMES[72:]:
        x, exp = dmr_sink.scenario(G, name)
        if x.ops or x.cap != 64:
            continue
        for cuts in ([len(x.bits)], [1] * len(x.bits), dmr_sink.ragged(len(x.bits), (31,))):
            got = core.run(dmr_sink.Scenario(name, x.bits, cuts))
            assert np.array_equal(got["frames"], exp["frames"]) and np.array_equal(got["info"], exp["info"]), (name, cuts[:3])


def test_reset_in_mid_burst_is_a_fresh_sink_on_the_remainder():
    a, ea = dmr_sink.scenario(G, "reset_mid_burst")
    b, eb = dmr_sink.scenario(G, "reset_remainder")
    tail = ea["call_of"] >= 1
    assert tail.sum() == len(eb["frames"]) > 0
    assert np.array_equal(ea["frames"][tail], eb["frames"]) and np.array_equal(ea["info"][tail], eb["info"])


def test_slot_time_helper_equals_dmrtiming(core):
    """every value DMRTiming::set_slot_times stored, in every scenario: with rx_time tags on a symbol's first and second bit, and with none"""
    seen = 0
    for name in NAMES[:14] + NAMES[72:]:
        x, exp = dmr_sink.scenario(G, name)
        if x.ops:
            continue   # end_bit starts again at a reset, the scenario's tags do not
        called = [i for i in range(len(exp["info"])) if core.slot_time_set(exp["info"][i])]
        assert [int(exp["info"][i][2]) for i in called] == [int(t[1]) for t in exp["timing"]], name
        for i, t in zip(called, exp["timing"]):
            assert core.slot_time(dmr_sink.end_bit(exp["info"][i]), x.tags) == int(t[2]), (name, i)
            seen += 1
    x, _ = dmr_sink.scenario(G, "tags")
    assert {t[0] & 1 for t in x.tags} == {0, 1} and seen > 50


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dmr_sink_ref")
    r, t = dmr_sink.load_ref(d), dmr_tx.load_ref(d)
    if r is None or t is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r, t


def test_golden_equals_the_live_reference(refs):
    g = dmr_sink.record_golden(*refs)
    assert sorted(g) == sorted(G)
    for k in g:
        assert np.array_equal(g[k], G[k]), k


def _flat_file(path):
    bursts = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(NAMES)))
        for name in NAMES:
            x, exp = dmr_sink.scenario(G, name)
            wf, wi, _ = dmr_sink.written(exp, x.cap)
            f.write(struct.pack("<IIII", len(x.bits), len(x.cuts), x.cap, len(wf)))
            for c, size in enumerate(x.cuts):
                f.write(struct.pack("<III", size, x.ops.get(c, 0), int(exp["counts"][c])))
            f.write(x.bits.tobytes() + wf.tobytes() + wi.tobytes())
            bursts += len(wf)
    return bursts


def test_core_header_equals_the_golden_under_the_sanitizers(tmp_path):
    exe, data = str(tmp_path / "test_dmr_sink_core"), str(tmp_path / "golden.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_dmr_sink_core.cpp"), "-o", exe])
    n = _flat_file(data)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d scenarios, %d bursts" % (len(NAMES), n)), r.stdout


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_exports_and_argtypes():
    header = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    lib = q.load_library()
    for n in ("create", "destroy", "reset", "flush", "process", "sync"):
        assert "qrl_dmr_sink_" + n + "(" in header and "qrl_dmr_sink_" + n in q.EXPORTED_SYMBOLS
        assert getattr(lib, "qrl_dmr_sink_" + n)
    vp, sz = C.c_void_p, C.c_size_t
    assert lib.qrl_dmr_sink_process.argtypes == [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp]
    assert (q.DMR_SINK_FRAME_BYTES, q.DMR_SINK_INFO_BYTES) == (40, 16)


def test_null_arguments_and_bad_sizes_are_arg_errors():
    lib = q.load_library()
    buf = (C.c_uint8 * 512)()
    p = (C.addressof(buf) + 15) & ~15
    fake = p   # never dereferenced: every refusal below comes before the handle or the context is used
    out = C.c_void_p()
    assert lib.qrl_dmr_sink_create(None, 1, None, C.byref(out)) == QRL_ERR_ARG
    assert lib.qrl_dmr_sink_create(fake, 1, None, None) == QRL_ERR_ARG
    assert lib.qrl_dmr_sink_create(fake, 0, None, C.byref(out)) == QRL_ERR_ARG and not out.value
    pr = lib.qrl_dmr_sink_process
    assert pr(None, p, 64, 64, None, 1, p, p, 4, p) == QRL_ERR_ARG
    assert pr(fake, None, 64, 64, None, 1, p, p, 4, p) == QRL_ERR_ARG
    assert pr(fake, p, 64, 64, None, 1, None, p, 4, p) == QRL_ERR_ARG
    assert pr(fake, p, 64, 64, None, 1, p, None, 4, p) == QRL_ERR_ARG
    assert pr(fake, p, 64, 64, None, 1, p, p, 4, None) == QRL_ERR_ARG
    assert pr(fake, p, 64, 64, None, 1, p, p, 0, p) == QRL_ERR_ARG            # cap_frames 0
    assert pr(fake, p, 64, 65, None, 1, p, p, 4, p) == QRL_ERR_ARG            # n past the stride, whatever the batch
    big = (1 << 32) - 128
    assert pr(fake, p, 1 << 33, big, None, 1, p, p, 4, p) == -5                # QRL_ERR_TOO_BIG: n + 127 would wrap the kernel's 32-bit tile count
    assert b"qrl_dmr_sink_process" in lib.qrl_last_error()
    for f in (lib.qrl_dmr_sink_reset, lib.qrl_dmr_sink_flush, lib.qrl_dmr_sink_sync):
        assert f(None) == QRL_ERR_ARG
    lib.qrl_dmr_sink_destroy(None)


# ------------------------------------------------------------------------------------------------------------------ the call layer, repeater mode
RX_NAMES = [str(n) for n in G["rx_names"]]


@pytest.mark.parametrize("name", RX_NAMES)
def test_call_layer_core_equals_the_golden(core, name):
    x, want = dmr_sink.rx_scenario(G, name)
    got = core.run_call(x)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "bursts %s differ; first: core %s, reference %s" % (bad[:8], got[bad[0], :16], want[bad[0], :16])


def test_call_layer_without_slot_records_reads_every_burst_as_undecoded(core):
    """qrl_dmr_rx_process in repeater mode: cachDecoded() false for every burst, so addFrames passes over all that validate"""
    x, _ = dmr_sink.rx_scenario(G, "fixed_slot_1_calls_on_both")
    got = core.run_call(x, with_slots=False)
    f = dmr_rx.flags(got)
    assert ((f & dmr_rx.VALID) != 0).all() and (f == (dmr_rx.VALID | dmr_sink.SLOT_REFUSED)).all() and not got[:, 2:16].any()


def test_dmo_mode_of_the_new_entry_point_is_the_old_call_layer(core):
    """DMO mode with slot records = tests/golden/ref/dmr_rx.npz, recorded before there was a mode: the slot records are not asked"""
    R = dmr_rx.load_golden()
    for k in dmr_rx.plain(R):
        _, inp, want, cc, prom, _ = dmr_rx.scenario(R, str(R["names"][k]))
        x = dmr_sink.RxScenario("dmo", (cc, prom, dmr_sink.MODE_DMO, 1))
        x.frames, x.slots = inp, np.full((len(inp), 16), 0xFF, np.uint8)
        assert np.array_equal(core.run_call(x), want), R["names"][k]


def test_set_mode_argument_errors():
    lib = q.load_library()
    buf = (C.c_uint8 * 512)()
    fake = (C.addressof(buf) + 15) & ~15
    assert lib.qrl_dmr_rx_set_mode(None, 0, 1) == QRL_ERR_ARG
    for mode, ts in ((2, 1), (-1, 1), (0, 0), (0, 3)):
        # the mode is looked at before the handle is touched
        assert lib.qrl_dmr_rx_set_mode(fake, mode, ts) == QRL_ERR_ARG, (mode, ts)
    ps = lib.qrl_dmr_rx_process_slots
    assert ps(None, None, fake, fake, None, 1, 1, fake) == QRL_ERR_ARG
    assert ps(fake, None, None, fake, None, 1, 1, fake) == QRL_ERR_ARG
    assert ps(fake, None, fake, None, None, 1, 1, fake) == QRL_ERR_ARG
    assert ps(fake, None, fake, fake, None, 1, 1, None) == QRL_ERR_ARG
    assert ps(fake, None, fake, fake, None, 1, 0, fake) == QRL_ERR_ARG
    assert b"qrl_dmr_rx_process_slots" in lib.qrl_last_error()
    assert (q.DMR_MODE_REPEATER, q.DMR_MODE_DMO, q.DMR_RX_SLOT_REFUSED) == (0, 1, 0x0800)
    header = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    for text in ("#define QRL_DMR_MODE_REPEATER 0", "#define QRL_DMR_MODE_DMO 1", "#define QRL_DMR_RX_SLOT_REFUSED 0x0800"):
        assert text in header


def test_dmr_frame_hip_reads_the_slot_record(core):
    """cachDecoded(), getSlotNo(), getCACH(), the LCSS / AT readers and endBit() of host/dmr_frame_hip.h on every recorded slot record"""
    u8p = C.POINTER(C.c_uint8)
    core.lib.core_dmr_frame_hip_slot.argtypes = [u8p, u8p, u8p]
    core.lib.core_dmr_frame_hip_slot.restype = None
    l2 = np.zeros(80, np.uint8)
    seen = 0
    for name in NAMES[:17]:
        _, exp = dmr_sink.scenario(G, name)
        for info in exp["info"]:
            out = np.zeros(16, np.uint8)
            core.lib.core_dmr_frame_hip_slot(dmr_sink._p(l2, C.c_uint8), dmr_sink._p(np.ascontiguousarray(info), C.c_uint8), dmr_sink._p(out, C.c_uint8))
            assert np.array_equal(out, info), name
            seen += 1
    assert seen > 80
