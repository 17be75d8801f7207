"""DMR repeater-mode receive through the C++ facade (tests/host/test_dmr_sink_facade.cpp): with set_dmr_repeater on, gr_modem_hip::demodulate
delivers the bursts of the repeater-mode sink through dmrFrames / dmrFramesDecoded / dmrCallEvents, with a slot record each in dmrSlotInfo:
the records the core headers (which tests/test_dmr_sink.py holds to the reference) give for the oracle receiver's port-2 bits of the same
signal, whatever the work() calls were; host/dmr_frame_hip.h reads the slot record; off (the default) the slot callback stays silent and the
other three deliver the DMO slicer's bursts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dmr_l2
import dmr_rx
import dmr_sink

pytestmark = pytest.mark.gpu

ROOT = dmr_sink.ROOT
EXE = os.path.join(ROOT, "tests", "host", "test_dmr_sink_facade")
G = dmr_sink.load_golden()


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "dmr_sink_facade"])
    return EXE


@pytest.fixture(scope="module")
def air(tmp_path_factory, qrl_ctx):
    """the three downlink streams of dmr_sink.radio_rows through the DMR modulator at 1 Msps"""
    import torch
    import qradiolink_amd as q
    d = tmp_path_factory.mktemp("dmr_sink_facade")
    rows = dmr_sink.radio_rows(G)
    mod = q.Mod(qrl_ctx, q.MODEM_DMR, batch=rows.shape[0], max_bytes=rows.shape[1])
    iq = (mod.process(torch.from_numpy(rows).cuda()) * dmr_sink.RADIO_LEVEL).cpu().numpy().astype(np.complex64)
    mod.close()
    n = iq.shape[1] & ~1
    np.ascontiguousarray(iq[:, :n]).tofile(str(d / "iq.bin"))
    return d, n, rows


def _run(air, rep, ts=1, cc=1, prom=1):
    d, n, rows = air
    pre = str(d / ("out%d%d%d" % (rep, ts, prom)))
    r = subprocess.run([_exe(), str(rows.shape[0]), str(n), str(d / "iq.bin"), pre, str(rep), str(ts), str(cc), str(prom)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    load = lambda ext, w, s: np.fromfile("%s.%s.%d.bin" % (pre, ext, s), np.uint8).reshape(-1, w)
    return [(load("raw", 40, s), load("l2", 80, s), load("call", 128, s), load("info", 16, s),
             [[int(v) for v in line.split()] for line in open("%s.get.%d.txt" % (pre, s))]) for s in range(rows.shape[0])]


def _expected(core, row, cfg):
    """the core headers on the oracle receiver's port-2 bits of the row: (frames, info, call records)"""
    import orc
    bits = orc.demod_dmr(orc.mod_dmr(row) * np.float32(dmr_sink.RADIO_LEVEL))["bits_a"]
    f, i, got = core.call(np.zeros(dmr_sink.STATE_BYTES, np.uint8), bits, 64)
    x = dmr_sink.RxScenario("radio", cfg)
    x.frames, x.slots = f[:got], i[:got]
    save, dmr_rx.AUDIO_FEC = dmr_rx.AUDIO_FEC, 0
    try:
        call = core.run_call(x)
    finally:
        dmr_rx.AUDIO_FEC = save
    return f[:got], i[:got], call


@pytest.mark.parametrize("ts,prom", [(1, 1), (2, 0)])
def test_repeater_bursts_arrive_through_the_three_callbacks(air, tmp_path, ts, prom):
    core = dmr_sink.load_core(tmp_path)
    on = _run(air, 1, ts=ts, prom=prom)
    for s, row in enumerate(air[2]):
        raw, l2, rec, info, getters = on[s]
        f, i, call = _expected(core, row, (1, prom, dmr_sink.MODE_REPEATER, ts))
        assert raw.shape[0] == l2.shape[0] == rec.shape[0] == info.shape[0] == len(f) >= 4
        assert np.array_equal(raw, f) and np.array_equal(info, i), "stream %d: the sink's records" % s
        assert np.array_equal(l2, dmr_l2.records(raw, 0)) and np.array_equal(rec, call), "stream %d: layer 2 or the call layer" % s
        for r, g in zip(info, getters):
            end = dmr_sink.end_bit(r)
            assert g[:9] == [int(v) for v in r[:8]] + [end] and g[9] == int(core.slot_time_set(r)) and g[10] == (end // 2) * 5 * dmr_sink.TIME_PER_SAMPLE
    # the LC headers and the terminator are on TS1: the promiscuous tracker takes the call and locks to slot 1, the one fixed on slot 2 refuses it
    rec, info = on[0][2], on[0][3]
    flags, ts1 = dmr_rx.flags(rec), (info[:, 1] != 0) & (info[:, 2] == 1)
    assert ts1.sum() >= 2
    if prom:
        assert (flags[ts1] & dmr_rx.HEADER_VOICE).any() and (rec[ts1, 5] == 1).any() and not (flags & dmr_sink.SLOT_REFUSED).any()
    else:
        assert (flags[ts1] == dmr_rx.VALID | dmr_sink.SLOT_REFUSED).all() and not rec[:, 5].any()


def test_off_is_the_dmo_slicer(air):
    off = _run(air, 0)
    for raw, l2, rec, info, getters in off:
        assert info.size == 0 and not getters and raw.shape[0] == l2.shape[0] == rec.shape[0]
        assert not rec[:, 5].any()            # DMO mode: _timeslot_RX stays 0
