"""DMR layer 2 transmit through the C++ facade (tests/host/test_dmr_tx_facade.cpp): gr_mod_base_hip::setDMRCall / txDMRVoice build a call's
voice bursts on the device inside the modulator's input and give the same IQ as setDMRData fed the reference's recorded bursts, in passes
that cut the 72-byte slots at every offset; setDMRData itself still gives the oracle's gr_mod_dmr chain; host/dmr_frame_hip.h writes the
two records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dmr_tx
import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_dmr_tx_facade")
G = dmr_tx.load_golden()
CALLS_USED, NV = (0, 2, 10), 13          # DMO calls; 13 voice bursts: two superframes and a burst of the talker-alias header


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "dmr_tx_facade"])
    return EXE


def _frames(m):
    assert G["call_repeater"][m] == 0
    n = int(G["call_nslots"][m])
    return np.concatenate([G["call_frames"][m, :2 + NV], G["call_frames"][m, n - 4:n - 3]])


@pytest.mark.parametrize("max_bytes", [60, 201, 8190])
def test_call_and_voice_give_the_iq_of_the_recorded_bursts(tmp_path, max_bytes):
    """passes of 60 bytes: every slot is cut, some twice; of 201 bytes: slots cut at offsets 57, 42, 27, 12 and 69, inside the burst and inside
    the idle bytes; of 8190: one pass takes the whole call"""
    with open(str(tmp_path / "calls.bin"), "wb") as f:
        f.write(struct.pack("<II", len(CALLS_USED), NV))
        for m in CALLS_USED:
            f.write(G["calls"][m].tobytes() + G["call_voice"][m, :NV].tobytes() + _frames(m).tobytes())
    pre = str(tmp_path / "out")
    r = subprocess.run([_exe(), str(tmp_path / "calls.bin"), pre, str(max_bytes)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok %d streams" % len(CALLS_USED)), r.stdout + r.stderr
    for s, m in enumerate(CALLS_USED):
        call, data = np.fromfile("%s.call.%d.bin" % (pre, s), np.uint32), np.fromfile("%s.data.%d.bin" % (pre, s), np.uint32)
        frames = _frames(m)
        slots = np.zeros((frames.shape[0], 72), np.uint8)
        slots[:, :33] = frames
        nbytes = slots.size
        assert nbytes % 3 == 0 and data.size == 2 * (nbytes // 3) * 2500
        assert np.array_equal(call, data), "stream %d: setDMRCall / txDMRVoice and setDMRData differ" % s
        want = orc.mod_dmr(slots.reshape(-1), zero_runs=[(20 * (72 * i + 33), 780) for i in range(frames.shape[0])])
        g, w = data.view(np.float32) + np.float32(0), want.view(np.float32) + np.float32(0)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "stream %d: setDMRData differs from the oracle's gr_mod_dmr" % s
