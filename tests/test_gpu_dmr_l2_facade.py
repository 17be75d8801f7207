"""DMR layer 2 through the C++ facade (tests/host/test_dmr_l2_facade.cpp): with set_dmr_l2 on, gr_modem_hip::demodulate hands every burst of the
dmrFrames callback to dmrFramesDecoded as well, as the 80-byte record the restatement gives for it, and host/dmr_frame_hip.h reads that record
like the reference's DMRFrame; off (the default) nothing changes."""
import os
import subprocess

import numpy as np
import pytest

import dmr_l2
import sig
from test_gpu_dmr_l2 import CC, DST, SRC, _call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_dmr_l2_facade")


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "dmr_l2_facade"])
    return EXE


@pytest.fixture(scope="module")
def air(tmp_path_factory):
    d = tmp_path_factory.mktemp("dmr_l2_facade")
    frames, _, _ = _call(np.random.default_rng(2025))
    x, _ = sig.make_4fsk(levels=sig.dmr_levels(frames), seed=4, cfo=10.0)
    n = x.size & ~1
    iq = np.stack([x[:n], np.roll(x[:n], 3000)]).astype(np.complex64)
    iq.tofile(str(d / "iq.bin"))
    return d, n, len(frames)


def _run(air, l2):
    d, n, _ = air
    pre = str(d / ("out%d" % l2))
    r = subprocess.run([_exe(), "2", str(n), str(d / "iq.bin"), pre, str(l2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [(np.fromfile("%s.raw.%d.bin" % (pre, s), np.uint8).reshape(-1, 40), np.fromfile("%s.l2.%d.bin" % (pre, s), np.uint8).reshape(-1, 80),
             [line.split() for line in open("%s.get.%d.txt" % (pre, s))]) for s in range(2)]


def test_decoded_records_arrive_beside_the_raw_ones(air):
    off, on = _run(air, 0), _run(air, 1)
    for s in range(2):
        raw, l2, getters = on[s]
        assert np.array_equal(raw, off[s][0]) and off[s][1].size == 0            # default off: the raw callback is what it was, nothing else fires
        assert raw.shape[0] == air[2] == l2.shape[0]
        want = dmr_l2.records(raw, 1)
        assert np.array_equal(l2, want)
        for rec, g in zip(want, getters):
            assert [int(v) for v in g] == [rec[4], rec[3], rec[2], int.from_bytes(rec[12:16].tobytes(), "little"), int.from_bytes(rec[16:20].tobytes(), "little"),
                                           rec[9], rec[10], rec[8], int(rec[0] in (1, 2)), rec[20], rec[53], rec[79] if rec[0] in (1, 2) else 0]
        assert [int(g[3]) for g in getters if int(g[1]) in (1, 2, 3, 6)] == [SRC] * 4 and [int(g[4]) for g in getters if int(g[1]) in (1, 2, 3, 6)] == [DST] * 4
        assert {int(g[2]) for g in getters if int(g[1]) < 16} == {CC}
