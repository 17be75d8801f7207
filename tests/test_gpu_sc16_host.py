"""The int16 work() overload of the C++ facade (tests/host/test_sc16_work.cpp): gr_demod_base_hip::work(const int16_t* const*, n) stages 4 bytes
per sample and calls qrl_demod_process_sc16; its bits equal those of the cf32 work() fed (float)v / 32768 and those of the oracle.  A 1 Msps
object refuses the overload and goes on with cf32."""
import os
import subprocess

import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_sc16_work")
MODEM_GMSK10K = 22


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc16_work"])
    return EXE


def test_facade_int16_work_matches_cf32_work_and_oracle(tmp_path):
    S, rate, offset = 2, 4000000, 25000.0
    iq = sig.make_batch("gmsk10k", S, nframes=2, device_rate=rate, rx_offset_hz=offset, seed=23)
    n = iq.shape[1] & ~3
    v = np.clip(np.rint(iq[:, :n].view(np.float32) * np.float32(131072.0)), -32768, 32767).astype(np.int16)     # amplitude 0.05 -> about 6 500 counts
    v.tofile(str(tmp_path / "iq.bin"))
    r = subprocess.run([_exe(), "demod", str(MODEM_GMSK10K), str(S), str(n), str(rate), "%r" % offset, str(tmp_path / "iq.bin"), str(tmp_path / "bits")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    x = (v.astype(np.float32) * np.float32(1.0 / 32768.0)).view(np.complex64)
    for s in range(S):
        ref = orc.demod_gmsk(orc.frontend(x[s], rate, offset))["bits_a"]
        assert ref.size >= 80
        got16 = np.fromfile(str(tmp_path / ("bits.sc16.%d.bin" % s)), dtype=np.uint8)
        got32 = np.fromfile(str(tmp_path / ("bits.cf32.%d.bin" % s)), dtype=np.uint8)
        # the calls of the driver end at the last whole chunk pair; both runs see the same samples
        assert got16.size == got32.size and np.array_equal(got16, got32), "stream %d: int16 and cf32 work() differ" % s
        assert got16.size >= ref.size - 64 and np.array_equal(got16, ref[:got16.size]), "stream %d differs from the oracle" % s


def test_facade_int16_work_is_refused_at_1_msps():
    r = subprocess.run([_exe(), "refuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert kv["refused"] == "1" and kv["cf32_after"] == "1"
