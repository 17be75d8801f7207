"""The 8-bit work() overloads of the C++ facade (tests/host/test_iq8_work.cpp), at one device rate with the spectrum tap on:
gr_demod_base_hip::work(const int8_t* const*, n) and work(const uint8_t* const*, n) stage 2 bytes per sample and call qrl_demod_process_sc8 /
_cu8 and, for the tap, qrl_fft_process_sc8 / _cu8 on the same uploaded slot.  Bits and spectra equal those of the cf32 work() fed the converted
floats (float)v / 128, and the bits equal the oracle's.  A 1 Msps object refuses both overloads and goes on with cf32."""
import os
import subprocess

import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_iq8_work")
MODEM_GMSK10K = 22


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "iq8_work"])
    return EXE


def test_facade_8_bit_work_matches_cf32_work_and_oracle(tmp_path):
    S, rate, offset = 2, 4000000, 25000.0
    iq = sig.make_batch("gmsk10k", S, nframes=2, device_rate=rate, rx_offset_hz=offset, seed=23)
    n = iq.shape[1] & ~7
    v = np.clip(np.rint(iq[:, :n].view(np.float32) * np.float32(512.0)), -128, 127).astype(np.int8)     # peak 0.13 -> 68 counts
    assert 20 < np.abs(v.astype(np.int32)).max() < 120
    v.tofile(str(tmp_path / "iq.bin"))
    r = subprocess.run([_exe(), "demod", str(MODEM_GMSK10K), str(S), str(n), str(rate), "%r" % offset, str(tmp_path / "iq.bin"), str(tmp_path / "bits")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert int(kv["frames"]) >= 2, kv
    assert kv["equal_sc8"] == "1", "the sc8 spectra differ from the cf32 ones"
    assert kv["equal_cu8"] == "1", "the cu8 spectra differ from the cf32 ones"
    x = (v.astype(np.float32) * np.float32(1.0 / 128.0)).view(np.complex64)
    for s in range(S):
        ref = orc.demod_gmsk(orc.frontend(x[s], rate, offset))["bits_a"]
        assert ref.size >= 80
        got32 = np.fromfile(str(tmp_path / ("bits.cf32.%d.bin" % s)), dtype=np.uint8)
        for fmt in ("sc8", "cu8"):
            got = np.fromfile(str(tmp_path / ("bits.%s.%d.bin" % (fmt, s))), dtype=np.uint8)
            # the calls of the driver end at the last whole sample pair; all runs see the same samples
            assert got.size == got32.size and np.array_equal(got, got32), "stream %d: %s and cf32 work() differ" % (s, fmt)
            assert got.size >= ref.size - 64 and np.array_equal(got, ref[:got.size]), "stream %d (%s) differs from the oracle" % (s, fmt)


def test_facade_8_bit_work_is_refused_at_1_msps():
    r = subprocess.run([_exe(), "refuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert kv["refused"] == "4" and kv["cf32_after"] == "1"
