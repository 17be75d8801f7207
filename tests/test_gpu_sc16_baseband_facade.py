"""work(int16) of the C++ facade at 1 Msps (tests/host/test_sc16_baseband_work.cpp): with gr_demod_base_hip::set_sc16_baseband(true) the
int16 overload stages 4 bytes per sample and delivers the bits the cf32 work() delivers for (float)v / 32768, which are the oracle's; the
setting survives set_mode, is reachable through gr_modem_hip, and without it the overload is refused as before."""
import os
import subprocess

import numpy as np
import pytest

import orc
import sc16_baseband as sb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_sc16_baseband_work")


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc16_baseband_work"])
    return EXE


def test_facade_int16_work_at_1_msps_matches_cf32_work_and_oracle(tmp_path):
    c = sb.case("gmsk10k")
    v, offsets = sb.inputs("gmsk10k", False)
    S, n = 2, v.shape[1] // 2
    np.ascontiguousarray(v[:S]).tofile(str(tmp_path / "iq.bin"))
    r = subprocess.run([_exe(), "demod", str(c["modem"]), str(S), str(n), "%r" % offsets[0], str(tmp_path / "iq.bin"), str(tmp_path / "bits")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    x = (v[:S].astype(np.float32) * sb.SCALE0).view(np.complex64)        # the facade's scale is the default for the whole stream
    for s in range(S):
        ref = c["oracle"](orc.frontend(x[s], 1000000, offsets[s]))["bits_a"]
        assert ref.size >= 80
        got16 = np.fromfile(str(tmp_path / ("bits.sc16.%d.bin" % s)), dtype=np.uint8)
        got32 = np.fromfile(str(tmp_path / ("bits.cf32.%d.bin" % s)), dtype=np.uint8)
        assert got16.size == got32.size and np.array_equal(got16, got32), "stream %d: int16 and cf32 work() differ" % s
        assert got16.size == ref.size and np.array_equal(got16, ref), "stream %d differs from the oracle" % s


def test_facade_setter_switches_the_refusal_off_and_on():
    r = subprocess.run([_exe(), "switch"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert kv == {"refused_by_default": "1", "refused_when_on": "0", "refused_after_set_mode": "0", "refused_when_off_again": "1",
                  "refused_after_modem_setter": "0", "done": "1"}, kv
