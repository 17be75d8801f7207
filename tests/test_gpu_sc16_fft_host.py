"""The spectrum tap under the int16 work() overload of the C++ facade (tests/host/test_sc16_fft_work.cpp): gr_demod_base_hip at 2 Msps with
enable_gui_fft(true) takes work(const int16_t* const*, n) without throwing, and its spectra equal, bit for bit, those of a second object fed
(float)v / 32768 through the cf32 work() -- with the demodulator valve open and with it closed."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_sc16_fft_work")


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc16_fft_work"])
    return EXE


def test_facade_int16_work_feeds_the_spectrum_tap():
    r = subprocess.run([_exe()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    for valve in ("open", "closed"):
        assert kv["threw_" + valve] == "0", "work(int16) threw with the spectrum tap on (valve %s)" % valve
        assert int(kv["frames_" + valve]) >= 2, kv
        assert kv["equal_" + valve] == "1", "valve %s: the int16 spectra differ from the cf32 ones" % valve
