"""work(int8) / work(uint8) of the C++ facade at 1 Msps (tests/host/test_iq8_baseband_work.cpp): with gr_demod_base_hip::set_iq8_baseband(true)
the 8-bit overloads stage 2 bytes per sample and deliver the oracle's bits for the converted floats -- sc8 (float)v * scale, cu8
((float)u - bias) * scale with the scale and the bias of set_sc8_scale / set_cu8_scale --, with the spectrum tap reading the same uploaded slot;
the setting survives set_mode, is reachable through gr_modem_hip, is independent of set_sc16_baseband, and without it the overloads throw
as before."""
import os
import subprocess

import numpy as np
import pytest

import iq8_baseband as ib
import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_iq8_baseband_work")


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "iq8_baseband_work"])
    return EXE


def test_facade_8_bit_work_at_1_msps_matches_the_oracle(tmp_path):
    name = "gmsk10k"
    c = ib.case(name)
    v8, u8, scale, offsets = ib.whole(name)
    S, n = 2, v8.shape[1] // 2
    np.ascontiguousarray(v8[:S]).tofile(str(tmp_path / "sc8.bin"))
    np.ascontiguousarray(u8[:S]).tofile(str(tmp_path / "cu8.bin"))
    r = subprocess.run([_exe(), "demod", str(c["modem"]), str(S), str(n), "%r" % offsets[0], "%r" % float(scale), "%r" % float(ib.BIAS1),
                        str(tmp_path / "sc8.bin"), str(tmp_path / "cu8.bin"), str(tmp_path / "bits")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(item.split("=", 1) for item in r.stdout.split())
    assert int(kv["fft_sc8"]) >= 1 and int(kv["fft_cu8"]) >= 1, kv          # the spectrum tap ran on the 8-bit slot beside the demodulator
    for fmt in (ib.SC8, ib.CU8):
        x = ib.whole_converted(name, fmt)
        for s in range(S):
            ref = c["oracle"](orc.frontend(x[s], 1000000, offsets[s]))["bits_a"]
            assert ref.size >= 80
            got = np.fromfile(str(tmp_path / ("bits.%s.%d.bin" % (fmt, s))), dtype=np.uint8)
            assert got.size == ref.size and np.array_equal(got, ref), "%s stream %d differs from the oracle" % (fmt, s)


def test_facade_setter_switches_the_refusal_off_and_on():
    r = subprocess.run([_exe(), "switch"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert kv == {"sc8_refused_by_default": "1", "cu8_refused_by_default": "1", "sc8_refused_under_sc16_baseband": "1",
                  "cu8_refused_under_sc16_baseband": "1", "sc8_refused_when_on": "0", "cu8_refused_when_on": "0",
                  "int16_refused_under_iq8_baseband": "1", "cu8_refused_after_set_mode": "0", "sc8_refused_when_off_again": "1",
                  "cu8_refused_when_off_again": "1", "cu8_refused_after_modem_setter": "0", "done": "1"}, kv
