"""Per-stream carrier offsets through the C++ facade (tests/host/test_per_stream_offset.cpp): gr_demod_base_hip::set_carrier_offset(hz, stream)
gives every radio of the batch its own offset, bit-exact with the oracle, and set_mode keeps them; gr_mod_base_hip's back-end-less handle
(1 Msps, zero offset) gains the back end when ONE stream is retuned."""
import os
import subprocess

import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_per_stream_offset")


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "per_stream"])
    return EXE


def test_facade_demod_per_stream_offsets_survive_set_mode(tmp_path):
    offsets = [1200.0, -900.0, 0.0]
    ss = [sig.make_stream("2fsk1k", 2, 1000000, rx_offset_hz=f, seed=40 + b, lead=37 * b)[0] for b, f in enumerate(offsets)]
    n = min(s.size for s in ss) & ~1
    iq = np.stack([s[:n] for s in ss]).astype(np.complex64)
    iq.tofile(str(tmp_path / "iq.bin"))
    r = subprocess.run([_exe(), "demod", "18", "3", str(n), str(tmp_path / "iq.bin"), str(tmp_path / "bits")] + ["%r" % f for f in offsets],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for b, f in enumerate(offsets):
        ref = orc.demod_2fsk(orc.frontend(iq[b], 1000000, f), sps=10, filter_width=2000, fm=False)["bits_a"]
        for run in (0, 1):   # 1: after set_mode (re-open, the phases restart at 0)
            got = np.fromfile(str(tmp_path / ("bits.%d.%d.bin" % (run, b))), dtype=np.uint8)
            assert got.size == ref.size and np.array_equal(got, ref), "run %d stream %d" % (run, b)


def test_facade_mod_one_stream_offset_opens_the_back_end():
    r = subprocess.run([_exe(), "mod"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    assert kv["backend_before"] == "0" and kv["backend_zero"] == "0"
    assert kv["backend_after"] == "1" and float(kv["offset0"]) == 0.0 and float(kv["offset1"]) == 5000.0
    assert kv["backend_reopen"] == "1" and float(kv["offset0_reopen"]) == -7000.0
