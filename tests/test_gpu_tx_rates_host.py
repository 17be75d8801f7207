"""The transmitter facade at 100 Msps through the driver that is already there (tests/host/test_sc16_tx_work.cpp): gr_mod_base_hip passes the device
rate through to qrl_mod_create / qrl_amod_create, and both work() overloads (int16 and cf32) give the oracle's back end at that rate: the int16
samples equal the converted cf32 samples of a second object fed the same queue and the converted oracle output, and clipped(s) is the numpy count."""
import os
import subprocess

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_sc16_tx_work")
MODEM_QPSK250K, MODEM_NBFM5000 = 26, 9
S = 2
RATE = 100000000


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc16_tx_work"])
    return EXE


def conv(x, scale=32767.0):
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(r, -32768, 32767).astype(np.int16), int(np.count_nonzero((r > 32767) | (r < -32768)))


def _run(tmp_path, kind, modem, rate, offset, gain, n, payload):
    payload.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([_exe(), kind, str(modem), str(S), str(rate), "%r" % offset, "%r" % gain, str(n), str(tmp_path / "in.bin"), str(tmp_path / "iq")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    got16 = [np.fromfile(str(tmp_path / ("iq.sc16.%d.bin" % s)), dtype=np.int16) for s in range(S)]
    got32 = [np.fromfile(str(tmp_path / ("iq.cf32.%d.bin" % s)), dtype=np.complex64) for s in range(S)]
    return got16, got32, kv


def _check(got16, got32, kv, refs, expect_clip):
    for s in range(S):
        want, nclip = conv(refs[s])
        assert got32[s].size == refs[s].size and got16[s].size == 2 * refs[s].size, "stream %d: sample counts differ" % s
        assert np.array_equal(got32[s].view(np.uint32), refs[s].view(np.uint32)), "stream %d: cf32 work() differs from the oracle" % s
        assert np.array_equal(got16[s], conv(got32[s])[0]), "stream %d: int16 work() differs from the converted cf32 work()" % s
        assert np.array_equal(got16[s], want), "stream %d differs from the converted oracle output" % s
        assert (nclip > 0) == expect_clip
        assert int(kv["clipped.%d" % s]) == nclip, "stream %d: clipped() %s, numpy %d" % (s, kv["clipped.%d" % s], nclip)
        assert int(kv["clipped_cf32.%d" % s]) == 0


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_facade_work_qpsk_100_msps(tmp_path, gain):
    offset, n = 25000.0, 67
    rng = np.random.default_rng(63)
    data = np.stack([rng.integers(0, 256, n, dtype=np.uint8) for _ in range(S)])
    inc = orc.phase_inc_to_turn(2 * np.pi * offset / 1000000.0)
    # multiply_const_cc(4) is exact in f32: the gain-1 modulator output x 4 is the gain-4 one
    refs = [orc.tx_interp(orc.rotator(orc.mod_qpsk(data[s]) * np.float32(gain), inc), RATE) for s in range(S)]
    got16, got32, kv = _run(tmp_path, "mod", MODEM_QPSK250K, RATE, offset, gain, n, data)
    _check(got16, got32, kv, refs, expect_clip=gain > 1.0)


@pytest.mark.parametrize("gain", [1.0, 4.0])
def test_facade_work_nbfm_100_msps(tmp_path, gain):
    offset, n = -12500.0, 64
    t = np.arange(n) / 8000.0
    audio = np.stack([0.5 * np.sin(2 * np.pi * 700 * t) + 0.2 * np.sin(2 * np.pi * 1900 * t),
                      np.random.default_rng(64).uniform(-0.7, 0.7, n)]).astype(np.float32)
    inc = orc.phase_inc_to_turn(2 * np.pi * offset / 1000000.0)
    refs = [orc.tx_interp(orc.rotator(orc.mod_nbfm(audio[s], filter_width=5000, bb_gain=gain), inc), RATE) for s in range(S)]
    got16, got32, kv = _run(tmp_path, "amod", MODEM_NBFM5000, RATE, offset, gain, n, audio)
    _check(got16, got32, kv, refs, expect_clip=gain > 1.0)
