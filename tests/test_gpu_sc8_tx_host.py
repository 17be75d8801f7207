"""The int8 work() overload of the transmitter facade (tests/host/test_sc8_tx_work.cpp): gr_mod_base_hip::work(int8_t* const*) downloads 2 bytes
per sample of qrl_mod_process_sc8.  Its samples equal those of the C ABI call made directly with the same settings and the converted oracle output,
under a scale set before two set_mode calls (so it was kept across them), and clipped(s) is the numpy count of saturated components."""
import os
import subprocess

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "test_sc8_tx_work")
MODEM_QPSK250K, MODEM_GMSK10K = 26, 22
S = 3


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc8_tx_work"])
    return EXE


def conv(x, scale):
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(r, -128, 127).astype(np.int8), int(np.count_nonzero((r > 127) | (r < -128)))


@pytest.mark.parametrize("gain,scale", [(1.0, 127.0), (1.0, 100.0), (4.0, 100.0)])
def test_facade_int8_work_qpsk_4_msps(tmp_path, gain, scale):
    rate, offset, n = 4000000, 25000.0, 67
    rng = np.random.default_rng(71)
    data = np.stack([rng.integers(0, 256, n, dtype=np.uint8) for _ in range(S)])
    inc = orc.phase_inc_to_turn(2 * np.pi * offset / 1000000.0)
    # multiply_const_cc(4) is exact in f32: the gain-1 modulator output x 4 is the gain-4 one
    refs = [orc.tx_interp(orc.rotator(orc.mod_qpsk(data[s]) * np.float32(gain), inc), rate) for s in range(S)]
    data.tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([_exe(), str(MODEM_QPSK250K), str(MODEM_GMSK10K), str(S), str(rate), "%r" % offset, "%r" % gain, "%r" % scale, str(n),
                        str(tmp_path / "in.bin"), str(tmp_path / "iq")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    kv = dict(line.split("=", 1) for line in r.stdout.split())
    for s in range(S):
        want, nclip = conv(refs[s], scale)
        facade = np.fromfile(str(tmp_path / ("iq.facade.%d.bin" % s)), dtype=np.int8)
        abi = np.fromfile(str(tmp_path / ("iq.abi.%d.bin" % s)), dtype=np.int8)
        assert facade.size == want.size and np.array_equal(facade, abi), "stream %d: work(int8) differs from qrl_mod_process_sc8" % s
        assert np.array_equal(abi, want), "stream %d differs from the converted oracle output" % s
        if scale != 127.0:
            assert not np.array_equal(want, conv(refs[s], 127.0)[0]), "the scale must show in the samples"
        assert (nclip > 0) == (gain > 1.0)
        assert int(kv["clipped.%d" % s]) == nclip and int(kv["abi_clipped.%d" % s]) == nclip
