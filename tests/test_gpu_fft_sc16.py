"""int16 IQ (sc16) into the spectrum tap: Fft.process_sc16 followed by get_fft_data() equals, bit for bit, a second Fft fed the converted floats
(float)v * scale through work() -- spectra and the None returns of the fill / transform / hold state machine -- and the first frame is held to
orc.power_spectrum by the rule of tests/test_gpu_side.py::test_rx_fft_spectrum_and_state_machine."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

QRL_ERR_ARG = -1


def _dev16(v):
    import torch
    B, n2 = v.shape
    pitch = (n2 // 2 + 3) // 4 * 4
    buf = torch.zeros((B, 2 * pitch), dtype=torch.int16, device="cuda")
    buf[:, :n2] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return buf[:, :n2]


def _window(n, wintype):
    if wintype == 0:
        return np.hamming(n).astype(np.float32)
    k = 2 * np.pi * np.arange(n) / (n - 1)
    return (0.35875 - 0.48829 * np.cos(k) + 0.14128 * np.cos(2 * k) - 0.01168 * np.cos(3 * k)).astype(np.float32)   # 5: Blackman-Harris


@pytest.mark.parametrize("n,wintype,scale", [(256, 0, 1.0 / 32768.0), (1024, 5, 1.0 / 32768.0), (256, 5, 1.0 / 2047.0)])
def test_fft_sc16_equals_fft_of_the_floats(qrl_ctx, n, wintype, scale):
    import torch
    import qradiolink_amd as q
    rng = np.random.default_rng(n + wintype)
    B = 3
    t = np.arange(3 * n + 10)
    x = np.stack([0.6 * np.exp(2j * np.pi * (0.07 + 0.11 * b) * t) + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size)) for b in range(B)])
    peak = 30000.0 if scale > 1e-4 else 2000.0
    f = np.ascontiguousarray(x.astype(np.complex64)).view(np.float32).reshape(B, -1)
    v = np.rint(f * np.float32(peak / np.abs(f).max())).astype(np.int16)
    lim = 32768 if scale < 1e-4 else 2048
    v[:, 0:10] = np.array([-lim, lim - 1, 0, 1, -1, -lim, lim - 1, 1, 0, -1], np.int16)
    v[:, 2 * n - 4:2 * n] = np.array([lim - 1, -lim, -1, 1], np.int16)
    xf = np.ascontiguousarray(v.astype(np.float32) * np.float32(scale)).view(np.complex64)
    d32 = torch.from_numpy(xf).cuda()
    f16, f32 = q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype), q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype)
    if scale != 1.0 / 32768.0:
        f16.set_sc16_scale(scale)
    for bad in (0.0, float("nan"), float("inf")):
        assert f16.lib.qrl_fft_set_sc16_scale(f16.h, C.c_float(bad)) == QRL_ERR_ARG     # refused: the scale stays

    def step(a, b):
        f16.process_sc16(_dev16(v[:, 2 * a:2 * b]))
        f32.work(d32[:, a:b].contiguous())

    def read():
        g16, g32 = f16.get_fft_data(), f32.get_fft_data()
        assert (g16 is None) == (g32 is None)
        if g16 is None:
            return None
        g16, g32 = g16.cpu().numpy(), g32.cpu().numpy()
        assert g16.shape == (B, n) and np.array_equal(g16.view(np.uint32), g32.view(np.uint32))
        return g16

    step(0, n)
    assert read() is None                                # a new block is disabled: nothing was taken
    f16.set_enabled(True); f32.set_enabled(True)
    step(0, n // 2)
    step(n // 2, n)
    assert read() is None                                # buffer full; the transform runs when the next sample arrives
    step(n, n + 6)                                       # -> FFT of samples [0, n): the frame boundary falls inside this call
    step(n + 6, 2 * n)                                   # held until somebody reads
    got = read()
    assert got is not None
    assert read() is None
    w = _window(n, wintype)
    for b in range(B):
        want = orc.power_spectrum(xf[b, :n], w)
        strong = want > want.max() - 80.0                # float32 FFT against float64: compare where the spectrum is not rounding noise
        assert np.max(np.abs(got[b][strong] - want[strong])) < 0.05
        assert np.argmax(got[b]) == np.argmax(want)
    # the second frame: 6 samples taken before the hold, the rest after the read; formats alternate on the int16 handle
    f16.work(d32[:, 2 * n:3 * n - 6].contiguous())
    f32.work(d32[:, 2 * n:3 * n - 6].contiguous())
    step(3 * n - 6, 3 * n + 2)
    assert read() is not None
    # a misaligned base and a stride that is no multiple of 4 samples are refused
    buf = torch.zeros((B, 2 * (n + 8)), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert f16.lib.qrl_fft_process_sc16(f16.h, C.c_void_p(buf.data_ptr() + 4), n + 8, n) == QRL_ERR_ARG
    assert f16.lib.qrl_fft_process_sc16(f16.h, C.c_void_p(buf.data_ptr()), n + 6, n) == QRL_ERR_ARG
    f16.close(); f32.close()
