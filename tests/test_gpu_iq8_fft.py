"""8-bit IQ (sc8, cu8) into the spectrum tap, as tests/test_gpu_fft_sc16.py does it for int16: Fft.process_sc8 / process_cu8 followed by
get_fft_data() equal, bit for bit, a second Fft fed the converted floats through work() -- spectra and the None returns of the fill / transform /
hold state machine -- and the first frame is held to orc.power_spectrum.  Two FFT sizes, two windows, calls shorter and longer than the FFT
size, and a scale and bias that are not the defaults."""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_fft_sc16 import _window

pytestmark = pytest.mark.gpu

QRL_ERR_ARG = -1
F = np.float32


def _dev8(v):
    """[B, 2 k] int8 / uint8 -> a cuda view whose row pitch is a multiple of 8 samples"""
    import torch
    B, n2 = v.shape
    pitch = (n2 // 2 + 7) // 8 * 8
    buf = torch.zeros((B, 2 * pitch), dtype=torch.int8 if v.dtype == np.int8 else torch.uint8, device="cuda")
    buf[:, :n2] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return buf[:, :n2]


@pytest.mark.parametrize("fmt,n,wintype,scale,bias", [
    ("sc8", 256, 0, 1.0 / 128.0, None), ("sc8", 1024, 5, 0.0123, None),
    ("cu8", 256, 5, 1.0 / 128.0, 127.5), ("cu8", 1024, 0, 1.0 / 127.0, float(F(127.4))),
])
def test_fft_iq8_equals_fft_of_the_floats(qrl_ctx, fmt, n, wintype, scale, bias):
    import torch
    import qradiolink_amd as q
    rng = np.random.default_rng(n + wintype)
    B = 3
    t = np.arange(3 * n + 10)
    x = np.stack([0.6 * np.exp(2j * np.pi * (0.07 + 0.11 * b) * t) + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size)) for b in range(B)])
    f = np.ascontiguousarray(x.astype(np.complex64)).view(np.float32).reshape(B, -1)
    v = np.rint(f * np.float32(110.0 / np.abs(f).max())).astype(np.int8)
    v[:, 0:10] = np.array([-128, 127, 0, 1, -1, -128, 127, 1, 0, -1], np.int8)
    v[:, 2 * n - 4:2 * n] = np.array([127, -128, -1, 1], np.int8)
    if fmt == "sc8":
        codes = v
        xf = np.ascontiguousarray(v.astype(F) * F(scale)).view(np.complex64)
    else:
        codes = (v.astype(np.int16) + 128).astype(np.uint8)
        xf = np.ascontiguousarray((codes.astype(F) - F(bias)) * F(scale)).view(np.complex64)
    d32 = torch.from_numpy(xf).cuda()
    f8, f32 = q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype), q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype)
    if fmt == "sc8":
        if scale != 1.0 / 128.0:
            f8.set_sc8_scale(scale)
        for bad in (0.0, float("nan"), float("inf")):
            assert f8.lib.qrl_fft_set_sc8_scale(f8.h, C.c_float(bad)) == QRL_ERR_ARG     # refused: the scale stays
    else:
        if (scale, bias) != (1.0 / 128.0, 127.5):
            f8.set_cu8_scale(scale, bias)
        for bad in (0.0, float("nan"), float("inf")):
            assert f8.lib.qrl_fft_set_cu8_scale(f8.h, C.c_float(bad), C.c_float(127.5)) == QRL_ERR_ARG
        for bad in (float("nan"), float("inf")):
            assert f8.lib.qrl_fft_set_cu8_scale(f8.h, C.c_float(1.0), C.c_float(bad)) == QRL_ERR_ARG
    run8 = f8.process_sc8 if fmt == "sc8" else f8.process_cu8

    def step(a, b):
        run8(_dev8(codes[:, 2 * a:2 * b]))
        f32.work(d32[:, a:b].contiguous())

    def read():
        g8, g32 = f8.get_fft_data(), f32.get_fft_data()
        assert (g8 is None) == (g32 is None)
        if g8 is None:
            return None
        g8, g32 = g8.cpu().numpy(), g32.cpu().numpy()
        assert g8.shape == (B, n) and np.array_equal(g8.view(np.uint32), g32.view(np.uint32))
        return g8

    step(0, n)
    assert read() is None                                # a new block is disabled: nothing was taken
    f8.set_enabled(True); f32.set_enabled(True)
    step(0, n // 2)                                      # calls shorter than the FFT size
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
    # the second frame: 6 samples taken before the hold, the rest after the read; formats alternate on the 8-bit handle
    f8.work(d32[:, 2 * n:3 * n - 6].contiguous())
    f32.work(d32[:, 2 * n:3 * n - 6].contiguous())
    step(3 * n - 6, 3 * n + 2)
    assert read() is not None
    # one call longer than the FFT size: the frame boundary inside it, the transform of the frame before at its start
    f8b, f32b = q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype), q.Fft(qrl_ctx, B, fftsize=n, wintype=wintype)
    if fmt == "sc8":
        f8b.set_sc8_scale(scale)
    else:
        f8b.set_cu8_scale(scale, bias)
    f8b.set_enabled(True); f32b.set_enabled(True)
    (f8b.process_sc8 if fmt == "sc8" else f8b.process_cu8)(_dev8(codes[:, 0:2 * (2 * n + 8)]))
    f32b.work(d32[:, 0:2 * n + 8].contiguous())
    g8, g32 = f8b.get_fft_data(), f32b.get_fft_data()
    assert g8 is not None and g32 is not None and np.array_equal(g8.cpu().numpy().view(np.uint32), g32.cpu().numpy().view(np.uint32))
    f8b.close(); f32b.close()
    # a misaligned base and a stride that is no multiple of 8 samples are refused
    buf = torch.zeros((B, 2 * (n + 16)), dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    fn = f8.lib.qrl_fft_process_sc8 if fmt == "sc8" else f8.lib.qrl_fft_process_cu8
    assert fn(f8.h, C.c_void_p(buf.data_ptr() + 8), n + 16, n) == QRL_ERR_ARG
    assert "aligned" in f8.lib.qrl_last_error().decode()
    assert fn(f8.h, C.c_void_p(buf.data_ptr()), n + 12, n) == QRL_ERR_ARG
    assert "stride" in f8.lib.qrl_last_error().decode()
    f8.close(); f32.close()
