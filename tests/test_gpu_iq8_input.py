"""8-bit IQ (sc8, cu8) straight into the device-rate front end: qrl_demod_process_sc8 / qrl_demod_process_cu8 bit-exact against the oracle fed the
converted floats -- sc8: np.float32(v) * np.float32(scale); cu8: (np.float32(u) - np.float32(bias)) * np.float32(scale) -- per kernel class of
the front end (front_end_rates.py), in ragged calls, counts of every call included.

Input, cuts and comparison are those of test_gpu_front_end_rates.py and test_gpu_sc16_input.py (B = 3 distinct streams, M_OUT = 30000 outputs at
1 Msps, GMSK-10k behind the front end), quantised to 8 bits at 1 / 128 (amplitude 0.3 + noise -> a few tens of counts, asserted) with full-scale
codes (-128 / 127, or 0 / 255) written over fixed positions of every stream.  The cu8 codes are the sc8 codes + 128.  Every cut is a multiple of
8 samples -- an 8-bit call needs a 16-byte aligned base, so a slice of one tensor is only a valid next call behind such a cut -- except in the
case that sends calls of n = 4 and n = 2 (mod 8) down the per-output kernels; the calls behind them start off the 8-sample grid and are taken
from copies of the input shifted to a 16-byte boundary.

Kernel per D (qrl_demod_profile_read reports the same names as for cf32):
  k_decim_pm    9 (3 phase slabs), 18 (5), 25 (7, K = 1 last step), 27 (7), 50 (13), 98 100 (25): native 2-byte ring
  k_decim_mfma  8 33 65 101: per-sample staging with the conversion at the load
  k_decim       3 129;  k_decim_plx 66 128: raw words in the prefetch registers
"""
from concurrent.futures import ThreadPoolExecutor
import ctypes as C

import numpy as np
import pytest

import front_end_rates as fer
import orc
import sig
from test_gpu_front_end_rates import B, M_OUT, MODEM_GMSK10K, OFFSET, PS_OFFSETS, _cuts, _input, _same_as_oracle
from test_gpu_parity import _compare
from test_gpu_sc16_input import FULL_SCALE_AT, LAST_D, RATES

gpu = pytest.mark.gpu

QRL_ERR_ARG = -1
OPT_SC16_BASEBAND_ON = 1
SC8, CU8 = "sc8", "cu8"
SCALE = np.float32(1.0 / 128.0)
BIAS = np.float32(127.5)
CU8_RATES = [25, 50, 33, 3, 66]
CASES = ([(SC8, D, False) for name in (fer.PM, fer.M16, fer.GENERIC, fer.PL) for D in RATES[name]] + [(CU8, D, False) for D in CU8_RATES]
         + [(SC8, 18, True), (SC8, 80, True)])


def test_the_rates_of_this_file_are_the_issues():
    assert RATES == {fer.PM: [9, 18, 25, 27, 50, 98, 100], fer.M16: [8, 33, 65, 101], fer.GENERIC: [3, 129], fer.PL: [66, 128]}
    assert [fer.front_end_class(D) for D in CU8_RATES] == [fer.PM, fer.PM, fer.M16, fer.GENERIC, fer.PL]


@pytest.fixture(scope="module")
def noise():
    """the noise of test_gpu_front_end_rates.py (same generator and seed), for the longest case of this file"""
    rng = np.random.default_rng(20183)
    return (np.float32(0.05) * rng.standard_normal((B, 2 * M_OUT * LAST_D), dtype=np.float32)).view(np.complex64)


def _cuts8(D, n):
    """_cuts with every size rounded up to a multiple of 8 samples; the last call takes the rest"""
    c = [(k + 7) // 8 * 8 for k in _cuts(D, n)[:-1]]
    c.append(n - sum(c))
    assert all(k > 0 and k % 8 == 0 for k in c) and sum(c) == n and c[-1] > 20000 * D
    assert c[2] < 60 * D and c[4] < 12 * D        # still shorter than the edge region / a warm-up that reaches through the call
    return c


def quantise8(iq):
    """[B, n] complex64 -> [B, 2 n] int8 at 1 / 128, with the full-scale codes"""
    v = np.clip(np.rint(iq.view(np.float32) * np.float32(128.0)), -128, 127).astype(np.int8)
    assert 20 < np.abs(v.astype(np.int32)).max() < 120         # max |v - centre| before the full-scale codes are written
    for b in range(v.shape[0]):
        for j, p in enumerate(FULL_SCALE_AT):
            v[b, p + (b if p >= 0 else -b)] = -128 if j % 2 == 0 else 127
    return v


def as_cu8(v):
    """the unsigned codes of the same samples: u = v + 128 (full scale: 0 / 255)"""
    return (v.astype(np.int16) + 128).astype(np.uint8)


def converted(codes, fmt, scale=SCALE, bias=BIAS):
    """the contract's floats, [B, n] complex64"""
    f = codes.astype(np.float32)
    if fmt == CU8:
        f = f - np.float32(bias)
    return (f * np.float32(scale)).view(np.complex64)


def oracle_refs(x, D, offsets):
    with ThreadPoolExecutor(B) as pool:
        refs = list(pool.map(lambda b: orc.demod_gmsk(orc.frontend(x[b], D * 1000000, offsets[b]), sps=1, filter_width=20000), range(B)))
    for b, ref in enumerate(refs):        # on the oracle alone: a vacuous comparison cannot pass
        assert ref["bits_a"].size >= 80 and ref["bits_b"].size >= 80, (b, ref["bits_a"].size)
        assert ref["filtered"].size > 2000
    return refs


class _Refs:
    """codes and oracle outputs per (format, D, per_stream, scale, bias), computed once and shared by the tests that need them"""
    def __init__(self, noise):
        self.noise, self.cache = noise, {}

    def get(self, fmt, D, per_stream=False, scale=SCALE, bias=BIAS):
        key = (fmt, D, per_stream, float(scale), float(bias))
        if key not in self.cache:
            offsets = PS_OFFSETS if per_stream else [OFFSET] * B
            v = quantise8(_input(self.noise, D, offsets))
            codes = v if fmt == SC8 else as_cu8(v)
            self.cache[key] = (codes, offsets, oracle_refs(converted(codes, fmt, scale, bias), D, offsets))
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(noise):
    return _Refs(noise)


def _shifted(t, d, n, r):
    """a copy of d ([B, 2 n]) in which sample s lies at position s + 8 - r: 16-byte aligned where s = r (mod 8); pitch n + 8"""
    c = t.zeros((B, 2 * (n + 8)), dtype=d.dtype, device="cuda")
    c[:, 2 * (8 - r):2 * (8 - r) + 2 * n] = d
    return c


def _run_cut8(qrl_ctx, D, codes, fmt, cuts, offsets, per_stream, scale=None, bias=None, rotation=None):
    """codes ([B, 2 n] int8 / uint8) through a GMSK-10k handle at D Msps in the given calls.  rotation: {name: tensor-making data} of the same samples
    in the other formats -- call k is fed format k % 4 of (cf32, sc16, sc8, cu8).  Returns (ports, profile_read())"""
    import torch
    import qradiolink_amd as q
    n = codes.shape[1] // 2
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=max(cuts), device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    if per_stream:
        dem.set_carrier_offsets(offsets)
    if scale is not None:
        if fmt == SC8:
            dem.set_sc8_scale(scale)
        else:
            dem.set_cu8_scale(scale, bias)
    dem.profile(True)
    d = torch.from_numpy(codes).cuda()
    run = dem.process_sc8 if fmt == SC8 else dem.process_cu8
    starts = np.concatenate(([0], np.cumsum(cuts)[:-1]))
    copies = {int(r): _shifted(torch, d, n, int(r)) for r in sorted({int(s) % 8 for s in starts} - {0})}
    if rotation is not None:
        assert not copies
        dem.set_sc16_scale(float(SCALE))
        dem.set_cu8_scale(float(SCALE), 128.0)            # (u - 128) / 128 == v / 128 exactly: all four formats carry the same samples
        f32 = torch.from_numpy(rotation["cf32"]).cuda()
        d16 = torch.from_numpy(rotation["sc16"]).cuda()
        du8 = torch.from_numpy(rotation["cu8"]).cuda()
    idx = {"filtered": 0, "constellation": 1, "bits_a": 2, "bits_b": 3}
    ports = {k: [[] for _ in range(B)] for k in idx}
    for call, (s, k) in enumerate(zip(starts, cuts)):
        s, k = int(s), int(k)
        if rotation is not None and call % 4 == 0:
            out = dem.process(f32[:, s:s + k])
        elif rotation is not None and call % 4 == 1:
            out = dem.process_sc16(d16[:, 2 * s:2 * (s + k)])
        elif rotation is not None and call % 4 == 3:
            out = dem.process_cu8(du8[:, 2 * s:2 * (s + k)])
        elif s % 8 == 0:
            out = run(d[:, 2 * s:2 * (s + k)])
        else:
            sh = 8 - s % 8
            out = run(copies[s % 8][:, 2 * (s + sh):2 * (s + sh + k)])
        cnt = out["counts"].cpu().numpy()
        for name, j in idx.items():
            host = out[name].cpu().numpy()
            for b in range(B):
                ports[name][b].append(host[b, :cnt[b, j]].copy())
    prof = dem.profile_read()
    dem.close()
    return {k: [np.concatenate(x) for x in ports[k]] for k in ports}, prof


@gpu
@pytest.mark.parametrize("fmt,D,per_stream", CASES)
def test_iq8_front_end_bit_exact_at_rate(qrl_ctx, refs, fmt, D, per_stream):
    codes, offsets, want = refs.get(fmt, D, per_stream)
    cuts = _cuts8(D, codes.shape[1] // 2)
    out, (ms, launches, kernel) = _run_cut8(qrl_ctx, D, codes, fmt, cuts, offsets, per_stream)
    assert kernel == fer.front_end_class(D), (D, kernel)
    assert launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
@pytest.mark.parametrize("fmt", [SC8, CU8])
def test_iq8_calls_of_4_and_2_mod_8_samples_take_the_per_output_kernels(qrl_ctx, refs, fmt):
    """D = 50: the third call has n = 4 (mod 8), the fourth and the fifth n = 2 (mod 8) -- no whole 16-byte pieces per row, so not the LDS-DMA
    kernel; the fourth starts at a sample = 4 (mod 8), the fifth at 6 (mod 8); from the sixth call on the stream is back on the grid"""
    D = 50
    codes, offsets, want = refs.get(fmt, D)
    cuts = _cuts8(D, codes.shape[1] // 2)
    cuts[2] -= 4
    cuts[3] += 2
    cuts[4] += 2
    assert cuts[2] % 8 == 4 and cuts[3] % 8 == 2 and cuts[4] % 8 == 2 and sum(cuts) == codes.shape[1] // 2 and cuts[4] < 12 * D
    assert [int(s) % 8 for s in np.cumsum(cuts)[:-1]] == [0, 0, 4, 6, 0, 0]
    out, (ms, launches, kernel) = _run_cut8(qrl_ctx, D, codes, fmt, cuts, offsets, False)
    assert kernel == fer.PM and launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
def test_cu8_scale_and_bias_that_make_the_multiply_round(qrl_ctx, refs):
    """D = 25 with set_cu8_scale(1 / 127, 127.4f): the subtract gives fractions and the multiply rounds"""
    D, scale, bias = 25, np.float32(1.0 / 127.0), np.float32(127.4)
    codes, offsets, want = refs.get(CU8, D, False, scale, bias)
    x = codes[:, :4096].astype(np.float32) - bias
    assert np.any((x * scale).astype(np.float64) != x.astype(np.float64) * float(scale))      # the products of this input are not all exact
    cuts = _cuts8(D, codes.shape[1] // 2)
    out, (ms, launches, kernel) = _run_cut8(qrl_ctx, D, codes, CU8, cuts, offsets, False, scale=float(scale), bias=float(bias))
    assert kernel == fer.PM and launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
def test_cf32_sc16_sc8_and_cu8_calls_in_rotation_on_one_handle(qrl_ctx, refs):
    """D = 50: call k is fed format k % 4 of (cf32, sc16, sc8, cu8), each carrying the same samples (int16 at scale 1 / 128, cu8 = v + 128 with
    bias 128) = the all-sc8 run = the oracle"""
    D = 50
    codes, offsets, want = refs.get(SC8, D)
    cuts = _cuts8(D, codes.shape[1] // 2)
    rotation = {"cf32": converted(codes, SC8), "sc16": codes.astype(np.int16), "cu8": as_cu8(codes)}
    assert np.array_equal(converted(rotation["cu8"], CU8, SCALE, 128.0).view(np.uint32), rotation["cf32"].view(np.uint32))
    mixed, (ms, launches, kernel) = _run_cut8(qrl_ctx, D, codes, SC8, cuts, offsets, False, rotation=rotation)
    assert kernel == fer.PM and launches == len(cuts) and len(cuts) >= 4
    plain, _ = _run_cut8(qrl_ctx, D, codes, SC8, cuts, offsets, False)
    for port in mixed:
        for b in range(B):
            assert np.array_equal(mixed[port][b].view(np.uint8), plain[port][b].view(np.uint8)), (port, b)
    _same_as_oracle(mixed, want)


@gpu
def test_iq8_is_refused_by_a_1_msps_handle_which_stays_usable(qrl_ctx):
    import torch
    import qradiolink_amd as q
    iq = sig.make_batch("gmsk10k", 2, nframes=1, device_rate=1000000, rx_offset_hz=1200.0, seed=31)
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=2, max_chunk=iq.shape[1], carrier_offset_hz=1200.0)
    v = torch.zeros((2, 2 * 4096), dtype=torch.int8, device="cuda")
    u = torch.zeros((2, 2 * 4096), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    host, cnt = np.zeros((2, 2 * 4096), np.int8), np.zeros((2, 4), np.uint32)
    for baseband in (False, True):
        dem.enable_sc16_baseband(baseband)
        for name, t in (("qrl_demod_process_sc8", v), ("qrl_demod_process_cu8", u)):
            rc = getattr(dem.lib, name)(dem.h, t.data_ptr(), 4096, 4096, C.byref(dem._out))
            assert rc == QRL_ERR_ARG
            err = dem.lib.qrl_last_error().decode()
            assert "1 Msps" in err and "front end" in err and name in err, err
            assert getattr(dem.lib, name + "_host")(dem.h, host.ctypes.data, 4096, 4096, None, None, 0, cnt.ctypes.data) == QRL_ERR_ARG
            assert "1 Msps" in dem.lib.qrl_last_error().decode()
        with pytest.raises(q.QrlError):
            dem.process_sc8(v)
        with pytest.raises(q.QrlError):
            dem.process_cu8(u)
    dem.enable_sc16_baseband(False)
    out = q.collect(dem, torch.from_numpy(iq).cuda(), iq.shape[1])          # nothing changed: the stream starts at its first sample
    dem.close()
    _compare(iq, out, "gmsk10k", 1000000, 1200.0)


@gpu
def test_iq8_stride_alignment_and_setters_are_checked_before_anything_is_launched(qrl_ctx, refs):
    """a stride of 4 (mod 8) samples and a base 8 bytes off a valid allocation are QRL_ERR_ARG, each with its own text; bad setter values are
    refused; the handle has not moved"""
    import torch
    import qradiolink_amd as q
    D = 9
    codes, offsets, want = refs.get(SC8, D)
    n = codes.shape[1] // 2
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=n, device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    d = torch.from_numpy(codes).cuda()
    torch.cuda.current_stream().synchronize()
    assert d.data_ptr() % 16 == 0 and n % 8 == 0
    for name in ("qrl_demod_process_sc8", "qrl_demod_process_cu8"):
        fn = getattr(dem.lib, name)
        assert fn(dem.h, d.data_ptr(), n - 4, 1024, C.byref(dem._out)) == QRL_ERR_ARG       # stride = 4 (mod 8)
        err = dem.lib.qrl_last_error().decode()
        assert "stride" in err and "aligned" not in err and name in err, err
        assert fn(dem.h, d.data_ptr() + 8, n, 1024, C.byref(dem._out)) == QRL_ERR_ARG       # pointer arithmetic only: nothing reads it
        err = dem.lib.qrl_last_error().decode()
        assert "aligned" in err and "stride" not in err and name in err, err
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(q.QrlError):
            dem.set_sc8_scale(bad)
        with pytest.raises(q.QrlError):
            dem.set_cu8_scale(bad, 127.5)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(q.QrlError):
            dem.set_cu8_scale(1.0 / 128.0, bad)
    out = dem.process_sc8(d)
    cnt = out["counts"].cpu().numpy()
    got = {name: [out[name].cpu().numpy()[b, :cnt[b, j]] for b in range(B)] for name, j in (("filtered", 0), ("constellation", 1), ("bits_a", 2), ("bits_b", 3))}
    dem.close()
    _same_as_oracle(got, want)


@gpu
@pytest.mark.parametrize("fmt", [SC8, CU8])
def test_iq8_host_entry_points_upload_2_byte_samples(qrl_ctx, refs, fmt):
    """qrl_demod_process_sc8_host / _cu8_host, D = 9 (25 for cu8), the stream in two calls whose lengths are no multiples of 8: the device pitch
    is rounded up to 8 samples, the rows are uploaded as 2-byte samples from a host pitch of n, and the bits of the two calls together are the
    oracle's"""
    import qradiolink_amd as q
    D = 9 if fmt == SC8 else 25
    codes, offsets, want = refs.get(fmt, D)
    n = codes.shape[1] // 2
    n1 = (n // 2) // 8 * 8 + (2 if fmt == SC8 else 5)
    assert n1 % 8 and (n - n1) % 8
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=n, device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    fn = dem.lib.qrl_demod_process_sc8_host if fmt == SC8 else dem.lib.qrl_demod_process_cu8_host
    cap = dem.caps[2]
    got_a, got_b = [[] for _ in range(B)], [[] for _ in range(B)]
    for start, count in ((0, n1), (n1, n - n1)):
        a, b_, cnt = np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), np.zeros((B, 4), np.uint32)
        rc = fn(dem.h, codes.ctypes.data + 2 * start, n, count, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data)
        assert rc == 0, dem.lib.qrl_last_error().decode()
        for s in range(B):
            got_a[s].append(a[s, :cnt[s, 2]].copy())
            got_b[s].append(b_[s, :cnt[s, 3]].copy())
    dem.close()
    for s in range(B):
        assert np.array_equal(np.concatenate(got_a[s]), want[s]["bits_a"]), "bits A stream %d" % s
        assert np.array_equal(np.concatenate(got_b[s]), want[s]["bits_b"]), "bits B stream %d" % s
