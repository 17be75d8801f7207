"""16-bit integer IQ (sc16) straight into the device-rate front end: qrl_demod_process_sc16 bit-exact against the oracle fed the converted
floats np.float32(v) * np.float32(scale), per kernel class of the front end (front_end_rates.py), in ragged calls.

Input, cuts and comparison are those of test_gpu_front_end_rates.py (B = 3 distinct streams, M_OUT = 30000 outputs at 1 Msps, GMSK-10k behind
the front end), quantised to int16 at scale 1 / 32768 (amplitude 0.3 -> about +-9 800 counts) with a handful of full-scale samples
(-32768, 32767) written over fixed positions of every stream.  Every cut is a multiple of 4 samples -- an sc16 call needs a 16-byte aligned
base, so a slice of one tensor is only a valid next call behind such a cut -- except in the one case that sends a call of n = 2 (mod 4)
down the per-output kernels; the call behind it starts at a sample = 2 (mod 4) and is taken from a copy of the input shifted by two samples.

Kernel per D (qrl_demod_profile_read reports the same names as for cf32):
  k_decim_pm    9 (3 phase slabs), 18 (5), 25 (7, K = 1 last step), 27 (7), 50 (13), 98 100 (25): native 4-byte ring
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

gpu = pytest.mark.gpu

QRL_ERR_ARG = -1
SCALE = np.float32(1.0 / 32768.0)
RATES = {
    fer.PM: [9, 18, 25, 27, 50, 98, 100],
    fer.M16: [8, 33, 65, 101],
    fer.GENERIC: [3, 129],
    fer.PL: [66, 128],
}
LAST_D = 129
CASES = [(D, False) for name in (fer.PM, fer.M16, fer.GENERIC, fer.PL) for D in RATES[name]] + [(18, True), (80, True)]
FULL_SCALE_AT = (5, 6, 4001, 4002, 120001, -3)          # int16 positions of every stream (shifted by the stream index) set to -32768 / 32767


def test_the_table_of_this_file_agrees_with_the_partition():
    for name, ds in RATES.items():
        assert [fer.front_end_class(D) for D in ds] == [name] * len(ds)


@pytest.fixture(scope="module")
def noise():
    """the noise of test_gpu_front_end_rates.py (same generator and seed), for the longest case of this file"""
    rng = np.random.default_rng(20183)
    return (np.float32(0.05) * rng.standard_normal((B, 2 * M_OUT * LAST_D), dtype=np.float32)).view(np.complex64)


def _cuts4(D, n):
    """_cuts with every size rounded up to a multiple of 4 samples; the last call takes the rest"""
    c = [(k + 3) // 4 * 4 for k in _cuts(D, n)[:-1]]
    c.append(n - sum(c))
    assert all(k > 0 and k % 4 == 0 for k in c) and sum(c) == n and c[-1] > 20000 * D
    assert c[2] < 60 * D and c[4] < 12 * D        # still shorter than the edge region / a warm-up that reaches through the call
    return c


def _quantise(iq):
    """[B, n] complex64 -> [B, 2 n] int16 at 1 / 32768, with the full-scale samples"""
    v = np.clip(np.rint(iq.view(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)
    assert 8000 < np.abs(v).max() < 32000
    for b in range(v.shape[0]):
        for j, p in enumerate(FULL_SCALE_AT):
            v[b, p + (b if p >= 0 else -b)] = -32768 if j % 2 == 0 else 32767
    return v


def _converted(v, scale):
    return (v.astype(np.float32) * np.float32(scale)).view(np.complex64)


class _Refs:
    """oracle outputs per (D, per_stream, scale), computed once and shared by the tests that need them"""
    def __init__(self, noise):
        self.noise, self.cache = noise, {}

    def get(self, D, per_stream=False, scale=SCALE):
        key = (D, per_stream, float(scale))
        if key not in self.cache:
            offsets = PS_OFFSETS if per_stream else [OFFSET] * B
            v = _quantise(_input(self.noise, D, offsets))
            x = _converted(v, scale)
            with ThreadPoolExecutor(B) as pool:
                refs = list(pool.map(lambda b: orc.demod_gmsk(orc.frontend(x[b], D * 1000000, offsets[b]), sps=1, filter_width=20000), range(B)))
            for b, ref in enumerate(refs):        # on the oracle alone: a vacuous comparison cannot pass
                assert ref["bits_a"].size >= 80 and ref["bits_b"].size >= 80, (b, ref["bits_a"].size)
                assert ref["filtered"].size > 2000
            self.cache[key] = (v, offsets, refs)
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(noise):
    return _Refs(noise)


def _run_cut16(qrl_ctx, D, v, cuts, offsets, per_stream, scale=None, mixed=False):
    """v ([B, 2 n] int16) through a GMSK-10k handle at D Msps in the given calls; mixed: every second call is fed the converted floats through
    qrl_demod_process instead.  Returns (ports, profile_read())"""
    import torch
    import qradiolink_amd as q
    n = v.shape[1] // 2
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=max(cuts), device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    if per_stream:
        dem.set_carrier_offsets(offsets)
    if scale is not None:
        dem.set_sc16_scale(scale)
    dem.profile(True)
    d = torch.from_numpy(v).cuda()
    starts = np.concatenate(([0], np.cumsum(cuts)[:-1]))
    assert all(s % 4 in (0, 2) for s in starts)
    d2 = None
    if any(s % 4 == 2 for s in starts):            # sample s at position s + 2: aligned where s = 2 (mod 4); pitch n + 4
        d2 = torch.zeros((B, 2 * (n + 4)), dtype=torch.int16, device="cuda")
        d2[:, 4:4 + 2 * n] = d
    f = torch.from_numpy(_converted(v, SCALE if scale is None else scale)).cuda() if mixed else None
    idx = {"filtered": 0, "constellation": 1, "bits_a": 2, "bits_b": 3}
    ports = {k: [[] for _ in range(B)] for k in idx}
    for call, (s, k) in enumerate(zip(starts, cuts)):
        s, k = int(s), int(k)
        if mixed and call % 2 == 1:
            out = dem.process(f[:, s:s + k])
        elif s % 4 == 0:
            out = dem.process_sc16(d[:, 2 * s:2 * (s + k)])
        else:
            out = dem.process_sc16(d2[:, 2 * (s + 2):2 * (s + 2 + k)])
        cnt = out["counts"].cpu().numpy()
        for name, j in idx.items():
            host = out[name].cpu().numpy()
            for b in range(B):
                ports[name][b].append(host[b, :cnt[b, j]].copy())
    prof = dem.profile_read()
    dem.close()
    return {k: [np.concatenate(x) for x in ports[k]] for k in ports}, prof


@gpu
@pytest.mark.parametrize("D,per_stream", CASES)
def test_sc16_front_end_bit_exact_at_rate(qrl_ctx, refs, D, per_stream):
    v, offsets, want = refs.get(D, per_stream)
    cuts = _cuts4(D, v.shape[1] // 2)
    out, (ms, launches, kernel) = _run_cut16(qrl_ctx, D, v, cuts, offsets, per_stream)
    assert kernel == fer.front_end_class(D), (D, kernel)
    assert launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
def test_sc16_call_of_2_mod_4_samples_takes_the_per_output_kernels(qrl_ctx, refs):
    """D = 50: the third call has n = 2 (mod 4) -- no whole 16-byte pieces per row, so not the LDS-DMA kernel -- and so has the fourth, which
    also starts at a sample = 2 (mod 4); from the fifth call on the stream is back on the grid"""
    D = 50
    v, offsets, want = refs.get(D)
    cuts = _cuts4(D, v.shape[1] // 2)
    cuts[2] -= 2
    cuts[3] += 2
    assert cuts[2] % 4 == 2 and cuts[3] % 4 == 2 and sum(cuts) == v.shape[1] // 2
    out, (ms, launches, kernel) = _run_cut16(qrl_ctx, D, v, cuts, offsets, False)
    assert kernel == fer.PM and launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
def test_sc16_scale_that_is_no_power_of_two(qrl_ctx, refs):
    """D = 25 with set_sc16_scale(1 / 32767): the multiply rounds"""
    D, scale = 25, np.float32(1.0 / 32767.0)
    v, offsets, want = refs.get(D, False, scale)
    x = v[:, :4096].astype(np.float32)
    assert np.any(x * scale != (x.astype(np.float64) * float(scale)))      # the products of this input are not all exact
    cuts = _cuts4(D, v.shape[1] // 2)
    out, (ms, launches, kernel) = _run_cut16(qrl_ctx, D, v, cuts, offsets, False, scale=float(scale))
    assert kernel == fer.PM and launches == len(cuts)
    _same_as_oracle(out, want)


@gpu
def test_sc16_and_cf32_calls_alternate_on_one_handle(qrl_ctx, refs):
    """D = 50: process_sc16(v) and process(converted floats of the same samples) call by call = the all-sc16 run = the oracle"""
    D = 50
    v, offsets, want = refs.get(D)
    cuts = _cuts4(D, v.shape[1] // 2)
    mixed, (ms, launches, kernel) = _run_cut16(qrl_ctx, D, v, cuts, offsets, False, mixed=True)
    assert kernel == fer.PM and launches == len(cuts)
    plain, _ = _run_cut16(qrl_ctx, D, v, cuts, offsets, False)
    for port in mixed:
        for b in range(B):
            assert np.array_equal(mixed[port][b].view(np.uint8), plain[port][b].view(np.uint8)), (port, b)
    _same_as_oracle(mixed, want)


@gpu
def test_sc16_is_refused_by_a_1_msps_handle_which_stays_usable(qrl_ctx):
    import torch
    import qradiolink_amd as q
    iq = sig.make_batch("gmsk10k", 2, nframes=1, device_rate=1000000, rx_offset_hz=1200.0, seed=31)
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=2, max_chunk=iq.shape[1], carrier_offset_hz=1200.0)
    v = torch.zeros((2, 2 * 4096), dtype=torch.int16, device="cuda")
    torch.cuda.current_stream().synchronize()
    rc = dem.lib.qrl_demod_process_sc16(dem.h, v.data_ptr(), 4096, 4096, C.byref(dem._out))
    assert rc == QRL_ERR_ARG
    err = dem.lib.qrl_last_error().decode()
    assert "1 Msps" in err and "front end" in err, err
    with pytest.raises(q.QrlError):
        dem.process_sc16(v)
    host, cnt = np.zeros((2, 2 * 4096), np.int16), np.zeros((2, 4), np.uint32)
    assert dem.lib.qrl_demod_process_sc16_host(dem.h, host.ctypes.data, 4096, 4096, None, None, 0, cnt.ctypes.data) == QRL_ERR_ARG
    assert "1 Msps" in dem.lib.qrl_last_error().decode()
    out = q.collect(dem, torch.from_numpy(iq).cuda(), iq.shape[1])          # nothing changed: the stream starts at its first sample
    dem.close()
    _compare(iq, out, "gmsk10k", 1000000, 1200.0)


@gpu
def test_sc16_stride_and_alignment_are_checked_before_anything_is_launched(qrl_ctx, refs):
    """a stride that is no multiple of 4 samples and a base 8 bytes off a valid allocation are QRL_ERR_ARG; the handle has not moved"""
    import torch
    import qradiolink_amd as q
    D = 9
    v, offsets, want = refs.get(D)
    n = v.shape[1] // 2
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=n, device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    d = torch.from_numpy(v).cuda()
    torch.cuda.current_stream().synchronize()
    assert d.data_ptr() % 16 == 0
    fn = dem.lib.qrl_demod_process_sc16
    assert fn(dem.h, d.data_ptr(), n - 2, 1024, C.byref(dem._out)) == QRL_ERR_ARG       # stride = 2 (mod 4)
    assert "stride" in dem.lib.qrl_last_error().decode()
    assert fn(dem.h, d.data_ptr() + 8, n, 1024, C.byref(dem._out)) == QRL_ERR_ARG       # pointer arithmetic only: nothing reads it
    assert "aligned" in dem.lib.qrl_last_error().decode()
    with pytest.raises(q.QrlError):
        dem.set_sc16_scale(0.0)
    with pytest.raises(q.QrlError):
        dem.set_sc16_scale(float("inf"))
    out = dem.process_sc16(d)
    cnt = out["counts"].cpu().numpy()
    got = {name: [out[name].cpu().numpy()[b, :cnt[b, j]] for b in range(B)] for name, j in (("filtered", 0), ("constellation", 1), ("bits_a", 2), ("bits_b", 3))}
    dem.close()
    _same_as_oracle(got, want)


@gpu
def test_sc16_host_entry_point_uploads_4_byte_samples(qrl_ctx, refs):
    """qrl_demod_process_sc16_host, D = 9, the stream in two calls whose lengths are 2 (mod 4): the device pitch is rounded up to 4 samples, the
    rows are uploaded as 4-byte samples from a host pitch of n, and the bits of the two calls together are the oracle's"""
    import qradiolink_amd as q
    D = 9
    v, offsets, want = refs.get(D)
    n = v.shape[1] // 2
    n1 = (n // 2) // 4 * 4 + 2
    assert n1 % 4 == 2 and (n - n1) % 4 == 2
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=n, device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    cap = dem.caps[2]
    got_a, got_b = [[] for _ in range(B)], [[] for _ in range(B)]
    for start, count in ((0, n1), (n1, n - n1)):
        a, b_, cnt = np.zeros((B, cap), np.uint8), np.zeros((B, cap), np.uint8), np.zeros((B, 4), np.uint32)
        rc = dem.lib.qrl_demod_process_sc16_host(dem.h, v.ctypes.data + 4 * start, n, count, a.ctypes.data, b_.ctypes.data, cap, cnt.ctypes.data)
        assert rc == 0, dem.lib.qrl_last_error().decode()
        for s in range(B):
            got_a[s].append(a[s, :cnt[s, 2]].copy())
            got_b[s].append(b_[s, :cnt[s, 3]].copy())
    dem.close()
    for s in range(B):
        assert np.array_equal(np.concatenate(got_a[s]), want[s]["bits_a"]), "bits A stream %d" % s
        assert np.array_equal(np.concatenate(got_b[s]), want[s]["bits_b"]), "bits B stream %d" % s
