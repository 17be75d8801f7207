"""The front end at every device-rate geometry, 2 .. 183 Msps, through the C ABI and bit-exact against the oracle.

qrl_demod_create accepts any device_samp_rate that is a multiple of 1e6; the decimation D = rate / 1e6 alone decides which kernel runs
(DecimStage::plan) and each kernel has its own summation contract in the oracle.  One D per kernel class, per padding residue 4 NS - D
of the pm classes, per tile choice of the matrix kernel and per class boundary (front_end_rates.py has the partition); the rates
test_gpu_parity.py already runs (2, 4, 10, 25, 64, 100) are left out.  The cheapest chain, GMSK-10k, sits behind every front end.

Kernel name reported by qrl_demod_profile_read and LDS planned per workgroup, per D:
  k_decim      3 5 6 7: k_decim<4, 44>, (832 + 301 D) * 8 = 20.0 - 29.7 KB; 115 127 129 130 183: k_decim<1, 14>, (832 + 107 D) * 8 = 105.1 - 163.3 KB
               (above 64 KiB: launch_decim raises the kernel's dynamic-LDS limit first)
  k_decim_mfma 8 13 16 21 24: 16-block tile, 30 - 73 KB; 29 32 33 48: 8-block tile, 56 - 87 KB; 53 63 65 67: 8-block tile with 512 threads,
               100 - 123 KB; 95 101 113: 4-block tile with 512 threads, 120 - 140 KB
  k_decim_pm   9 11 12 (3 phase slabs), 17 18 19 20 (5), 26 27 28 (7), 49 50 51 52 (13): 38.9 KB; 97 98 99 (25): 71.7 KB
  k_decim_plx  66 80 96 102 128: 16 KB static (28 KB with per-stream offsets)
"""
from concurrent.futures import ThreadPoolExecutor
import ctypes as C

import numpy as np
import pytest

import front_end_rates as fer
import orc
import sig
from test_gpu_parity import _compare

gpu = pytest.mark.gpu

MODEM_GMSK10K = 22
B = 3                      # streams, all different
M_OUT = 30000              # outputs per stream at 1 Msps: several tiles / segments of every kernel, the ~88-block edge region of pm / pl, and > 80 decoded bits
OFFSET = 25000.0
PS_OFFSETS = [25000.0, -18750.0, 9300.0]

RATES = {
    fer.GENERIC: [3, 5, 6, 7, 115, 127, 129, 130, 183],
    fer.M16: [8, 13, 16, 21, 24, 29, 32, 33, 48, 53, 63, 65, 67, 95, 101, 113],
    fer.PM: [9, 11, 12, 17, 18, 19, 20, 26, 27, 28, 49, 50, 51, 52, 97, 98, 99],
    fer.PL: [66, 80, 96, 102, 128],
}
CASES = [(D, False) for name in (fer.GENERIC, fer.M16, fer.PM, fer.PL) for D in RATES[name]] + [(D, True) for D in (5, 21, 18, 80, 129)]


def test_the_table_of_this_file_agrees_with_the_partition():
    for name, ds in RATES.items():
        assert [fer.front_end_class(D) for D in ds] == [name] * len(ds)
    assert fer.LAST_D in RATES[fer.GENERIC]


@pytest.fixture(scope="module")
def noise():
    """complex Gaussian noise, 0.05 per component, for the longest case; every case takes a prefix of it"""
    rng = np.random.default_rng(20183)
    return (np.float32(0.05) * rng.standard_normal((B, 2 * M_OUT * fer.LAST_D), dtype=np.float32)).view(np.complex64)


def _cuts(D, n):
    """Fixed, ragged, even-sized calls that add up to n = M_OUT * D samples:
       2 samples | 2 D | 58 D + 2 (shorter than the ~60 D edge region) | 5000 D + 6 | 10 D + 2 (the warm-up of the next call reaches through this
       call into the one before: the big call in front ends inside it) | 700 D + 2 (D // 3) + 2 | the rest, one large call"""
    c = [2, 2 * D, 58 * D + 2, 5000 * D + 6, 10 * D + 2, 700 * D + 2 * (D // 3) + 2]
    c.append(n - sum(c))
    assert all(k > 0 and k % 2 == 0 for k in c) and sum(c) == n and c[-1] > 20000 * D
    return c


def _input(noise, D, offsets):
    n = M_OUT * D
    assert n % 2 == 0
    iq = np.empty((B, n), np.complex64)
    for b in range(B):
        f = offsets[b] + 3000.0 * (b + 1) * (-1) ** b          # a tone a few kHz off the stream's carrier offset
        coarse = 0.3 * np.exp(2j * np.pi * (f * np.arange(M_OUT) / 1e6 + 0.1 * b))     # sample m D + p: phasor of m D times phasor of p
        fine = np.exp(2j * np.pi * f * np.arange(D) / (D * 1e6))
        iq[b] = noise[b, :n] + np.outer(coarse.astype(np.complex64), fine.astype(np.complex64)).reshape(n)
    return iq


def _run_cut(qrl_ctx, D, iq, cuts, offsets, per_stream):
    """iq through a GMSK-10k handle at D Msps in the given calls; returns (ports as q.collect gives them, profile_read())"""
    import torch
    import qradiolink_amd as q
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=B, max_chunk=max(cuts), device_samp_rate=D * 1000000, carrier_offset_hz=offsets[0])
    if per_stream:
        dem.set_carrier_offsets(offsets)
    dem.profile(True)
    d = torch.from_numpy(iq).cuda()
    idx = {"filtered": 0, "constellation": 1, "bits_a": 2, "bits_b": 3}
    ports = {k: [[] for _ in range(B)] for k in idx}
    s = 0
    for k in cuts:
        out = dem.process(d[:, s:s + k])        # even cuts of an even-pitched, aligned tensor: every slice is 16-byte aligned
        s += k
        cnt = out["counts"].cpu().numpy()
        for name, j in idx.items():
            host = out[name].cpu().numpy()
            for b in range(B):
                ports[name][b].append(host[b, :cnt[b, j]].copy())
    prof = dem.profile_read()
    dem.close()
    return {k: [np.concatenate(v) for v in ports[k]] for k in ports}, prof


def _same_as_oracle(out, refs):
    """what test_gpu_parity._compare asserts, against references computed beforehand"""
    for b, ref in enumerate(refs):
        for port in ("bits_a", "bits_b"):
            assert out[port][b].size == ref[port].size, (port, b, out[port][b].size, ref[port].size)
            assert np.array_equal(out[port][b], ref[port]), "%s stream %d differs" % (port, b)
        for port in ("filtered", "constellation"):
            got, want = out[port][b].view(np.float32) + np.float32(0), ref[port].view(np.float32) + np.float32(0)   # sign of an exact zero: see _compare
            assert got.size == want.size, (port, b, got.size, want.size)
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, "%s stream %d not bit-identical: %d floats, first at complex item %d of %d" % (port, b, bad.size, bad[0] // 2, got.size // 2)


@gpu
@pytest.mark.parametrize("D,per_stream", CASES)
def test_front_end_bit_exact_at_rate(qrl_ctx, noise, D, per_stream):
    offsets = PS_OFFSETS if per_stream else [OFFSET] * B
    iq = _input(noise, D, offsets)
    cuts = _cuts(D, iq.shape[1])
    with ThreadPoolExecutor(B) as pool:          # the oracle holds no state between calls; ctypes drops the GIL
        refs = list(pool.map(lambda b: orc.demod_gmsk(orc.frontend(iq[b], D * 1000000, offsets[b]), sps=1, filter_width=20000), range(B)))
    for b, ref in enumerate(refs):
        assert ref["bits_a"].size >= 80 and ref["bits_b"].size >= 80, (b, ref["bits_a"].size)
        assert ref["filtered"].size > 2000
    out, (ms, launches, kernel) = _run_cut(qrl_ctx, D, iq, cuts, offsets, per_stream)
    assert kernel == fer.front_end_class(D), (D, kernel)
    assert launches == len(cuts)
    _same_as_oracle(out, refs)


# ---- which rates create
def _create(qrl_ctx, rate):
    """qrl_demod_create for a one-stream GMSK-10k handle at `rate`: (status, handle)"""
    import qradiolink_amd as q
    cfg = q._Config()
    cfg.modem_type, cfg.use_mode_defaults = MODEM_GMSK10K, 1
    cfg.device_samp_rate, cfg.carrier_offset_hz = rate, OFFSET
    cfg.batch, cfg.max_chunk, cfg.enable_side_outputs = 1, 4096, 1
    h = C.c_void_p()
    rc = qrl_ctx.lib.qrl_demod_create(qrl_ctx.h, C.byref(cfg), C.byref(h))
    return rc, h


@gpu
def test_every_rate_up_to_the_last_creates(qrl_ctx):
    """docs/KERNELS.md promises a kernel for every D <= 128; the generic kernel's tile carries the range on to 183"""
    failed = []
    for D in range(fer.FIRST_D, fer.LAST_D + 1):
        rc, h = _create(qrl_ctx, D * 1000000)
        if rc != 0 or not h:
            failed.append((D, rc, qrl_ctx.lib.qrl_last_error().decode()))
        else:
            qrl_ctx.lib.qrl_demod_destroy(h)
    assert not failed, failed


@gpu
@pytest.mark.parametrize("D", [fer.LAST_D + 1, 200])
def test_rate_that_cannot_be_planned_is_refused_at_create(qrl_ctx, D):
    """QRL_ERR_ARG from qrl_demod_create (never a launch error from the first qrl_demod_process), no handle, and the context stays usable"""
    import torch
    import qradiolink_amd as q
    rc, h = _create(qrl_ctx, D * 1000000)
    assert rc == -1 and not h, (rc, h.value)       # QRL_ERR_ARG
    assert "front-end plan" in qrl_ctx.lib.qrl_last_error().decode()
    iq = sig.make_batch("gmsk10k", 2, nframes=1, device_rate=1000000, rx_offset_hz=1200.0, seed=31)
    dem = q.Demod(qrl_ctx, MODEM_GMSK10K, batch=2, max_chunk=iq.shape[1], carrier_offset_hz=1200.0)
    out = q.collect(dem, torch.from_numpy(iq).cuda(), iq.shape[1])
    dem.close()
    _compare(iq, out, "gmsk10k", 1000000, 1200.0)
