"""int16 IQ (sc16) into the wideband receivers: qrl_chan_process_sc16 / qrl_chan_channelize_sc16 give, bit for bit, what the cf32 entry points
compute when fed (float)v * scale -- held here to the oracle on those converted floats (int16 channel samples and 4FSK dibits array_equal; the
RSSI tags to the 1e-4 dB of tests/test_gpu_chan.py, log10f against libm, and array_equal to a cf32 handle on the same floats).  Streaming kernel
(LDS-DMA of raw pairs, converted on landing), general-M kernel, forms 1 and 2, single carrier, alternating formats, scale, refusals, channelize.
Every input carries -32768, 32767, 0 and +-1 at its head, in its middle and at its tail."""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_chan import _wideband, _wideband_xl

pytestmark = pytest.mark.gpu

QRL_ERR_ARG = -1
EDGE = np.array([-32768, 32767, 0, 1, -1, -32768, 32767, 1, 0, -1], np.int16)   # five I, Q pairs
CUTS1 = [[64 * 2500], [64 * 31, 64 * 1200, 64 * 1269]]


def _quantise(iq, peak=30000.0, edge=EDGE):
    """complex64 [B, n] -> int16 [B, 2 n], peak near +-peak, with the edge values planted"""
    f = np.ascontiguousarray(iq).view(np.float32).reshape(iq.shape[0], -1)
    v = np.rint(f * np.float32(peak / np.abs(f).max())).astype(np.int16)
    n2 = v.shape[1]
    for at in (0, (n2 // 4) * 2 + 6, n2 - edge.size):
        v[:, at:at + edge.size] = edge
    return v


def _floats(v, scale=1.0 / 32768.0):
    """what the sc16 entry points are defined by: one exact conversion, one rounded f32 multiply"""
    return np.ascontiguousarray(v.astype(np.float32) * np.float32(scale)).view(np.complex64)


def _dev16(v):
    """int16 [B, 2 n] host -> cuda view [B, 2 n] of a buffer whose row pitch is a multiple of 4 samples (16-byte rows), as the ABI demands"""
    import torch
    B, n2 = v.shape
    pitch = (n2 // 2 + 3) // 4 * 4
    buf = torch.zeros((B, 2 * pitch), dtype=torch.int16, device="cuda")
    buf[:, :n2] = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return buf[:, :n2]


def _dev32(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class _Collect:
    """int16 samples, RSSI tags and dibits of every (stream, channel), call by call"""

    def __init__(self, ch, fsk):
        self.ch, self.fsk = ch, fsk
        B, cc = ch.batch, ch.cc
        self.s = [[[] for _ in range(cc)] for _ in range(B)]
        self.t = [[[] for _ in range(cc)] for _ in range(B)]
        self.d = [[[] for _ in range(cc)] for _ in range(B)]

    def take(self):
        ch = self.ch
        cnt, o = ch.counts.cpu().numpy(), ch.out.cpu().numpy()
        rc, r = ch.rssi_counts.cpu().numpy(), ch.rssi.cpu().numpy()
        if self.fsk:
            fc, bits = ch.fsk_counts.cpu().numpy(), ch.dibits.cpu().numpy()
        for b in range(ch.batch):
            for c in range(ch.cc):
                self.s[b][c].append(o[b, c, :cnt[b, c]].copy())
                self.t[b][c].append(r[b, c, :rc[b, c]].copy())
                if self.fsk:
                    self.d[b][c].append(bits[b, c, :fc[b, c, 2]].copy())

    def samples(self, b, c):
        return np.concatenate(self.s[b][c])

    def tags(self, b, c):
        return np.concatenate(self.t[b][c])

    def dibits(self, b, c):
        return np.concatenate(self.d[b][c])


def _feed(ch, v, cuts, fmts, fsk=False):
    """the stream v (int16 [B, 2 n]) through handle ch, cut into calls; fmts[k] = 'sc16' | 'cf32' (the converted floats) for call k"""
    col = _Collect(ch, fsk)
    x = _floats(v)
    pos = 0
    for k, cut in enumerate(cuts):
        if fmts[k % len(fmts)] == "sc16":
            ch.process_sc16(_dev16(v[:, 2 * pos:2 * (pos + cut)]))
        else:
            ch.process(_dev32(x[:, pos:pos + cut]))
        col.take()
        pos += cut
    return col


# ---- the shared M = 64 stream set: four distinct streams, 64 * 2500 samples, and the oracle's answer on their converted floats (computed once)
M64, N64, CAL64 = 64, 64 * 2500, -7.25
_cache = {}


def _set64():
    if "v" not in _cache:
        import sig
        iq = _wideband(M64, N64, seed=1664, nstreams=4)
        fs = 25000.0 * M64
        t = np.arange(N64)
        for c, seed in ((3, 5), (33, 6), (62, 7)):     # DMR-like 4FSK carriers on stream 0, bin 32 (the VALU bin) next to one of them
            x, _ = sig.make_4fsk(nsym=int(N64 / fs * 4800) - 2, seed=seed, amp=0.4, noise=0.0, fs=fs)
            f0 = c * 25000.0 if c <= M64 // 2 else (c - M64) * 25000.0
            m = min(N64, x.size)
            iq[0, :m] += (x[:m] * np.exp(2j * np.pi * f0 * t[:m] / fs)).astype(np.complex64)
        v = _quantise(iq)
        x = _floats(v)
        _cache["v"] = v
        _cache["ref"] = [orc.demod_mmdvm_multi_full(x[b], M64, cal=CAL64) for b in range(4)]
        assert np.abs(_cache["ref"][0][0]).max() > 1000
    return _cache["v"], _cache["ref"]


def _check64(col, rows, streams, ref, fsk=True, channels=None):
    channels = range(M64) if channels is None else channels
    for b, st in zip(rows, streams):
        s_ref, r_ref, d_ref = ref[st]
        for k, c in enumerate(channels):
            g = col.samples(b, k)
            assert g.size == s_ref.shape[1] and np.array_equal(g, s_ref[c]), (b, c)
            tg = col.tags(b, k)
            assert tg.size == r_ref[c].size and np.allclose(tg, r_ref[c], rtol=0, atol=1e-4), (b, c)
            if fsk:
                dd = col.dibits(b, k)
                assert dd.size == d_ref[c].size and np.array_equal(dd, d_ref[c]), (b, c)


@pytest.mark.parametrize("cuts", CUTS1)
def test_streaming_kernel_sc16_bit_exact(qrl_ctx, cuts):
    """1. M = 64, batch 2, RSSI and 4FSK tail on, one call and ragged cuts (31 instants: under one segment): k_pfb_stream64's sc16 instantiation"""
    import qradiolink_amd as q
    v, ref = _set64()
    chs = []
    for _ in range(2):
        ch = q.Channelizer(qrl_ctx, M64, batch=2, max_chunk=max(cuts))
        ch.calibrate_rssi(CAL64)
        ch.enable_4fsk()
        chs.append(ch)
    chs[0].profile(True)
    col = _feed(chs[0], v[:2], cuts, ["sc16"], fsk=True)
    ms, launches, name = chs[0].profile_read()
    assert name == "k_pfb_stream64" and launches == len(cuts)
    _check64(col, (0, 1), (0, 1), ref)
    # the RSSI tags, which the oracle holds to 1e-4 dB only: bit for bit those of a cf32 handle fed the converted floats
    col32 = _feed(chs[1], v[:2], cuts, ["cf32"], fsk=True)
    for b in range(2):
        for c in range(M64):
            assert np.array_equal(col.tags(b, c), col32.tags(b, c)), (b, c)
    for ch in chs:
        ch.close()


def test_streaming_kernel_sc16_ring_walked_all_the_way_round(qrl_ctx):
    """2. batch 32 (row b = stream b % 4): few segments per stream, so a segment has more tiles than the ring has room for (68 blocks / 16 per
    tile): every ring position and both staging slots are reused with live data around them"""
    import torch
    import qradiolink_amd as q
    v, ref = _set64()
    B = 32
    # the launch rule of launch_pfb_chan: three workgroups per CU, segments of whole 16-instant tiles, at least 4 tiles each
    slots = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    m_count = N64 // 64
    nseg = min(max(1, slots // B), (m_count + 63) // 64)
    seg_len = ((m_count + nseg - 1) // nseg + 15) // 16 * 16
    assert seg_len // 16 >= 6, "segments of %d tiles do not walk the ring round" % (seg_len // 16)
    ch = q.Channelizer(qrl_ctx, M64, batch=B, max_chunk=N64)
    ch.calibrate_rssi(CAL64)
    ch.profile(True)
    col = _feed(ch, v[np.arange(B) % 4], [N64], ["sc16"])
    assert ch.profile_read()[2] == "k_pfb_stream64"
    _check64(col, range(B), [b % 4 for b in range(B)], ref, fsk=False)
    ch.close()


def test_general_m_kernel_sc16_m10_ragged_cuts(qrl_ctx):
    """3a. M = 10 (k_pfb_chan<0>), calls of 1000, 333 and 25 instants up to 60 000 samples"""
    import qradiolink_amd as q
    M, n = 10, 60000
    v = _quantise(_wideband(M, n, seed=310, nstreams=2))
    x = _floats(v)
    cuts = []
    while sum(cuts) < n:
        cuts.append(min((10 * 1000, 10 * 333, 10 * 25)[len(cuts) % 3], n - sum(cuts)))
    ch = q.Channelizer(qrl_ctx, M, batch=2, max_chunk=max(cuts))
    col = _feed(ch, v, cuts, ["sc16"])
    ch.close()
    for b in range(2):
        ref = orc.demod_mmdvm_multi(x[b], M)
        for c in range(M):
            g = col.samples(b, c)
            assert g.size == ref.shape[1] and np.array_equal(g, ref[c]), (b, c)
    assert np.abs(ref).max() > 1000


@pytest.mark.parametrize("option", ["legacy_pfb", "legacy_tail", "channel_range"])
def test_general_m_kernel_sc16_m64_options(qrl_ctx, option):
    """3b. M = 64 on the general-M kernel (QRL_CHAN_OPT_LEGACY_PFB = 1: k_pfb_chan<16>), with the separate per-channel kernels
    (QRL_CHAN_OPT_LEGACY_TAIL = 1), and a channel range (channel_first = 3, channel_count = 4) on the streaming kernel; fresh handles"""
    import qradiolink_amd as q
    v, ref = _set64()
    cuts = [64 * 777, 64 * 1723]
    rng = (3, 4) if option == "channel_range" else (0, 0)
    ch = q.Channelizer(qrl_ctx, M64, batch=2, max_chunk=max(cuts), channel_first=rng[0], channel_count=rng[1])
    ch.calibrate_rssi(CAL64)
    if option == "legacy_pfb":
        ch.set_option(q.CHAN_OPT_LEGACY_PFB, 1)
    if option == "legacy_tail":
        ch.set_option(q.CHAN_OPT_LEGACY_TAIL, 1)
    ch.enable_4fsk()
    ch.profile(True)
    col = _feed(ch, v[:2], cuts, ["sc16"], fsk=True)
    assert ch.profile_read()[2] == ("k_pfb_chan" if option == "legacy_pfb" else "k_pfb_stream64")
    _check64(col, (0, 1), (0, 1), ref, channels=range(3, 7) if option == "channel_range" else None)
    ch.close()


def test_form_1_sc16_bit_exact(qrl_ctx):
    """4a. form 1 (legacy freq-xlating receiver): (N, D, chunk) = (7, 10, 10002), k_decim_mfma's sc16 fetch and k_hist_sc16"""
    import qradiolink_amd as q
    N, D, chunk, n = 7, 10, 10002, 48000
    v = _quantise(_wideband_xl(24000.0 * D, n, seed=417, nstreams=2, offsets=[0.0, 25000.0, -50000.0, 75000.0]))
    cuts = [min(chunk, n - s) & ~1 for s in range(0, n, chunk)]
    used = sum(cuts)
    ch = q.Channelizer(qrl_ctx, N, batch=2, max_chunk=chunk, form=1, decimation=D)
    ch.calibrate_rssi(1.5)
    # (the calls are consecutive: a cut that lost a sample to the even rule would shift the stream, as in tests/test_gpu_chan.py the last one only can)
    assert all(c == chunk for c in cuts[:-1])
    col = _feed(ch, v[:, :2 * used], cuts, ["sc16"])
    ch.close()
    x = _floats(v[:, :2 * used])
    for b in range(2):
        ref, rref = orc.demod_mmdvm_xlating(x[b], N, D=D, cal=1.5)
        for c in range(N):
            g = col.samples(b, c)
            assert g.size == ref.shape[1] and np.array_equal(g, ref[c]), (b, c)
            tg = col.tags(b, c)
            assert tg.size == rref[c].size and np.allclose(tg, rref[c], rtol=0, atol=1e-4)
    assert np.abs(ref).max() > 1000


def test_form_2_sc16_bit_exact(qrl_ctx):
    """4b. form 2 (64 freq-xlating FIR decimators 1:64 + the per-channel chain + 4FSK tail), chunk = 64 * 625 + 2"""
    import qradiolink_amd as q
    v, _ = _set64()
    N, chunk = 64, 64 * 625 + 2
    cuts = [min(chunk, N64 - s) & ~1 for s in range(0, N64, chunk)]
    used = sum(cuts)
    ch = q.Channelizer(qrl_ctx, N, batch=2, max_chunk=chunk, form=2)
    ch.calibrate_rssi(-3.0)
    ch.enable_4fsk()
    ch.profile(True)
    col = _feed(ch, v[:2, :2 * used], cuts, ["sc16"], fsk=True)
    assert ch.profile_read()[2].startswith("k_decim_mfma")
    ch.close()
    x = _floats(v[:2, :2 * used])
    for b in range(2):
        ref, rref, dref = orc.demod_mmdvm_xlating_bank_4fsk(x[b], N, cal=-3.0)
        for c in range(N):
            g = col.samples(b, c)
            assert g.size == ref.shape[1] and np.array_equal(g, ref[c]), (b, c)
            tg = col.tags(b, c)
            assert tg.size == rref[c].size and np.allclose(tg, rref[c], rtol=0, atol=1e-4)
            dd = col.dibits(b, c)
            assert dd.size == dref[c].size and np.array_equal(dd, dref[c]), (b, c)
    assert np.abs(ref).max() > 1000


def test_single_carrier_sc16_bit_exact(qrl_ctx):
    """5. num_channels = 1 (gr_demod_mmdvm: k_resamp reads the caller's buffer), calls of 33333 samples (odd)"""
    import qradiolink_amd as q
    rng = np.random.default_rng(55)
    n, fs, chunk = 125000, 250000.0, 33333
    t = np.arange(n)
    iq = []
    for s in range(2):
        dev, fm = rng.uniform(1000, 4000), rng.uniform(200, 1500)
        ph = (dev / fm) * np.sin(2 * np.pi * fm * t / fs + rng.uniform(0, 6)) + 2 * np.pi * rng.uniform(-500, 500) * t / fs
        iq.append((0.2 * np.exp(1j * ph) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
    v = _quantise(np.stack(iq))
    x = _floats(v)
    cuts = [min(chunk, n - s) for s in range(0, n, chunk)]
    ch = q.Channelizer(qrl_ctx, 1, batch=2, max_chunk=chunk)
    ch.calibrate_rssi(2.0)
    ch.profile(True)
    col = _feed(ch, v, cuts, ["sc16"])
    ch.close()
    for b in range(2):
        ref, rref = orc.demod_mmdvm(x[b], cal=2.0)
        g = col.samples(b, 0)
        assert g.size == ref.size and np.array_equal(g, ref)
        tg = col.tags(b, 0)
        assert tg.size == rref.size and np.allclose(tg, rref, rtol=0, atol=1e-4)
        assert np.abs(ref).max() > 1000


@pytest.mark.parametrize("first", ["cf32", "sc16"])
def test_formats_alternate_on_one_handle(qrl_ctx, first):
    """6. the format belongs to the call: cf32 (the converted floats) and sc16 calls alternate over the cuts of test 1 and give the whole stream's result"""
    import qradiolink_amd as q
    v, ref = _set64()
    cuts = CUTS1[1]
    ch = q.Channelizer(qrl_ctx, M64, batch=2, max_chunk=max(cuts))
    ch.calibrate_rssi(CAL64)
    ch.enable_4fsk()
    col = _feed(ch, v[:2], cuts, [first, "sc16" if first == "cf32" else "cf32"], fsk=True)
    ch.close()
    _check64(col, (0, 1), (0, 1), ref)


def test_scale_setter(qrl_ctx):
    """7. scale 1 / 2047 (no power of two) on a 12-bit input: the oracle of the converted floats; 0, NaN and inf are refused and the old scale stays"""
    import qradiolink_amd as q
    M, cuts = 10, [10 * 1500, 10 * 1500]
    n = sum(cuts)
    v = _quantise(_wideband(M, n, seed=712, nstreams=2), peak=2000.0, edge=np.array([-2048, 2047, 0, 1, -1, -2048, 2047, 1, 0, -1], np.int16))
    assert np.abs(v.astype(np.int32)).max() <= 2048
    scale = 1.0 / 2047.0
    x = _floats(v, scale)
    ch = q.Channelizer(qrl_ctx, M, batch=2, max_chunk=max(cuts))
    ch.set_sc16_scale(scale)
    col = _Collect(ch, False)
    ch.process_sc16(_dev16(v[:, :2 * cuts[0]]))
    col.take()
    for bad in (0.0, float("nan"), float("inf"), float("-inf")):
        assert ch.lib.qrl_chan_set_sc16_scale(ch.h, C.c_float(bad)) == QRL_ERR_ARG, bad
        with pytest.raises(q.QrlError):
            ch.set_sc16_scale(bad)
    ch.process_sc16(_dev16(v[:, 2 * cuts[0]:]))
    col.take()
    ch.close()
    for b in range(2):
        ref = orc.demod_mmdvm_multi(x[b], M)
        for c in range(M):
            g = col.samples(b, c)
            assert g.size == ref.shape[1] and np.array_equal(g, ref[c]), (b, c)
    assert np.abs(ref).max() > 1000


def test_refusals_leave_the_handle_usable(qrl_ctx):
    """8. a misaligned base (iq offset by one sample), a stride that is no multiple of 4 samples and, on a form 3 handle, any sc16 call: QRL_ERR_ARG,
    nothing changed -- the valid calls that follow still give the oracle's answer"""
    import torch
    import qradiolink_amd as q
    v, ref = _set64()
    lib = q.load_library()
    cuts = CUTS1[1]
    ch = q.Channelizer(qrl_ctx, M64, batch=2, max_chunk=max(cuts))
    ch.calibrate_rssi(CAL64)
    ch.enable_4fsk()
    vp = C.c_void_p
    n0 = cuts[0]
    wide = torch.zeros((2, 2 * (n0 + 8)), dtype=torch.int16, device="cuda")
    chan_out = torch.zeros((1, 2, M64, n0 // 64), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    args = (vp(ch.out.data_ptr()), ch.cap, vp(ch.counts.data_ptr()))
    assert lib.qrl_chan_process_sc16(ch.h, vp(wide.data_ptr() + 4), n0 + 8, n0, *args) == QRL_ERR_ARG          # base off by one sample
    assert b"16-byte" in lib.qrl_last_error()
    assert lib.qrl_chan_process_sc16(ch.h, vp(wide.data_ptr()), n0 + 6, n0, *args) == QRL_ERR_ARG              # stride % 4 == 2
    assert lib.qrl_chan_channelize_sc16(ch.h, vp(wide.data_ptr() + 4), n0 + 8, n0, vp(chan_out.data_ptr()), n0 // 64, 1) == QRL_ERR_ARG
    assert lib.qrl_chan_channelize_sc16(ch.h, vp(wide.data_ptr()), n0 + 6, n0, vp(chan_out.data_ptr()), n0 // 64, 1) == QRL_ERR_ARG
    col = _feed(ch, v[:2], cuts, ["sc16"], fsk=True)
    ch.close()
    _check64(col, (0, 1), (0, 1), ref)
    # form 3: its input is channel samples.  Refused, and the handle goes on with qrl_chan_process_channels: the channel samples of stream 0 (a form 0
    # handle's channelize half on the converted floats) through it give the oracle's int16 samples of those channels
    n = N64
    pfb = q.Channelizer(qrl_ctx, M64, batch=1, max_chunk=n)
    rows = torch.zeros((1, 1, M64, n // 64), dtype=torch.complex64, device="cuda")
    torch.cuda.synchronize()
    pfb.channelize_async(_dev32(_floats(v[:1])), rows, 1)
    pfb.sync()
    pfb.close()
    f3 = q.Channelizer(qrl_ctx, 1, batch=M64, max_chunk=n // 64, form=3)
    f3.calibrate_rssi(CAL64)
    raw = _dev16(v[:1].repeat(M64, axis=0)[:, :2 * 64 * 16])
    assert lib.qrl_chan_process_sc16(f3.h, vp(raw.data_ptr()), raw.stride(0) // 2, 64 * 16, vp(f3.out.data_ptr()), f3.cap, vp(f3.counts.data_ptr())) == QRL_ERR_ARG
    assert b"form 3" in lib.qrl_last_error()
    assert lib.qrl_chan_channelize_sc16(f3.h, vp(raw.data_ptr()), raw.stride(0) // 2, 64 * 16, vp(rows.data_ptr()), n // 64, 1) == QRL_ERR_ARG
    assert b"form 3" in lib.qrl_last_error()
    chan_in = rows.reshape(M64, n // 64)
    f3.process_channels_async(chan_in, n // 64)
    f3.sync()
    cnt, o = f3.counts.cpu().numpy(), f3.out.cpu().numpy()
    for c in range(M64):
        g = o[c, 0, :cnt[c, 0]]
        assert g.size == ref[0][0].shape[1] and np.array_equal(g, ref[0][0][c]), c
    f3.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_channelize_sc16_equals_channelize_of_the_floats(qrl_ctx, groups):
    """9. the channelize half: chan_out equals, bit for bit, that of a second fresh handle fed the converted floats (held to the oracle by the
    existing tests), over two calls"""
    import torch
    import qradiolink_amd as q
    v, _ = _set64()
    x = _floats(v)
    cuts = [64 * 31, 64 * 1200]
    outs = []
    for fmt in ("sc16", "cf32"):
        ch = q.Channelizer(qrl_ctx, M64, batch=2, max_chunk=max(cuts))
        got, pos = [], 0
        for cut in cuts:
            chan_out = torch.full((groups, 2, M64 // groups, cut // 64), float("nan"), dtype=torch.complex64, device="cuda")
            torch.cuda.synchronize()
            if fmt == "sc16":
                ch.channelize_sc16_async(_dev16(v[:2, 2 * pos:2 * (pos + cut)]), chan_out, groups)
            else:
                ch.channelize_async(_dev32(x[:2, pos:pos + cut]), chan_out, groups)
            ch.sync()
            got.append(chan_out.cpu().numpy())
            pos += cut
        ch.close()
        outs.append(got)
    for a, b in zip(*outs):
        assert not np.isnan(a.view(np.float32)).any()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(outs[0][1]).max() > 0.01
