"""int16 IQ (sc16) output of the transmitters (qrl_mod / qrl_amod / qrl_synth _process_sc16): every terminal kernel against the oracle's cf32
output converted in numpy, bit for bit, with an odd out_stride and a sentinel behind every row; saturation and exact per-stream clip counters; the
scale setter; NaN; cf32 and sc16 calls alternating on one handle; a misaligned pointer."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

B = 3
SENTINEL = 0x5A5A
QRL_ERR_ARG = -1
QPSK250K, QPSK2K, BPSK2K, FSK2_1K, GMSK10K, NBFM5000, USB2500, AM5000 = 26, 7, 0, 18, 22, 9, 11, 14


# ---- the reference conversion: the float_to_short rule on the oracle's cf32 samples
def conv(x, scale=32767.0):
    """complex64 [n] -> (int16 [n, 2], clipped components)"""
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(r, -32768, 32767).astype(np.int16).reshape(-1, 2), int(np.count_nonzero((r > 32767) | (r < -32768)))


def _bytes(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 256, n, dtype=np.uint8) for _ in range(B)])


def _audio(seed, n):
    t = np.arange(n) / 8000.0
    rng = np.random.default_rng(seed)
    return np.stack([0.5 * np.sin(2 * np.pi * 700 * t) + 0.2 * np.sin(2 * np.pi * 1900 * t), rng.uniform(-0.7, 0.7, n),
                     0.6 * np.sin(2 * np.pi * 440 * t) * rng.uniform(0.2, 1.0, n)]).astype(np.float32)


def _pcm(N, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return np.stack([(rng.uniform(3000, 12000) * np.sin(2 * np.pi * rng.uniform(200, 2500) * t / 24000 + rng.uniform(0, 6))
                      + rng.normal(0, 300, n)).astype(np.int16) for _ in range(N)])


def back_end(x1, rate, offset):
    """gr_mod_base back end on a 1 Msps stream: rotator, then the interpolator to the device rate"""
    y = orc.rotator(x1, orc.phase_inc_to_turn(2 * np.pi * offset / 1000000.0)) if offset != 0.0 else x1
    return orc.tx_interp(y, rate) if rate > 1000000 else y


# name -> (modem, oracle at 1 Msps, bytes per call, device rate (0: no back end), offset, terminal kernel)
MOD_CASES = {
    "qpsk250k": (QPSK250K, lambda d: orc.mod_qpsk(d), 67, 0, 0.0, "k_tx_interp_sym"),
    "qpsk2k": (QPSK2K, lambda d: orc.mod_qpsk(d, sps=500, filter_width=1300), 3, 0, 0.0, "k_tx_interp"),
    "bpsk2k": (BPSK2K, lambda d: orc.mod_bpsk(d, sps=250, filter_width=2800), 2, 0, 0.0, "k_tx_interp"),
    "2fsk1k": (FSK2_1K, lambda d: orc.mod_2fsk(d, sps=50, filter_width=2000, fm=False), 4, 0, 0.0, "k_tx_interp_c"),
    "m17": ("M17", lambda d: orc.mod_m17(d), 6, 0, 0.0, "k_tx_interp_c"),
    "dmr": ("DMR", lambda d: orc.mod_dmr(d), 33, 0, 0.0, "k_tx_interp_c"),
    # (33 bytes of DMR are 660 items at 24 ksps, all inside the 1439-item delay of gr_zero_idle_bursts: zeros.  132 bytes reach the signal.)
    "dmr-132": ("DMR", lambda d: orc.mod_dmr(d), 132, 0, 0.0, "k_tx_interp_c"),
    "dsss": ("BPSK8", lambda d: orc.mod_dsss(d), 1, 0, 0.0, "k_tx_interp_c"),
    "qpsk250k-1M-rot": (QPSK250K, lambda d: orc.mod_qpsk(d), 41, 1000000, -12500.0, "k_tx_rot"),
    "qpsk250k-4M": (QPSK250K, lambda d: orc.mod_qpsk(d), 67, 4000000, 25000.0, "k_tx_interp_c (back end)"),
    "gmsk10k-10M": (GMSK10K, lambda d: orc.mod_gmsk(d, sps=10, filter_width=20000), 20, 10000000, 50000.0, "k_tx_interp_c (back end, taps in global memory)"),
    "2fsk1k-2M": (FSK2_1K, lambda d: orc.mod_2fsk(d, sps=50, filter_width=2000, fm=False), 2, 2000000, 0.0, "k_tx_interp_c (back end)"),
}
# name -> (modem, oracle at 1 Msps, audio samples, device rate, offset)
AMOD_CASES = {
    "nbfm-4M": (NBFM5000, lambda a: orc.mod_nbfm(a, filter_width=5000), 324, 4000000, 25000.0),
    "am-1M": (AM5000, lambda a: orc.mod_am(a), 250, 0, 0.0),                       # k_an_fir_ccc is the terminal kernel
    "usb-2M": (USB2500, lambda a: orc.mod_ssb(a, sb=0), 2048, 2000000, 0.0),
}


@functools.lru_cache(maxsize=None)
def mod_case(name):
    """(payloads [B, n], oracle output per stream) of a MOD_CASES row, computed once"""
    _, oracle, n, rate, offset, _ = MOD_CASES[name]
    data = _bytes(sorted(MOD_CASES).index(name) + 100, n)
    return data, [back_end(oracle(data[b]), rate, offset) for b in range(B)]


@functools.lru_cache(maxsize=None)
def amod_case(name):
    _, oracle, n, rate, offset = AMOD_CASES[name]
    audio = _audio(sorted(AMOD_CASES).index(name) + 200, n)
    return audio, [back_end(oracle(audio[b]), rate, offset) for b in range(B)]


def _modem(q, m):
    return getattr(q, "MODEM_" + m) if isinstance(m, str) else m


def _buffer(torch, count):
    """[B, count + 3, 2] int16 filled with the sentinel: an odd pitch, and three samples behind every row that must stay"""
    return torch.full((B, count + 3, 2), SENTINEL, dtype=torch.int16, device="cuda")


def _counters(torch):
    c = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return c


def check_rows(buf, view, refs, scale=32767.0):
    """buf: the whole buffer (numpy [B, pitch, 2]); view: what the call returned; refs: the oracle's cf32 output per stream.  Returns the numpy clip counts."""
    clips = []
    for b in range(B):
        want, nclip = conv(refs[b], scale)
        assert view.shape[1] == want.shape[0], "stream %d: %d samples, the oracle has %d" % (b, view.shape[1], want.shape[0])
        assert np.array_equal(buf[b, :want.shape[0]], want), "stream %d differs from the converted oracle output" % b
        assert np.all(buf[b, want.shape[0]:] == SENTINEL), "stream %d: written behind its %d samples" % (b, want.shape[0])
        clips.append(nclip)
    return clips


def assert_no_saturation(refs):
    """default gain: the case exercises rounding, not saturation"""
    for x in refs:
        assert np.abs(x.view(np.float32)).max() * 32767 < 32767


@pytest.mark.parametrize("name", sorted(MOD_CASES))
def test_mod_sc16_matches_converted_oracle(qrl_ctx, name):
    import torch
    import qradiolink_amd as q
    modem, _, n, rate, offset, _ = MOD_CASES[name]
    data, refs = mod_case(name)
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256                                                # more than one workgroup per stream
    mod = q.Mod(qrl_ctx, _modem(q, modem), batch=B, max_bytes=n, device_samp_rate=rate, carrier_offset_hz=offset)
    buf, clip = _buffer(torch, count), _counters(torch)
    mod.set_sc16_clip_counts(clip)
    view = mod.process_sc16_async(torch.from_numpy(data).cuda(), out=buf)
    mod.sync()
    assert view.dtype == torch.int16 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


@pytest.mark.parametrize("name", sorted(AMOD_CASES))
def test_amod_sc16_matches_converted_oracle(qrl_ctx, name):
    import torch
    import qradiolink_amd as q
    modem, _, n, rate, offset = AMOD_CASES[name]
    audio, refs = amod_case(name)
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256
    mod = q.AMod(qrl_ctx, modem, batch=B, max_samples=n, device_samp_rate=rate, carrier_offset_hz=offset)
    buf, clip = _buffer(torch, count), _counters(torch)
    mod.set_sc16_clip_counts(clip)
    view = mod.process_sc16(torch.from_numpy(audio).cuda(), out=buf)
    assert view.dtype == torch.int16 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


@pytest.mark.parametrize("single", [False, True], ids=["3-channels", "single-carrier"])
def test_synth_sc16_matches_converted_oracle(qrl_ctx, single):
    import torch
    import qradiolink_amd as q
    N, n = (1, 240) if single else (3, 240)
    x = np.stack([_pcm(N, n, seed=300 + 10 * N + b) for b in range(B)])
    refs = [orc.mod_mmdvm(x[b, 0]) if single else orc.mod_mmdvm_multi(x[b]) for b in range(B)]
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256 and count % 256
    syn = q.Synth(qrl_ctx, N, batch=B, max_samples=n, single_carrier=single)
    buf, clip = _buffer(torch, count), _counters(torch)
    syn.set_sc16_clip_counts(clip)
    view = syn.process_sc16(torch.from_numpy(x).cuda(), out=buf)
    assert view.dtype == torch.int16 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    syn.close()


# ---- saturation and the clip counters
def _saturation_preconditions(refs):
    conv_all = [conv(x) for x in refs]
    allv = np.concatenate([c[0].ravel() for c in conv_all])
    assert (allv == 32767).any() and (allv == -32768).any()
    counts = [c[1] for c in conv_all]
    assert all(c > 0 for c in counts) and len(set(counts)) >= 2, counts


def test_mod_saturation_and_clip_counts(qrl_ctx):
    """QPSK250K at 4 Msps with bb_gain 4: three calls sc16, cf32, sc16; output exact, counts[b] exact, added up over the sc16 calls, untouched by the cf32 one"""
    import torch
    import qradiolink_amd as q
    cuts = [67, 5, 40]
    data = _bytes(400, sum(cuts))
    # multiply_const_cc(4) is exact in f32, so the oracle's gain-1 modulator output x 4 is the gain-4 one
    refs = [back_end(orc.mod_qpsk(data[b]) * np.float32(4.0), 4000000, 25000.0) for b in range(B)]
    e = np.cumsum([0] + cuts) * 128                                    # 32 samples per byte at 1 Msps, x 4
    parts = [[x[e[i]:e[i + 1]] for x in refs] for i in range(3)]
    _saturation_preconditions(parts[0])
    _saturation_preconditions(parts[2])
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(cuts), bb_gain=4.0, device_samp_rate=4000000, carrier_offset_hz=25000.0)
    clip = _counters(torch)
    mod.set_sc16_clip_counts(clip)
    d = torch.from_numpy(data).cuda()
    buf = _buffer(torch, parts[0][0].size)
    view = mod.process_sc16_async(d[:, :cuts[0]].contiguous(), out=buf)
    mod.sync()
    c0 = check_rows(buf.cpu().numpy(), view, parts[0])
    assert clip.cpu().numpy().tolist() == c0
    mid = mod.process(d[:, cuts[0]:cuts[0] + cuts[1]].contiguous()).cpu().numpy()
    for b in range(B):
        assert np.array_equal(mid[b].view(np.uint32), parts[1][b].view(np.uint32))
    assert clip.cpu().numpy().tolist() == c0, "a cf32 call touched the clip counters"
    buf = _buffer(torch, parts[2][0].size)
    view = mod.process_sc16_async(d[:, cuts[0] + cuts[1]:].contiguous(), out=buf)
    mod.sync()
    c2 = check_rows(buf.cpu().numpy(), view, parts[2])
    assert clip.cpu().numpy().tolist() == [a + b for a, b in zip(c0, c2)]
    mod.set_sc16_clip_counts(None)                                     # counting off: the array stays as it is
    mod.process_sc16(d[:, :cuts[0]].contiguous())
    assert clip.cpu().numpy().tolist() == [a + b for a, b in zip(c0, c2)]
    mod.close()


def test_amod_saturation_and_clip_counts(qrl_ctx):
    """NBFM with bb_gain 3 (k_tx_interp_c as the analogue chain's terminal kernel): exact output and counters over two sc16 calls with a cf32 call between"""
    import torch
    import qradiolink_amd as q
    cuts = [324, 8, 100]
    audio = _audio(401, sum(cuts))
    refs = [orc.mod_nbfm(audio[b], filter_width=5000, bb_gain=3.0) for b in range(B)]
    e = np.cumsum([0] + cuts) * 125
    parts = [[x[e[i]:e[i + 1]] for x in refs] for i in range(3)]
    _saturation_preconditions(parts[0])
    _saturation_preconditions(parts[2])
    mod = q.AMod(qrl_ctx, NBFM5000, batch=B, max_samples=max(cuts), bb_gain=3.0)
    clip = _counters(torch)
    mod.set_sc16_clip_counts(clip)
    a = torch.from_numpy(audio).cuda()
    buf = _buffer(torch, parts[0][0].size)
    view = mod.process_sc16(a[:, :cuts[0]].contiguous(), out=buf)
    c0 = check_rows(buf.cpu().numpy(), view, parts[0])
    assert clip.cpu().numpy().tolist() == c0
    mid = mod.process(a[:, cuts[0]:cuts[0] + cuts[1]].contiguous()).cpu().numpy()
    for b in range(B):
        assert np.array_equal((mid[b].view(np.float32) + np.float32(0)).view(np.uint32), (parts[1][b].view(np.float32) + np.float32(0)).view(np.uint32))
    assert clip.cpu().numpy().tolist() == c0, "a cf32 call touched the clip counters"
    buf = _buffer(torch, parts[2][0].size)
    view = mod.process_sc16(a[:, cuts[0] + cuts[1]:].contiguous(), out=buf)
    c2 = check_rows(buf.cpu().numpy(), view, parts[2])
    assert clip.cpu().numpy().tolist() == [x + y for x, y in zip(c0, c2)]
    mod.close()


# the counting block of the terminal kernels the two tests above do not reach, each with lanes behind the end of its last workgroup
def _clip_case(name):
    """(make handle, input [B, ...], oracle output per stream) at bb_gain 4; x 4 is exact in f32, so where the oracle takes no gain its output x 4 is the reference"""
    g = np.float32(4.0)
    if name in ("k_tx_interp_sym", "k_tx_interp", "k_tx_rot"):
        modem, oracle, n, rate, offset, _ = MOD_CASES[{"k_tx_interp_sym": "qpsk250k", "k_tx_interp": "qpsk2k", "k_tx_rot": "qpsk250k-1M-rot"}[name]]
        data = _bytes(600 + len(name), n)
        refs = [back_end(oracle(data[b]) * g, rate, offset) for b in range(B)]
        return (lambda q, ctx: q.Mod(ctx, modem, batch=B, max_bytes=n, bb_gain=4.0, device_samp_rate=rate, carrier_offset_hz=offset)), data, refs
    if name == "k_an_fir_ccc":
        audio = _audio(610, 250)
        return (lambda q, ctx: q.AMod(ctx, AM5000, batch=B, max_samples=250, bb_gain=4.0)), audio, [orc.mod_am(audio[b], bb_gain=4.0) for b in range(B)]
    single = name == "k_ring_store_sc16"
    N = 1 if single else 3
    x = np.stack([_pcm(N, 240, seed=620 + 10 * N + b) for b in range(B)])
    refs = [orc.mod_mmdvm(x[b, 0], bb_gain=4.0) if single else orc.mod_mmdvm_multi(x[b]) * g for b in range(B)]
    return (lambda q, ctx: q.Synth(ctx, N, batch=B, max_samples=240, bb_gain=4.0, single_carrier=single)), x, refs


@pytest.mark.parametrize("name", ["k_tx_interp_sym", "k_tx_interp", "k_tx_rot", "k_an_fir_ccc", "k_pfb_synth", "k_ring_store_sc16"])
def test_clip_counts_of_every_other_terminal_kernel(qrl_ctx, name):
    """bb_gain 4 on the handles whose terminal kernel is `name`: saturated output exact, counts[b] exact and non-zero, a second call adds"""
    import torch
    import qradiolink_amd as q
    make, x, refs = _clip_case(name)
    count = refs[0].size
    assert count % 256, "the last workgroup must be ragged"
    want = [conv(r)[1] for r in refs]
    assert all(c > 0 for c in want), want
    h = make(q, qrl_ctx)
    clip = _counters(torch)
    h.set_sc16_clip_counts(clip)
    buf = _buffer(torch, count)
    d = torch.from_numpy(x).cuda()
    if isinstance(h, q.Mod):
        view = h.process_sc16_async(d, out=buf)
        h.sync()
    else:
        view = h.process_sc16(d, out=buf)
    assert check_rows(buf.cpu().numpy(), view, refs) == want
    assert clip.cpu().numpy().tolist() == want
    if isinstance(h, q.Mod):
        h.reset()                                                      # the same stream again: the same count on top
        h.process_sc16(d)
        assert clip.cpu().numpy().tolist() == [2 * c for c in want]
    h.close()


# ---- scale
def test_set_sc16_scale(qrl_ctx):
    """2048 (a 12-bit DAC's range) is exact; 0, inf and nan are refused and leave 2048 in force"""
    import torch
    import qradiolink_amd as q
    data, refs = mod_case("qpsk250k")
    n = data.shape[1]
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=n)
    mod.set_sc16_scale(2048.0)
    d = torch.from_numpy(data).cuda()
    k = 30
    buf = _buffer(torch, k * 32)
    view = mod.process_sc16_async(d[:, :k].contiguous(), out=buf)
    mod.sync()
    check_rows(buf.cpu().numpy(), view, [x[:k * 32] for x in refs], scale=2048.0)
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        assert mod.lib.qrl_mod_set_sc16_scale(mod.h, C.c_float(bad)) == QRL_ERR_ARG
        with pytest.raises(q.QrlError):
            mod.set_sc16_scale(bad)
    buf = _buffer(torch, (n - k) * 32)
    view = mod.process_sc16_async(d[:, k:].contiguous(), out=buf)
    mod.sync()
    check_rows(buf.cpu().numpy(), view, [x[k * 32:] for x in refs], scale=2048.0)
    mod.close()
    for cls_args in ((q.AMod, (NBFM5000,), dict(batch=1, max_samples=8)), (q.Synth, (1,), dict(batch=1, max_samples=8))):
        h = cls_args[0](qrl_ctx, *cls_args[1], **cls_args[2])
        h.set_sc16_scale(2048.0)
        for bad in (0.0, float("inf"), float("nan")):
            with pytest.raises(q.QrlError):
                h.set_sc16_scale(bad)
        h.close()


# ---- NaN
def test_nan_gives_zero_and_is_not_counted(qrl_ctx):
    import torch
    import qradiolink_amd as q
    data, _ = mod_case("qpsk250k")
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=data.shape[1])
    mod.set_bb_gain(float("nan"))
    clip = _counters(torch)
    mod.set_sc16_clip_counts(clip)
    count = data.shape[1] * 32
    buf = _buffer(torch, count)
    view = mod.process_sc16_async(torch.from_numpy(data).cuda(), out=buf)
    mod.sync()
    out = buf.cpu().numpy()
    assert view.shape == (B, count, 2)
    assert np.all(out[:, :count] == 0) and np.all(out[:, count:] == SENTINEL)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


# ---- the format belongs to the call: cuts, alternation, retune
def test_mod_alternating_formats_chunks_and_retune(qrl_ctx):
    """QPSK250K at 5 Msps, +10 kHz, cuts [100, 1, 333, 66] with a retune to -30 kHz before the third; calls sc16, cf32, sc16, cf32: the converted
    concatenation is the converted one-piece oracle stream (the shape of test_gpu_tx.py test_mod_back_end_chunks_and_retune)"""
    import torch
    import qradiolink_amd as q
    cuts = [100, 1, 333, 66]
    data = _bytes(500, sum(cuts))
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(cuts), device_samp_rate=5000000, carrier_offset_hz=10000.0)
    d = torch.from_numpy(data).cuda()
    parts, pos = [], 0
    for i, c in enumerate(cuts):
        if i == 2:
            mod.set_carrier_offset(-30000.0)
        blk = d[:, pos:pos + c].contiguous()
        if i % 2 == 0:
            parts.append(mod.process_sc16(blk).cpu().numpy())
        else:
            y = mod.process(blk).cpu().numpy()
            parts.append(np.stack([conv(y[b])[0] for b in range(B)]))
        pos += c
    mod.close()
    got = np.concatenate(parts, axis=1)
    k = (cuts[0] + cuts[1]) * 32
    inc0 = orc.phase_inc_to_turn(2 * np.pi * 10000.0 / 1e6)
    inc1 = orc.phase_inc_to_turn(2 * np.pi * -30000.0 / 1e6)
    for b in range(B):
        x1 = orc.mod_qpsk(data[b])
        rot = np.concatenate([orc.rotator(x1[:k], inc0), orc.rotator(x1[k:], inc1, (k * inc0) & (2 ** 64 - 1))])
        want = conv(orc.tx_interp(rot, 5000000))[0]
        assert got[b].shape == want.shape and np.array_equal(got[b], want), "stream %d differs" % b


def test_amod_alternating_formats_chunks(qrl_ctx):
    """NBFM at 4 Msps, chunks [1000, 324, 8, 1000], calls sc16, cf32, sc16, cf32"""
    import torch
    import qradiolink_amd as q
    cuts = [1000, 324, 8, 1000]
    audio = _audio(501, sum(cuts))
    mod = q.AMod(qrl_ctx, NBFM5000, batch=B, max_samples=max(cuts), device_samp_rate=4000000, carrier_offset_hz=25000.0)
    a = torch.from_numpy(audio).cuda()
    parts, pos = [], 0
    for i, c in enumerate(cuts):
        blk = a[:, pos:pos + c].contiguous()
        if i % 2 == 0:
            parts.append(mod.process_sc16(blk).cpu().numpy())
        else:
            y = mod.process(blk).cpu().numpy()
            parts.append(np.stack([conv(y[b])[0] for b in range(B)]))
        pos += c
    mod.close()
    got = np.concatenate(parts, axis=1)
    for b in range(B):
        want = conv(back_end(orc.mod_nbfm(audio[b], filter_width=5000), 4000000, 25000.0))[0]
        assert got[b].shape == want.shape and np.array_equal(got[b], want), "stream %d differs" % b


# ---- alignment
def test_misaligned_pointer_is_refused_and_the_handle_goes_on(qrl_ctx):
    import torch
    import qradiolink_amd as q
    data, refs = mod_case("qpsk250k")
    n = data.shape[1]
    count = n * 32
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=n)
    d = torch.from_numpy(data).cuda()
    buf = _buffer(torch, count)
    torch.cuda.synchronize()
    assert mod.lib.qrl_mod_process_sc16(mod.h, d.data_ptr(), d.stride(0), n, buf.data_ptr() + 2, count + 3) == QRL_ERR_ARG
    mod.sync()
    assert np.all(buf.cpu().numpy() == SENTINEL)
    view = mod.process_sc16_async(d, out=buf)                        # nothing was consumed: the stream starts here
    mod.sync()
    check_rows(buf.cpu().numpy(), view, refs)
    mod.close()
    amod = q.AMod(qrl_ctx, NBFM5000, batch=1, max_samples=8)
    a = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    o = torch.zeros((1, 1000 + 1, 2), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert amod.lib.qrl_amod_process_sc16(amod.h, a.data_ptr(), 8, 8, o.data_ptr() + 2, 1000) == QRL_ERR_ARG
    amod.close()
    syn = q.Synth(qrl_ctx, 1, batch=1, max_samples=24, single_carrier=True)
    x = torch.zeros((1, 1, 24), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert syn.lib.qrl_synth_process_sc16(syn.h, x.data_ptr(), 24, 24, o.data_ptr() + 2, 1000, None) == QRL_ERR_ARG
    syn.close()
