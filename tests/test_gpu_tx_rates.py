"""The transmitters' gr_mod_base back end at every device-rate class from 2 to 183 Msps, bit for bit against the oracle: both interpolator kernels
(k_tx_interp_c below the dispatch threshold of tx_common.hpp, k_tx_interp_mfma from it up), either side of a 32-phase tile, ragged calls with the
state carried, sc16 output with exact clip counts, per-stream offsets and a phase-continuous retune, the analogue handles, the limits of the range
and a TX -> RX loopback at 100 Msps.  Every comparison is a uint32 view against orc.tx_interp(orc.rotator(x1, inc), rate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
import sig

pytestmark = pytest.mark.gpu

B = 3
QPSK250K, NBFM5000, USB2500 = 26, 9, 11
QRL_ERR_ARG, QRL_ERR_TOO_BIG = -1, -5
M64 = 2 ** 64 - 1
OFFSET = 12500.0
CUTS = [1, 7, 3, 40]          # bytes per call: 32 samples at 1 Msps = one tile of columns; 224 cross the 210-lag warm-up; then ragged calls
MFMA_MIN_RATE = 4000000       # kTxMfmaMinInterp of tx_common.hpp: the first rate k_tx_interp_mfma takes
RATES = [2000000, MFMA_MIN_RATE - 1000000, MFMA_MIN_RATE, 31000000, 32000000, 33000000, 64000000, 65000000, 100000000, 183000000]
SENTINEL = 0x5A5A


def _inc(hz):
    return orc.phase_inc_to_turn(2 * np.pi * hz / 1000000.0)


@functools.lru_cache(maxsize=None)
def _payloads():
    rng = np.random.default_rng(183)
    data = rng.integers(0, 256, (B, sum(CUTS)), dtype=np.uint8)
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def _x1(gain=1.0):
    """the 1 Msps oracle of every stream; multiply_const_cc(4) is exact in f32, so the gain-1 output x 4 is the gain-4 one"""
    out = [orc.mod_qpsk(_payloads()[b]) * np.float32(gain) for b in range(B)]
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref(rate, gain=1.0):
    out = [orc.tx_interp(orc.rotator(x, _inc(OFFSET)), rate) for x in _x1(gain)]
    for y in out:
        y.setflags(write=False)
    return out


def _same_bits(got, ref, what):
    assert got.size == ref.size, "%s: %d samples, the oracle has %d" % (what, got.size, ref.size)
    g, r = np.ascontiguousarray(got).view(np.uint32), ref.view(np.uint32)
    if not np.array_equal(g, r):
        bad = np.flatnonzero(g != r)
        raise AssertionError("%s: %d of %d words differ, first at complex sample %d" % (what, bad.size, g.size, bad[0] // 2))


def conv(x, scale=32767.0):
    """complex64 [n] -> (int16 [n, 2], clipped components): the float_to_short rule, as tests/test_gpu_sc16_output.py converts"""
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(r, -32768, 32767).astype(np.int16).reshape(-1, 2), int(np.count_nonzero((r > 32767) | (r < -32768)))


@pytest.mark.parametrize("rate", RATES, ids=["%dM" % (r // 1000000) for r in RATES])
def test_every_rate_class_bit_exact_in_ragged_calls(qrl_ctx, rate):
    import torch
    import qradiolink_amd as q
    I = rate // 1000000
    data = _payloads()
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(CUTS), device_samp_rate=rate, carrier_offset_hz=OFFSET)
    assert mod.spb == 32 * I
    d = torch.from_numpy(np.array(data)).cuda()
    parts, pos = [], 0
    for c in CUTS:
        parts.append(mod.process(d[:, pos:pos + c].contiguous()).cpu().numpy())
        pos += c
    mod.close()
    got = np.concatenate(parts, axis=1)
    refs = _ref(rate)
    first = 210 * I                                                   # the outputs of the first 210 input samples: the stream start
    for b in range(B):
        _same_bits(got[b][:first], refs[b][:first], "%d Msps, stream %d, stream start" % (I, b))
        _same_bits(got[b], refs[b], "%d Msps, stream %d" % (I, b))


def _sc16_buffer(torch, count):
    """[B, count + 3, 2] int16 filled with a sentinel: an odd pitch, and three samples behind every row that must stay"""
    return torch.full((B, count + 3, 2), SENTINEL, dtype=torch.int16, device="cuda")


def _check_sc16(buf, view, refs):
    clips = []
    for b in range(B):
        want, nclip = conv(refs[b])
        assert view.shape[1] == want.shape[0]
        assert np.array_equal(buf[b, :want.shape[0]], want), "stream %d differs from the converted oracle output" % b
        assert np.all(buf[b, want.shape[0]:] == SENTINEL), "stream %d: written behind its %d samples" % (b, want.shape[0])
        clips.append(nclip)
    return clips


@pytest.mark.parametrize("rate", [100000000, 183000000], ids=["100M", "183M"])
def test_sc16_output_and_clip_counts(qrl_ctx, rate):
    """process_sc16 against rintf(ref * scale) saturated, at a bb_gain under which components clip: counts exact per stream and summed over the
    calls; then cf32 and sc16 calls alternating on a second handle"""
    import torch
    import qradiolink_amd as q
    I = rate // 1000000
    data = _payloads()
    refs = _ref(rate, 4.0)
    e = np.cumsum([0] + CUTS) * 32 * I
    parts = [[x[e[i]:e[i + 1]] for x in refs] for i in range(len(CUTS))]
    whole = [conv(x) for x in refs]
    allv = np.concatenate([w[0].ravel() for w in whole])
    assert (allv == 32767).any() and (allv == -32768).any() and all(w[1] > 0 for w in whole) and len({w[1] for w in whole}) >= 2
    d = torch.from_numpy(np.array(data)).cuda()
    for alternate in (False, True):
        mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(CUTS), device_samp_rate=rate, carrier_offset_hz=OFFSET)
        mod.set_bb_gain(4.0)
        clip = torch.zeros(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        mod.set_sc16_clip_counts(clip)
        total, pos = [0] * B, 0
        for i, c in enumerate(CUTS):
            chunk = d[:, pos:pos + c].contiguous()
            pos += c
            if alternate and i % 2 == 0:
                got = mod.process(chunk).cpu().numpy()
                for b in range(B):
                    _same_bits(got[b], parts[i][b], "%d Msps, cf32 call %d, stream %d" % (I, i, b))
            else:
                buf = _sc16_buffer(torch, parts[i][0].size)
                view = mod.process_sc16_async(chunk, out=buf)
                mod.sync()
                total = [a + n for a, n in zip(total, _check_sc16(buf.cpu().numpy(), view, parts[i]))]
            assert clip.cpu().numpy().tolist() == total, "call %d: clip counters" % i
        assert all(n > 0 for n in total)
        mod.close()


def test_per_stream_offsets_and_retune_at_100_msps(qrl_ctx):
    import torch
    import qradiolink_amd as q
    rate = 100000000
    first, second = [25000.0, 0.0, -12500.0], [25000.0, 7000.0, -12500.0]      # stream 1 retuned between two calls
    data = _payloads()
    cut = CUTS[0] + CUTS[1]
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=sum(CUTS) - cut, device_samp_rate=rate, carrier_offset_hz=first[0])
    mod.set_carrier_offsets(first)
    d = torch.from_numpy(np.array(data)).cuda()
    p1 = mod.process(d[:, :cut].contiguous()).cpu().numpy()
    mod.set_carrier_offsets(second)
    p2 = mod.process(d[:, cut:].contiguous()).cpu().numpy()
    mod.close()
    got = np.concatenate([p1, p2], axis=1)
    k = cut * 32                                                       # 1 Msps samples before the retune
    for b in range(B):
        x1 = _x1()[b]
        rot = np.concatenate([orc.rotator(x1[:k], _inc(first[b])), orc.rotator(x1[k:], _inc(second[b]), (k * _inc(first[b])) & M64)])
        _same_bits(got[b], orc.tx_interp(rot, rate), "stream %d" % b)


def test_analog_back_end_nbfm_at_100_msps(qrl_ctx):
    """125 x 100 outputs per audio sample; 500 inputs per 4 audio samples are no multiple of the 32-column tile"""
    import torch
    import qradiolink_amd as q
    rate, offset, cuts = 100000000, 25000.0, [8, 4, 12]
    n = sum(cuts)
    t = np.arange(n) / 8000.0
    audio = np.stack([0.6 * np.sin(2 * np.pi * 700 * t) + 0.3 * np.sin(2 * np.pi * 1500 * t), np.random.default_rng(44).uniform(-0.8, 0.8, n)]).astype(np.float32)
    mod = q.AMod(qrl_ctx, NBFM5000, batch=2, max_samples=max(cuts), bb_gain=0.75, device_samp_rate=rate, carrier_offset_hz=offset)
    assert mod.spa == 125 * 100
    parts, pos = [], 0
    for c in cuts:
        parts.append(mod.process(torch.from_numpy(np.ascontiguousarray(audio[:, pos:pos + c])).cuda()).cpu().numpy())
        pos += c
    mod.close()
    got = np.concatenate(parts, axis=1)
    for b in range(2):
        ref = orc.tx_interp(orc.rotator(orc.mod_nbfm(audio[b], filter_width=5000, bb_gain=0.75), _inc(offset)), rate)
        _same_bits(got[b], ref, "stream %d" % b)


def test_analog_back_end_usb_at_65_msps(qrl_ctx):
    """one call of 2048 audio samples (SSB works in whole chunks of 1024)"""
    import torch
    import qradiolink_amd as q
    rate, n = 65000000, 2048
    t = np.arange(n) / 8000.0
    audio = np.stack([0.6 * np.sin(2 * np.pi * 700 * t) + 0.3 * np.sin(2 * np.pi * 1500 * t), np.random.default_rng(45).uniform(-0.8, 0.8, n)]).astype(np.float32)
    mod = q.AMod(qrl_ctx, USB2500, batch=2, max_samples=n, bb_gain=0.75, device_samp_rate=rate, carrier_offset_hz=-10000.0)
    assert mod.spa == 125 * 65
    got = mod.process(torch.from_numpy(audio).cuda()).cpu().numpy()
    mod.close()
    for b in range(2):
        ref = orc.tx_interp(orc.rotator(orc.mod_ssb(audio[b], sb=0, bb_gain=0.75), _inc(-10000.0)), rate)
        _same_bits(got[b], ref, "stream %d" % b)


def _create_mod(q, ctx, rate, max_bytes):
    cfg = q._ModConfig()
    cfg.modem_type, cfg.use_mode_defaults, cfg.batch, cfg.max_bytes, cfg.device_samp_rate = QPSK250K, 1, 1, max_bytes, rate
    h = C.c_void_p()
    return ctx.lib.qrl_mod_create(ctx.h, C.byref(cfg), C.byref(h)), h


def _create_amod(q, ctx, rate, max_samples):
    cfg = q._AModConfig(NBFM5000, 1, max_samples, None, 1.0, rate, 0.0)
    h = C.c_void_p()
    return ctx.lib.qrl_amod_create(ctx.h, C.byref(cfg), C.byref(h)), h


def test_limits_of_the_rate_range(qrl_ctx):
    import torch
    import qradiolink_amd as q
    lib = qrl_ctx.lib
    for rate in (184000000, 65500000):
        for create in (_create_mod, _create_amod):
            rc, h = create(q, qrl_ctx, rate, 16)
            assert rc == QRL_ERR_ARG and not h.value, (rate, rc)
            assert "183" in lib.qrl_last_error().decode(), lib.qrl_last_error().decode()
    # 32 samples per byte at 1 Msps (QPSK-250k), 125 per audio sample (NBFM): the largest call would reach 2^32 device-rate samples per stream
    big_bytes = -(-2 ** 32 // (32 * 183))
    rc, h = _create_mod(q, qrl_ctx, 183000000, big_bytes)
    assert rc == QRL_ERR_TOO_BIG and not h.value, rc
    assert "2^32" in lib.qrl_last_error().decode()
    rc, h = _create_amod(q, qrl_ctx, 183000000, -(-2 ** 32 // (125 * 183)) + 3 & ~3)
    assert rc == QRL_ERR_TOO_BIG and not h.value, rc
    assert "2^32" in lib.qrl_last_error().decode()
    # a valid handle made afterwards works
    data = _payloads()[:, :CUTS[0]]
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=CUTS[0], device_samp_rate=183000000, carrier_offset_hz=OFFSET)
    got = mod.process(torch.from_numpy(np.array(data)).cuda()).cpu().numpy()
    mod.close()
    for b in range(B):
        _same_bits(got[b], _ref(183000000)[b][:got.shape[1]], "stream %d" % b)


def test_tx_rx_loopback_at_100_msps(qrl_ctx):
    """the body of test_device_rate_tx_rx_loopback (tests/test_gpu_tx.py) at the receivers' C3 rate: TX at 100 Msps with +25 kHz offset -> x 0.3 ->
    RX at 100 Msps tuned to the same offset; all three frames come back with their payloads"""
    import torch
    import qradiolink_amd as q
    rate = 100000000
    rng = np.random.default_rng(10)
    data, payloads = sig.frames("qpsk250k", 3, rng)
    # a run of idle bytes in front: the receiver acquires the constant phase the two filter delays leave behind before the first frame;
    # the tail flushes the back-end and front-end filters and the Viterbi frames
    data = np.concatenate([np.full(400, 0xAA, np.uint8), data, np.full(400, 0xAA, np.uint8)])
    mod = q.Mod(qrl_ctx, QPSK250K, batch=1, max_bytes=data.size, device_samp_rate=rate, carrier_offset_hz=25000.0)
    iq = mod.process(torch.from_numpy(data[None, :]).cuda())
    mod.close()
    iq.mul_(0.3)
    n = iq.shape[1] & ~7
    dem = q.Demod(qrl_ctx, QPSK250K, batch=1, max_chunk=n, device_samp_rate=rate, carrier_offset_hz=25000.0)
    out = q.collect(dem, iq[:, :n], n)
    dem.close()
    fr = sig.find_frames(out["bits_a"][0], bytes([0xDE, 0x98, 0xAA]), 1516 * 8)
    assert all(p in fr for p in payloads), "%d of %d frames found" % (sum(p in fr for p in payloads), len(payloads))
