"""int8 IQ (sc8) output of the transmitters (qrl_mod / qrl_amod / qrl_synth _process_sc8), the counterpart of tests/test_gpu_sc16_output.py with its
case tables: every terminal kernel against the oracle's cf32 output converted in numpy, bit for bit, in a buffer of 0x5A bytes with an odd out_stride (row
1 starts at an address = 2 mod 4; with the base moved by one sample every row does) and three samples behind every row that must stay; saturation and exact per-stream clip counters; the scale
setter; NaN; cf32, sc16 and sc8 calls alternating on one handle; the two formats' counters apart; a base moved by one sample; an odd byte address."""
import ctypes as C

import numpy as np
import pytest

import orc
import sc8_output_cases as K
import test_gpu_sc16_output as S16
from sc8_output_cases import B, conv8

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
QRL_ERR_ARG = -1
QPSK250K, NBFM5000, USB2500 = K.QPSK250K, K.NBFM5000, K.USB2500


def _buffer(torch, count):
    """[B, pitch, 2] int8 filled with 0x5A: an odd pitch, so row 1 starts at an address = 2 mod 4 and rows 0 and 2 end in the lower half of a 32-bit
    word, and three samples (four where that makes the pitch odd) behind every row that must stay"""
    buf = torch.full((B, count + 3 + count % 2, 2), SENTINEL, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 4 == 0 and buf.stride(0) % 4 == 2
    return buf


def _counters(torch):
    c = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return c


def check_rows(buf, view, refs, scale=127.0):
    """buf: the whole buffer (numpy [B, pitch, 2]); view: what the call returned; refs: the oracle's cf32 output per stream.  Returns the numpy clip counts."""
    clips = []
    for b in range(B):
        want, nclip = conv8(refs[b], scale)
        assert view.shape[1] == want.shape[0], "stream %d: %d samples, the oracle has %d" % (b, view.shape[1], want.shape[0])
        assert np.array_equal(buf[b, :want.shape[0]], want), "stream %d differs from the converted oracle output" % b
        assert np.all(buf[b, want.shape[0]:] == SENTINEL), "stream %d: written behind its %d samples" % (b, want.shape[0])
        clips.append(nclip)
    return clips


def assert_no_saturation(refs):
    for x in refs:
        assert conv8(x)[1] == 0


def _run(q, h, d, buf):
    if isinstance(h, q.Mod):
        view = h.process_sc8_async(d, out=buf)
        h.sync()
        return view
    return h.process_sc8(d, out=buf)


@pytest.mark.parametrize("name", sorted(S16.MOD_CASES))
def test_mod_sc8_matches_converted_oracle(qrl_ctx, name):
    import torch
    import qradiolink_amd as q
    modem, _, n, rate, offset, _ = S16.MOD_CASES[name]
    data, refs = S16.mod_case(name)
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256                                                # more than one workgroup per stream
    mod = q.Mod(qrl_ctx, S16._modem(q, modem), batch=B, max_bytes=n, device_samp_rate=rate, carrier_offset_hz=offset)
    buf, clip = _buffer(torch, count), _counters(torch)
    mod.set_sc8_clip_counts(clip)
    view = _run(q, mod, torch.from_numpy(data).cuda(), buf)
    assert view.dtype == torch.int8 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


@pytest.mark.parametrize("name", sorted(S16.AMOD_CASES))
def test_amod_sc8_matches_converted_oracle(qrl_ctx, name):
    import torch
    import qradiolink_amd as q
    modem, _, n, rate, offset = S16.AMOD_CASES[name]
    audio, refs = S16.amod_case(name)
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256
    mod = q.AMod(qrl_ctx, modem, batch=B, max_samples=n, device_samp_rate=rate, carrier_offset_hz=offset)
    buf, clip = _buffer(torch, count), _counters(torch)
    mod.set_sc8_clip_counts(clip)
    view = mod.process_sc8(torch.from_numpy(audio).cuda(), out=buf)
    assert view.dtype == torch.int8 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


@pytest.mark.parametrize("single", [False, True], ids=["3-channels", "single-carrier"])
def test_synth_sc8_matches_converted_oracle(qrl_ctx, single):
    import torch
    import qradiolink_amd as q
    N, n = (1, 240) if single else (3, 240)
    x = np.stack([S16._pcm(N, n, seed=300 + 10 * N + b) for b in range(B)])
    refs = [orc.mod_mmdvm(x[b, 0]) if single else orc.mod_mmdvm_multi(x[b]) for b in range(B)]
    assert_no_saturation(refs)
    count = refs[0].size
    assert count > 256 and count % 256
    syn = q.Synth(qrl_ctx, N, batch=B, max_samples=n, single_carrier=single)
    buf, clip = _buffer(torch, count), _counters(torch)
    syn.set_sc8_clip_counts(clip)
    view = syn.process_sc8(torch.from_numpy(x).cuda(), out=buf)
    assert view.dtype == torch.int8 and view.shape == (B, count, 2)
    check_rows(buf.cpu().numpy(), view, refs)
    assert clip.cpu().numpy().tolist() == [0] * B
    syn.close()


# ---- saturation and the clip counters
def test_mod_saturation_and_clip_counts(qrl_ctx):
    """QPSK250K at 4 Msps with bb_gain 4: calls sc8, cf32, sc16, sc8; output exact, the sc8 counts[b] exact and added up over the sc8 calls, untouched by
    the cf32 and the sc16 call; the sc16 counters hold the sc16 call's count alone"""
    import torch
    import qradiolink_amd as q
    cuts = K.MOD_SAT_CUTS
    data, parts = K.mod_saturation()
    K.saturation_preconditions(parts[0])
    K.saturation_preconditions(parts[2])
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(cuts), bb_gain=4.0, device_samp_rate=4000000, carrier_offset_hz=25000.0)
    clip, clip16 = _counters(torch), _counters(torch)
    mod.set_sc8_clip_counts(clip)
    mod.set_sc16_clip_counts(clip16)
    d = torch.from_numpy(data).cuda()
    buf = _buffer(torch, parts[0][0].size)
    view = _run(q, mod, d[:, :cuts[0]].contiguous(), buf)
    c0 = check_rows(buf.cpu().numpy(), view, parts[0])
    assert clip.cpu().numpy().tolist() == c0
    assert clip16.cpu().numpy().tolist() == [0] * B, "an sc8 call touched the sc16 counters"
    # the middle piece: its first 2 bytes cf32, the other 3 sc16
    mid = mod.process(d[:, cuts[0]:cuts[0] + 2].contiguous()).cpu().numpy()
    for b in range(B):
        assert np.array_equal(mid[b].view(np.uint32), parts[1][b][:2 * 128].view(np.uint32))
    mid16 = mod.process_sc16(d[:, cuts[0] + 2:cuts[0] + cuts[1]].contiguous()).cpu().numpy()
    want16 = [S16.conv(parts[1][b][2 * 128:]) for b in range(B)]
    for b in range(B):
        assert np.array_equal(mid16[b], want16[b][0])
    assert clip.cpu().numpy().tolist() == c0, "a cf32 or sc16 call touched the sc8 counters"
    assert clip16.cpu().numpy().tolist() == [w[1] for w in want16]
    buf = _buffer(torch, parts[2][0].size)
    view = _run(q, mod, d[:, cuts[0] + cuts[1]:].contiguous(), buf)
    c2 = check_rows(buf.cpu().numpy(), view, parts[2])
    assert clip.cpu().numpy().tolist() == [a + b for a, b in zip(c0, c2)]
    assert clip16.cpu().numpy().tolist() == [w[1] for w in want16]
    mod.set_sc8_clip_counts(None)                                      # counting off: the array stays as it is
    mod.process_sc8(d[:, :cuts[0]].contiguous())
    assert clip.cpu().numpy().tolist() == [a + b for a, b in zip(c0, c2)]
    mod.close()


def test_both_setters_may_name_one_array(qrl_ctx):
    import torch
    import qradiolink_amd as q
    cuts = K.MOD_SAT_CUTS
    data, parts = K.mod_saturation()
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(cuts), bb_gain=4.0, device_samp_rate=4000000, carrier_offset_hz=25000.0)
    clip = _counters(torch)
    mod.set_sc8_clip_counts(clip)
    mod.set_sc16_clip_counts(clip)
    d = torch.from_numpy(data).cuda()
    mod.process_sc8(d[:, :cuts[0]].contiguous())
    mod.process_sc16(d[:, cuts[0]:cuts[0] + cuts[1]].contiguous())
    want = [conv8(parts[0][b])[1] + S16.conv(parts[1][b])[1] for b in range(B)]
    assert clip.cpu().numpy().tolist() == want
    mod.close()


def test_amod_saturation_and_clip_counts(qrl_ctx):
    """NBFM with bb_gain 3 (k_tx_interp_c as the analogue chain's terminal kernel): exact output and counters over two sc8 calls with a cf32 call between"""
    import torch
    import qradiolink_amd as q
    cuts = K.AMOD_SAT_CUTS
    audio, parts = K.amod_saturation()
    K.saturation_preconditions(parts[0])
    K.saturation_preconditions(parts[2])
    mod = q.AMod(qrl_ctx, NBFM5000, batch=B, max_samples=max(cuts), bb_gain=3.0)
    clip = _counters(torch)
    mod.set_sc8_clip_counts(clip)
    a = torch.from_numpy(audio).cuda()
    buf = _buffer(torch, parts[0][0].size)
    view = mod.process_sc8(a[:, :cuts[0]].contiguous(), out=buf)
    c0 = check_rows(buf.cpu().numpy(), view, parts[0])
    assert clip.cpu().numpy().tolist() == c0
    mid = mod.process(a[:, cuts[0]:cuts[0] + cuts[1]].contiguous()).cpu().numpy()
    for b in range(B):
        assert np.array_equal((mid[b].view(np.float32) + np.float32(0)).view(np.uint32), (parts[1][b].view(np.float32) + np.float32(0)).view(np.uint32))
    assert clip.cpu().numpy().tolist() == c0, "a cf32 call touched the clip counters"
    buf = _buffer(torch, parts[2][0].size)
    view = mod.process_sc8(a[:, cuts[0] + cuts[1]:].contiguous(), out=buf)
    c2 = check_rows(buf.cpu().numpy(), view, parts[2])
    assert clip.cpu().numpy().tolist() == [x + y for x, y in zip(c0, c2)]
    mod.close()


def test_a_stream_that_clips_nowhere(qrl_ctx):
    """USB under a scale of 1000 with stream 1 silent: its counter stays where it was (no wave of it adds), the others are exact"""
    import torch
    import qradiolink_amd as q
    audio, refs = K.silent_stream()
    K.silent_preconditions(refs)
    mod = q.AMod(qrl_ctx, USB2500, batch=B, max_samples=audio.shape[1])
    mod.set_sc8_scale(K.SILENT_SCALE)
    clip = _counters(torch)
    mod.set_sc8_clip_counts(clip)
    buf = _buffer(torch, refs[0].size)
    view = mod.process_sc8(torch.from_numpy(audio).cuda(), out=buf)
    want = check_rows(buf.cpu().numpy(), view, refs, scale=K.SILENT_SCALE)
    assert want[1] == 0 and clip.cpu().numpy().tolist() == want
    mod.close()


@pytest.mark.parametrize("name", sorted(K.OTHER_KERNELS))
def test_clip_counts_of_every_other_terminal_kernel(qrl_ctx, name):
    """bb_gain 4 on the handles whose terminal kernel is `name`: saturated output exact, counts[b] exact and non-zero, a second call adds"""
    import torch
    import qradiolink_amd as q
    make, x, refs = K.clip_case(name)
    K.clip_case_preconditions(refs)
    count = refs[0].size
    want = [conv8(r)[1] for r in refs]
    h = make(q, qrl_ctx)
    clip = _counters(torch)
    h.set_sc8_clip_counts(clip)
    buf = _buffer(torch, count)
    d = torch.from_numpy(x).cuda()
    view = _run(q, h, d, buf)
    assert check_rows(buf.cpu().numpy(), view, refs) == want
    assert clip.cpu().numpy().tolist() == want
    if isinstance(h, q.Mod):
        h.reset()                                                      # the same stream again: the same count on top
        h.process_sc8(d)
        assert clip.cpu().numpy().tolist() == [2 * c for c in want]
    h.close()


# ---- scale
def test_set_sc8_scale(qrl_ctx):
    """64 is exact; 0, inf and nan are refused and leave 64 in force; the default is 127"""
    import torch
    import qradiolink_amd as q
    data, refs = S16.mod_case("qpsk250k")
    n = data.shape[1]
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=n)
    mod.set_sc8_scale(64.0)
    mod.set_sc16_scale(2048.0)                                         # a scale of its own: the int16 one is not it
    d = torch.from_numpy(data).cuda()
    k = 30
    buf = _buffer(torch, k * 32)
    view = _run(q, mod, d[:, :k].contiguous(), buf)
    check_rows(buf.cpu().numpy(), view, [x[:k * 32] for x in refs], scale=64.0)
    for bad in (0.0, float("inf"), float("-inf"), float("nan")):
        assert mod.lib.qrl_mod_set_sc8_scale(mod.h, C.c_float(bad)) == QRL_ERR_ARG
        with pytest.raises(q.QrlError):
            mod.set_sc8_scale(bad)
    buf = _buffer(torch, (n - k) * 32)
    view = _run(q, mod, d[:, k:].contiguous(), buf)
    check_rows(buf.cpu().numpy(), view, [x[k * 32:] for x in refs], scale=64.0)
    mod.close()
    for cls_args in ((q.AMod, (NBFM5000,), dict(batch=1, max_samples=8)), (q.Synth, (1,), dict(batch=1, max_samples=8))):
        h = cls_args[0](qrl_ctx, *cls_args[1], **cls_args[2])
        h.set_sc8_scale(64.0)
        for bad in (0.0, float("inf"), float("nan")):
            with pytest.raises(q.QrlError):
                h.set_sc8_scale(bad)
        h.close()


# ---- NaN
def test_nan_gives_zero_and_is_not_counted(qrl_ctx):
    import torch
    import qradiolink_amd as q
    data, _ = S16.mod_case("qpsk250k")
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=data.shape[1])
    mod.set_bb_gain(float("nan"))
    clip = _counters(torch)
    mod.set_sc8_clip_counts(clip)
    count = data.shape[1] * 32
    buf = _buffer(torch, count)
    view = _run(q, mod, torch.from_numpy(data).cuda(), buf)
    out = buf.cpu().numpy()
    assert view.shape == (B, count, 2)
    assert np.all(out[:, :count] == 0) and np.all(out[:, count:] == SENTINEL)
    assert clip.cpu().numpy().tolist() == [0] * B
    mod.close()


# ---- the format belongs to the call: cuts, alternation, retune
def test_mod_alternating_formats_chunks_and_retune(qrl_ctx):
    """QPSK250K at 5 Msps, +10 kHz, ragged cuts [100, 1, 333, 66, 7, 29] with a retune to -30 kHz before the third; calls sc8, cf32, sc16, sc8, sc16, cf32:
    every piece is the one-piece oracle stream's piece in the call's format"""
    import torch
    import qradiolink_amd as q
    cuts = [100, 1, 333, 66, 7, 29]
    fmts = ["sc8", "cf32", "sc16", "sc8", "sc16", "cf32"]
    data = S16._bytes(500, sum(cuts))
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=max(cuts), device_samp_rate=5000000, carrier_offset_hz=10000.0)
    d = torch.from_numpy(data).cuda()
    parts, pos = [], 0
    for i, c in enumerate(cuts):
        if i == 2:
            mod.set_carrier_offset(-30000.0)
        blk = d[:, pos:pos + c].contiguous()
        parts.append({"sc8": mod.process_sc8, "sc16": mod.process_sc16, "cf32": mod.process}[fmts[i]](blk).cpu().numpy())
        pos += c
    mod.close()
    k = (cuts[0] + cuts[1]) * 32
    inc0 = orc.phase_inc_to_turn(2 * np.pi * 10000.0 / 1e6)
    inc1 = orc.phase_inc_to_turn(2 * np.pi * -30000.0 / 1e6)
    e = np.cumsum([0] + cuts) * 160
    for b in range(B):
        x1 = orc.mod_qpsk(data[b])
        rot = np.concatenate([orc.rotator(x1[:k], inc0), orc.rotator(x1[k:], inc1, (k * inc0) & (2 ** 64 - 1))])
        want = orc.tx_interp(rot, 5000000)
        for i, f in enumerate(fmts):
            w = want[e[i]:e[i + 1]]
            got = parts[i][b]
            if f == "cf32":
                assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), "stream %d, call %d (cf32) differs" % (b, i)
            else:
                ref = conv8(w)[0] if f == "sc8" else S16.conv(w)[0]
                assert got.shape == ref.shape and np.array_equal(got, ref), "stream %d, call %d (%s) differs" % (b, i, f)


def test_amod_alternating_formats_chunks(qrl_ctx):
    """NBFM at 4 Msps, chunks [1000, 324, 8, 1000], calls sc8, cf32, sc16, sc8"""
    import torch
    import qradiolink_amd as q
    cuts = [1000, 324, 8, 1000]
    fmts = ["sc8", "cf32", "sc16", "sc8"]
    audio = S16._audio(501, sum(cuts))
    mod = q.AMod(qrl_ctx, NBFM5000, batch=B, max_samples=max(cuts), device_samp_rate=4000000, carrier_offset_hz=25000.0)
    a = torch.from_numpy(audio).cuda()
    parts, pos = [], 0
    for i, c in enumerate(cuts):
        blk = a[:, pos:pos + c].contiguous()
        y = {"sc8": mod.process_sc8, "sc16": mod.process_sc16, "cf32": mod.process}[fmts[i]](blk).cpu().numpy()
        parts.append(np.stack([conv8(y[b])[0] for b in range(B)]) if fmts[i] == "cf32" else y)
        pos += c
    mod.close()
    e = np.cumsum([0] + cuts) * 500
    for b in range(B):
        want = S16.back_end(orc.mod_nbfm(audio[b], filter_width=5000), 4000000, 25000.0)
        for i, f in enumerate(fmts):
            w = want[e[i]:e[i + 1]]
            ref = S16.conv(w)[0] if f == "sc16" else conv8(w)[0]
            assert parts[i][b].shape == ref.shape and np.array_equal(parts[i][b], ref), "stream %d, call %d (%s) differs" % (b, i, f)


# ---- alignment
def test_a_base_moved_by_one_sample_gives_the_same_rows(qrl_ctx):
    """iq = a 4-byte aligned base + 2 bytes: accepted, and with an even pitch EVERY row starts at an address = 2 mod 4"""
    import torch
    import qradiolink_amd as q
    data, refs = S16.mod_case("qpsk250k")
    n = data.shape[1]
    count = n * 32
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=n)
    d = torch.from_numpy(data).cuda()
    whole = torch.full((B * (count + 4) + 2, 2), SENTINEL, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    assert whole.data_ptr() % 4 == 0
    assert mod.lib.qrl_mod_process_sc8(mod.h, d.data_ptr(), d.stride(0), n, whole.data_ptr() + 2, count + 4) == 0
    mod.sync()
    out = whole.cpu().numpy()
    assert np.all(out[0] == SENTINEL) and np.all(out[-1] == SENTINEL)
    rows = out[1:-1].reshape(B, count + 4, 2)
    for b in range(B):
        assert np.array_equal(rows[b, :count], conv8(refs[b])[0]), "stream %d differs" % b
        assert np.all(rows[b, count:] == SENTINEL)
    mod.close()


def test_odd_byte_address_is_refused_and_the_handle_goes_on(qrl_ctx):
    import torch
    import qradiolink_amd as q
    data, refs = S16.mod_case("qpsk250k")
    n = data.shape[1]
    count = n * 32
    mod = q.Mod(qrl_ctx, QPSK250K, batch=B, max_bytes=n)
    d = torch.from_numpy(data).cuda()
    buf = _buffer(torch, count)
    torch.cuda.synchronize()
    assert mod.lib.qrl_mod_process_sc8(mod.h, d.data_ptr(), d.stride(0), n, buf.data_ptr() + 1, count + 2) == QRL_ERR_ARG
    mod.sync()
    assert np.all(buf.cpu().numpy() == SENTINEL)
    view = _run(q, mod, d, buf)                                       # nothing was consumed: the stream starts here
    check_rows(buf.cpu().numpy(), view, refs)
    mod.close()
    amod = q.AMod(qrl_ctx, NBFM5000, batch=1, max_samples=8)
    a = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
    o = torch.zeros((1, 1000 + 1, 2), dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    assert amod.lib.qrl_amod_process_sc8(amod.h, a.data_ptr(), 8, 8, o.data_ptr() + 1, 1000) == QRL_ERR_ARG
    amod.close()
    syn = q.Synth(qrl_ctx, 1, batch=1, max_samples=24, single_carrier=True)
    x = torch.zeros((1, 1, 24), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert syn.lib.qrl_synth_process_sc8(syn.h, x.data_ptr(), 24, 24, o.data_ptr() + 1, 1000, None) == QRL_ERR_ARG
    syn.close()
