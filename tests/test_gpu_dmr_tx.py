"""DMR layer 2 transmit on the GPU (kernels_dmr_tx.hip through qrl_dmr_l2_encode / qrl_dmr_voice_call_encode): the reference's recorded
bursts (tests/golden/ref/dmr_tx.npz) are the expected values, the reference itself is not read here.  Then the device's own decoder
(qrl_dmr_l2_decode) on what the encoder built, and the radio path: encoder -> DMR modulator -> DMR receiver -> DMO slicer -> layer 2 against
the oracle's chain on the same bytes."""
import numpy as np
import pytest

import dmr_l2
import dmr_tx
import orc

pytestmark = pytest.mark.gpu
G = dmr_tx.load_golden()
RECORDS, BURSTS, CALLS, VOICE = G["records"], G["bursts"], G["calls"], G["call_voice"]
NV = dmr_tx.CALL_VOICE
CALL_BURSTS = np.stack([dmr_tx.call_voice_frames(G, m) for m in range(CALLS.shape[0])])
GUARD, FILL = 256, 0xA5


def _guarded(call, batch, slots, slot_bytes, pad, shift):
    """run call(out pointer, out_stride) on rows of slots * slot_bytes + pad bytes inside a buffer of 0xA5, the first row `shift` bytes off a
    256-byte boundary -> rows [batch, slots, slot_bytes]; the pad bytes of every row and the bytes around the rows must stay 0xA5"""
    import torch
    stride = slots * slot_bytes + pad
    buf = torch.full((GUARD + shift + batch * stride + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert call(buf.data_ptr() + GUARD + shift, stride) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD + shift] == FILL).all() and (host[-GUARD:] == FILL).all(), "wrote outside the output"
    rows = host[GUARD + shift:-GUARD].reshape(batch, stride)
    assert (rows[:, slots * slot_bytes:] == FILL).all(), "wrote behind cap_frames * slot_bytes of a row"
    return rows[:, :slots * slot_bytes].reshape(batch, slots, slot_bytes)


def _encode(ctx, index, counts, slot_bytes, pad=0, shift=0):
    """golden records index[b, i] through qrl_dmr_l2_encode"""
    import torch
    batch, cap = index.shape
    d_rec = torch.from_numpy(np.ascontiguousarray(RECORDS[index])).cuda()
    d_cnt = torch.from_numpy(np.asarray(counts, np.int32)).cuda() if counts is not None else None
    return _guarded(lambda out, stride: ctx.lib.qrl_dmr_l2_encode(ctx.h, None, d_rec.data_ptr(), d_cnt.data_ptr() if d_cnt is not None else None,
                                                                  batch, cap, out, stride, slot_bytes), batch, cap, slot_bytes, pad, shift)


def _expected(index, counts, slot_bytes):
    batch, cap = index.shape
    want = np.zeros((batch, cap, slot_bytes), np.uint8)
    for b in range(batch):
        n = cap if counts is None else min(int(counts[b]), cap)
        want[b, :n, :33] = BURSTS[index[b, :n]]
    return want


def _differing(got, want):
    bad = np.nonzero((got != want).any(axis=2))
    return list(zip(*bad))[:8]


@pytest.mark.parametrize("slot_bytes", [33, 35, 36, 72])
def test_every_golden_record(qrl_ctx, slot_bytes):
    """all records, seven to a stream; 33 and 35 take the byte path, 36 and 72 whole dwords; the idle bytes behind a burst are zeros"""
    cap = 7
    batch = (RECORDS.shape[0] + cap - 1) // cap
    index = np.resize(np.arange(RECORDS.shape[0]), batch * cap).reshape(batch, cap)
    got = _encode(qrl_ctx, index, None, slot_bytes)
    assert not _differing(got, _expected(index, None, slot_bytes)), "bursts (stream, slot) differ from the reference's"
    assert not got[:, :, 33:].any()


@pytest.mark.parametrize("slot_bytes", [33, 35, 36, 72])
@pytest.mark.parametrize("batch,cap", [(1, 1), (3, 5), (1, 65), (72, 7)])
def test_shapes_counts_and_strides(qrl_ctx, batch, cap, slot_bytes):
    """the slot -> lane -> dword mapping at one slot, a few, one past a wave in one stream, and more streams than a wave has lanes; counts
    of 0, below, at and above cap_frames; rows 8 bytes longer than their slots (the dword path keeps its alignment), 5 bytes longer and a
    first row one byte off alignment (both force single bytes whatever slot_bytes is)"""
    rng = np.random.RandomState(1000 * batch + 10 * cap + slot_bytes)
    index = rng.randint(0, RECORDS.shape[0], (batch, cap))
    counts = rng.randint(0, cap + 1, batch).astype(np.int32)
    counts[0] = cap + 9
    if batch > 2:
        counts[1], counts[2] = 0, cap
    for pad, shift, cnt in ((8, 0, counts), (5, 0, counts), (0, 1, counts), (0, 0, None)):
        got = _encode(qrl_ctx, index, cnt, slot_bytes, pad, shift)
        assert not _differing(got, _expected(index, cnt, slot_bytes)), "pad %d shift %d" % (pad, shift)


def _call_encode(ctx, calls, voice, first, slot_bytes, pad=0):
    import torch
    batch, n = voice.shape[:2]
    d_calls, d_voice = torch.from_numpy(np.ascontiguousarray(calls)).cuda(), torch.from_numpy(np.ascontiguousarray(voice)).cuda()
    d_first = torch.from_numpy(np.asarray(first, np.int32)).cuda() if first is not None else None
    return _guarded(lambda out, stride: ctx.lib.qrl_dmr_voice_call_encode(ctx.h, None, d_calls.data_ptr(), d_voice.data_ptr(),
                                                                          d_first.data_ptr() if d_first is not None else None, batch, n, out,
                                                                          stride, slot_bytes), batch, n, slot_bytes, pad, 0)


@pytest.mark.parametrize("slot_bytes", [33, 72])
def test_every_golden_call(qrl_ctx, slot_bytes):
    """31 voice bursts per call: superframes 0..4 (the call's LC, the talker-alias header and blocks) and the wrap back to 0"""
    got = _call_encode(qrl_ctx, CALLS, VOICE, None, slot_bytes, pad=4)
    assert not _differing(got[:, :, :33], CALL_BURSTS) and not got[:, :, 33:].any()


def test_calls_in_cuts_and_from_other_first_bursts(qrl_ctx):
    """first = 0, n = 31 in cuts of 1, 5, 6 and 19 bursts; then every stream from another first burst; then 65 bursts of one call in one stream"""
    m = CALLS.shape[0]
    first = 0
    for n in (1, 5, 6, 19):
        got = _call_encode(qrl_ctx, CALLS, VOICE[:, first:first + n], np.full(m, first), 36)
        assert not _differing(got[:, :, :33], CALL_BURSTS[:, first:first + n]), "cut at %d" % first
        first += n
    starts = np.arange(m) % 12
    voice = np.stack([VOICE[b, starts[b]:starts[b] + 19] for b in range(m)])
    want = np.stack([CALL_BURSTS[b, starts[b]:starts[b] + 19] for b in range(m)])
    assert not _differing(_call_encode(qrl_ctx, CALLS, voice, starts, 33)[:, :, :33], want)
    # bursts 30 + k and k of a call carry the same superframe: 65 slots of one stream from first = 30 repeat the recorded 31, twice and a bit
    k = (30 + np.arange(65)) % 30
    got = _call_encode(qrl_ctx, CALLS[3:4], VOICE[3:4, k], [30], 72)
    assert not _differing(got[:, :, :33], CALL_BURSTS[3:4, k])
    big = 6 * 5 * 1000000 + 7                                      # far into a call: FN 1 of superframe 1
    got = _call_encode(qrl_ctx, CALLS[3:4], VOICE[3:4, 7:9], [big], 33)
    assert not _differing(got[:, :, :33], CALL_BURSTS[3:4, 7:9])


def _loopback(ctx, bursts, ftype, fn, cc):
    """device bursts [n, 33] -> 40-byte DMO records with torch ops -> qrl_dmr_l2_decode -> records [n, 80] on the host"""
    import torch
    import qradiolink_amd as q
    n = bursts.shape[0]
    rec = torch.zeros((1, n, 40), dtype=torch.uint8, device="cuda")
    rec[0, :, 0], rec[0, :, 1], rec[0, :, 2] = ftype, fn, cc
    rec[0, :, 4:37] = bursts
    return q.dmr_l2_decode(ctx, rec, None, audio_fec=False)[0].cpu().numpy()


def test_device_decoder_returns_what_the_encoder_was_given(qrl_ctx):
    import torch
    import qradiolink_amd as q
    d_rec = torch.from_numpy(RECORDS[None]).cuda()
    bursts = q.dmr_l2_encode(qrl_ctx, d_rec)[0]
    kind = d_rec[0, :, 0]
    ftype = torch.where(kind == dmr_tx.K_VOICE_SYNC, 2, torch.where(kind == dmr_tx.K_VOICE, 1, 0)).to(torch.uint8)
    rec = _loopback(qrl_ctx, bursts, ftype, d_rec[0, :, 1], d_rec[0, :, 2] & 15)
    assert np.array_equal(rec[:, 20:53][(RECORDS[:, 0] >= 1) & (RECORDS[:, 0] <= 8)], BURSTS[(RECORDS[:, 0] >= 1) & (RECORDS[:, 0] <= 8)])
    kind, cc, dt = RECORDS[:, 0], RECORDS[:, 2] & 15, RECORDS[:, 3] & 15
    data = (kind >= 1) & (kind <= 5) & ~((kind == 1) & (dt != 1) & (dt != 2))
    assert rec[data, 4].all() and np.array_equal(rec[data, 2], cc[data]) and np.array_equal(rec[data, 3], dt[data])
    for i in np.nonzero(data)[0]:
        r, pay = RECORDS[i], rec[i, 53:80]
        if kind[i] == dmr_tx.K_LC:
            assert bytes(pay[:9]) == bytes(r[4:13]) and (rec[i, 9], rec[i, 10]) == (r[4] & 0x3F, r[5])
            assert int.from_bytes(bytes(rec[i, 12:16]), "little") == int.from_bytes(bytes(r[10:13]), "big")
            assert int.from_bytes(bytes(rec[i, 16:20]), "little") == int.from_bytes(bytes(r[7:10]), "big")
        elif kind[i] == dmr_tx.K_CSBK:
            assert bytes(pay[:10]) == bytes(r[16:26]) and rec[i, 9] == r[16] & 0x3F and rec[i, 10] == r[17]
        elif kind[i] == dmr_tx.K_DATA_HEADER:
            want = bytearray(r[16:26])
            if want[0] & 15 == 0:
                want[9] &= 0xFE
            assert bytes(pay[:10]) == bytes(want)
        elif kind[i] == dmr_tx.K_RATE12:
            assert rec[i, 8] == 12 and bytes(pay[:12]) == bytes(r[16:28])
        else:
            assert rec[i, 8] == 18 and bytes(pay[:18]) == bytes(r[16:34])
    voice = (kind == dmr_tx.K_VOICE_SYNC) | (kind == dmr_tx.K_VOICE)
    assert np.array_equal(rec[voice, 53:80], RECORDS[voice, 16:43]) and np.array_equal(rec[voice, 2], cc[voice]) and rec[voice, 4].all()
    fn = RECORDS[:, 1].astype(int)
    lcss = np.where(kind == dmr_tx.K_VOICE, np.select([fn == 1, fn == 4, (fn == 2) | (fn == 3)], [1, 2, 3], 0), 0)
    assert np.array_equal(rec[voice, 7], lcss[voice]) and not rec[voice, 6].any()


def test_device_decoder_on_whole_calls_and_their_embedded_lc(qrl_ctx):
    """every voice burst of every call back through the decoder: its 27 bytes, the EMB's colour code and LCSS as the sequencing prescribes;
    the four fragments of each complete superframe reassemble to the nine LC bytes of that superframe"""
    import torch
    import qradiolink_amd as q
    m = CALLS.shape[0]
    bursts = q.dmr_voice_call_encode(qrl_ctx, torch.from_numpy(CALLS).cuda(), torch.from_numpy(VOICE).cuda())
    k = np.arange(m * NV) % NV
    fn = torch.from_numpy((k % 6).astype(np.uint8)).cuda()
    ftype = torch.where(fn == 0, 2, 1).to(torch.uint8)
    cc = torch.from_numpy(np.repeat(CALLS[:, 8] & 15, NV)).cuda()
    rec = _loopback(qrl_ctx, bursts.reshape(m * NV, 33), ftype, fn, cc).reshape(m, NV, 80)
    assert np.array_equal(rec[:, :, 53:80], VOICE) and rec[:, :, 4].all()
    assert np.array_equal(rec[:, :, 2], np.repeat((CALLS[:, 8] & 15)[:, None], NV, axis=1))
    assert np.array_equal(rec[:, :, 7], np.tile(np.array([0, 1, 3, 3, 2, 0])[np.arange(NV) % 6], (m, 1)))
    for c in range(m):
        rule = q.dmr_voice_call_records(CALLS[c], NV)
        for s in range(NV // 6):
            lc, crc = dmr_tx.embedded_lc(rec[c, 6 * s + 1:6 * s + 5, 20:53])
            assert lc == bytes(rule[6 * s + 1, 4:13]) and crc == sum(lc) % 31, "call %d superframe %d" % (c, s)
    alias = bytes(CALLS[-1, 9:36])
    lcs = [dmr_tx.embedded_lc(rec[-1, 6 * s + 1:6 * s + 5, 20:53])[0] for s in range(5)]
    assert lcs[1][3:] + lcs[2][2:] == alias[:13] == b"YO8RZZ Adrian"          # header, block 1: the text of the alias in order


RADIO_CALLS, RADIO_VOICE = dmr_tx.RADIO_CALLS, dmr_tx.RADIO_VOICE


@pytest.mark.parametrize("zero_runs", [False, True])
def test_radio_loopback(qrl_ctx, zero_runs):
    """dmr_call_slots -> qrl_dmr_l2_encode -> qrl_mod_process (DMR, 1 Msps) -> DMR receiver with the DMO slicer and layer 2, two streams, one
    call of 2 LC headers + 12 voice bursts + 2 terminators + 2 empty frames each; without and with the zero runs dmr_call_slots returns.
    The device's 80-byte records equal the oracle chain's for the same bytes, bit for bit, and hold what dmr_tx.check_radio_records asks
    (tests/test_dmr_tx_conditions.py asks the same of the oracle alone): every voice burst with no gap, and what was encoded comes back --
    with the zero runs only what lies in front of the last 24 symbols of a burst, which the reference's gr_zero_idle_bursts blanks."""
    import torch
    import qradiolink_amd as q
    slots = [q.dmr_call_slots(CALLS[m], VOICE[m, :RADIO_VOICE], stream=s) for s, m in enumerate(RADIO_CALLS)]
    records = np.stack([r for r, _ in slots])
    n_slots = records.shape[1]
    assert n_slots == 2 + RADIO_VOICE + 4
    rows = q.dmr_l2_encode(qrl_ctx, torch.from_numpy(records).cuda(), slot_bytes=q.DMR_SLOT_BYTES).reshape(2, n_slots * 72)
    sent = rows.cpu().numpy()
    for s, m in enumerate(RADIO_CALLS):
        want_bytes, _, want_runs = dmr_tx.radio_call(G, m)
        assert np.array_equal(sent[s], want_bytes) and [(t, c) for _, t, c in slots[s][1]] == want_runs
    mod = q.Mod(qrl_ctx, q.MODEM_DMR, batch=2, max_bytes=rows.shape[1])
    if zero_runs:
        mod.add_zero_runs([run for _, runs in slots for run in runs])
    iq = (mod.process(rows) * 0.05).contiguous()
    mod.close()
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=2, max_chunk=iq.shape[1])
    dem.enable_dmo_sink(cap_frames=32)
    dem.enable_dmo_l2(audio_fec=False)
    dem.process(iq)
    cnt, l2 = dem.dmo_counts.cpu().numpy(), dem.dmo_l2.cpu().numpy()
    dem.close()
    for s, m in enumerate(RADIO_CALLS):
        runs = [(t, c) for _, t, c in slots[s][1]] if zero_runs else None
        sliced = orc.DmoSink().process(orc.demod_dmr_port3(orc.mod_dmr(sent[s], zero_runs=runs) * np.float32(0.05)))
        want = np.array([list(dmr_l2.record(bytes([t, fn, cc, 0]) + burst + bytes(3), 0)) for t, fn, cc, burst in sliced], np.uint8)
        assert int(cnt[s]) == want.shape[0] and np.array_equal(l2[s, :want.shape[0]], want), "stream %d: records differ from the oracle chain's" % s
        assert not l2[s, want.shape[0]:].any()
        dmr_tx.check_radio_records(G, l2[s, :int(cnt[s])], m, zero_runs)
