"""DMR layer 2 on the GPU (kernels_dmr_l2.hip through qrl_dmr_l2_decode / qrl_dmr_trellis34_*): the reference's recorded records
(tests/golden/ref/dmr_l2.npz) and the restatement of tests/dmr_l2.py are the expected values; the reference itself is not read here."""
import ctypes as C

import numpy as np
import pytest

import dmr_l2
import orc
import sig

pytestmark = pytest.mark.gpu
INPUTS, AUDIO_FEC, GROUP, RECORDS = dmr_l2.load_golden()
GUARD = 256


def _decode_guarded(ctx, frames, counts, audio_fec):
    """qrl_dmr_l2_decode into the middle of a buffer of 0xA5: -> records [batch, cap, 80]; the bytes around them must stay 0xA5"""
    import torch
    batch, cap = frames.shape[:2]
    d_in = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    d_cnt = torch.from_numpy(np.asarray(counts, np.int32)).cuda() if counts is not None else None
    buf = torch.full((GUARD + batch * cap * 80 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.qrl_dmr_l2_decode(ctx.h, None, d_in.data_ptr(), d_cnt.data_ptr() if d_cnt is not None else None, batch, cap, int(audio_fec),
                                   buf.data_ptr() + GUARD)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all(), "wrote outside the output"
    return host[GUARD:-GUARD].reshape(batch, cap, 80)


def _expected(index, counts, cap):
    """records of the golden rows index[b, i] where i < min(counts[b], cap), zeros elsewhere"""
    want = np.zeros(index.shape + (80,), np.uint8)
    for b in range(index.shape[0]):
        n = cap if counts is None else min(int(counts[b]), cap)
        want[b, :n] = RECORDS[index[b, :n]]
    return want


@pytest.mark.parametrize("audio_fec", [0, 1])
def test_golden_set_through_the_mailbox(qrl_ctx, audio_fec):
    """every golden record, 16 to a stream; streams with counts of 0, below, at and above cap_frames: slots past the count come back as
    zeros although the mailbox holds records there, and a count above the cap writes nothing beyond the stream's own slots"""
    cap = 16
    rows = np.nonzero(AUDIO_FEC == audio_fec)[0]
    batch = (rows.size + cap - 1) // cap
    index = np.resize(rows, batch * cap).reshape(batch, cap)
    counts = np.full(batch, cap, np.int32)
    counts[1::7] = 0
    counts[2::7] = 5
    counts[3::7] = cap + 9
    counts[4::7] = 15
    counts[5::7] = 1
    got = _decode_guarded(qrl_ctx, INPUTS[index], counts, audio_fec)
    want = _expected(index, counts, cap)
    bad = np.nonzero((got != want).any(axis=2))
    assert bad[0].size == 0, "records (stream, slot) %s differ" % list(zip(*bad))[:8]
    assert {0, 5, cap, cap + 9} <= set(counts.tolist()) and len(set(RECORDS[index[counts >= cap]][..., 3].ravel())) == 18


def _mixed(n):
    """n golden rows of mixed types (audio FEC on) with searched rate 3/4 bursts at positions 0, 3, 4 and last"""
    pool = np.nonzero(AUDIO_FEC == 1)[0]
    searched = np.nonzero((AUDIO_FEC == 1) & (GROUP == 1) & (RECORDS[:, 3] == 8))[0][64:]      # past the clean ones: damaged and garbage
    rows = pool[(np.arange(n) * 37) % pool.size].copy()
    for k, pos in enumerate(p for p in (0, 3, 4, n - 1) if p < n):
        rows[pos] = searched[(5 * k + n) % searched.size]
    return rows


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_record_counts_around_the_lane_grouping(qrl_ctx, n):
    """four bursts per wave in the search, 64 slots per wave in the dispatch kernel: counts at and around both edges, counts = NULL"""
    rows = _mixed(n)
    got = _decode_guarded(qrl_ctx, INPUTS[rows][None], None, 1)
    assert np.array_equal(got[0], RECORDS[rows])
    assert RECORDS[rows[0], 3] == 8 and RECORDS[rows[-1], 3] == 8


def test_batched_mailboxes(qrl_ctx):
    rows = _mixed(24).reshape(3, 8)
    counts = np.array([0, 5, 11], np.int32)
    assert np.array_equal(_decode_guarded(qrl_ctx, INPUTS[rows], counts, 1), _expected(rows, counts, 8))
    rows = _mixed(140).reshape(70, 2)          # more streams than a wave has lanes
    counts = (np.arange(70) * 5 % 4).astype(np.int32)
    assert np.array_equal(_decode_guarded(qrl_ctx, INPUTS[rows], counts, 1), _expected(rows, counts, 2))
    assert set(counts.tolist()) == {0, 1, 2, 3}


def test_4096_fresh_records_against_the_restatement(qrl_ctx):
    """golden inputs with up to five more bit flips anywhere in the burst: new syndromes, new slot types, new search paths"""
    rng = np.random.RandomState(4096)
    rows = rng.randint(0, INPUTS.shape[0], 4096)
    rows[GROUP[rows] == 1] = rng.randint(0, 2560, int((GROUP[rows] == 1).sum()))     # keep the garbage share small for the Python side
    fresh = INPUTS[rows].copy()
    for i in range(fresh.shape[0]):
        for bit in rng.randint(0, 264, rng.randint(0, 6)):
            fresh[i, 4 + (bit >> 3)] ^= 0x80 >> (bit & 7)
    got = _decode_guarded(qrl_ctx, fresh.reshape(64, 64, 40), None, 1).reshape(-1, 80)
    want = dmr_l2.records(fresh, 1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "records %s differ from the restatement" % bad[:8]
    assert (want[:, 3] == 8).sum() >= 100 and len(set(want[:, 3])) == 18


def test_trellis34_encode_flips_decode(qrl_ctx):
    import torch
    import qradiolink_amd as q
    rng = np.random.RandomState(34)
    n = 515
    payloads = rng.randint(0, 256, (n, 18)).astype(np.uint8)
    base = rng.randint(0, 256, (n, 33)).astype(np.uint8)
    bursts = q.dmr_trellis34_encode(qrl_ctx, torch.from_numpy(payloads).cuda(), torch.from_numpy(base).cuda()).cpu().numpy()
    for i in range(n):
        bits = dmr_l2.to_bits(base[i])
        dmr_l2.trellis_encode(payloads[i], bits)
        assert bytes(dmr_l2.to_bytes(bits)) == bursts[i].tobytes(), i
    middle = np.unpackbits(bursts, axis=1)[:, 98:166]
    assert np.array_equal(middle, np.unpackbits(base, axis=1)[:, 98:166])       # the 68 middle bits are left alone
    damaged = bursts.copy()
    for i in range(n):
        if i % 16 == 15:
            damaged[i] = rng.randint(0, 256, 33)      # garbage: the long searches
        else:
            dmr_l2.flip(damaged[i], dmr_l2.INFO_BITS, i % 5, rng)
    got_p, got_ok = q.dmr_trellis34_decode(qrl_ctx, torch.from_numpy(damaged).cuda())
    got_p, got_ok = got_p.cpu().numpy(), got_ok.cpu().numpy()
    right = 0
    for i in range(n):
        want = dmr_l2.trellis_decode(dmr_l2.to_bits(damaged[i]))
        assert got_ok[i] == (want is not None), i
        assert got_p[i].tobytes() == (bytes(want) if want is not None else bytes(18)), i
        right += got_p[i].tobytes() == payloads[i].tobytes()
    assert right >= n // 2
    empty_p, empty_ok = q.dmr_trellis34_decode(qrl_ctx, torch.zeros((0, 33), dtype=torch.uint8, device="cuda"))
    assert empty_p.shape == (0, 18) and empty_ok.shape == (0,)


SRC, DST, CC = 2261234, 91, 6


def _call(rng):
    """LC header, six voice frames, terminator, a data header with two rate 3/4 and one rate 1/2 continuation, a CSBK: properly encoded"""
    def data(block_bits, dt):
        return sig.dmr_frame(block_bits, sig.DMR_MS_DATA_SYNC, CC, dt)

    sync = [(sig.DMR_MS_VOICE_SYNC >> (47 - i)) & 1 for i in range(48)]
    frames = [data(dmr_l2.info_bits_bptc(dmr_l2.lc_block(0, 0, 0, DST, SRC, 1)), 1)]
    frames.append(sig.dmr_frame(dmr_l2.voice_bits(rng, sync)))
    for fn in range(1, 6):
        e = dmr_l2.emb_word(CC, 0, (1, 3, 3, 2, 0)[fn - 1])
        frames.append(sig.dmr_frame(dmr_l2.voice_bits(rng, e[:8] + [int(v) for v in rng.integers(0, 2, 32)] + e[8:])))
    frames.append(data(dmr_l2.info_bits_bptc(dmr_l2.lc_block(0, 0, 0, DST, SRC, 2)), 2))
    hdr = bytearray(rng.integers(0, 256, 10).astype(np.uint8).tobytes())
    hdr[0] = 0x82                                                  # group, unconfirmed data
    hdr[2:5], hdr[5:8] = DST.to_bytes(3, "big"), SRC.to_bytes(3, "big")
    frames.append(data(dmr_l2.info_bits_bptc(dmr_l2.crc_block(hdr, 0xCCCC)), 6))
    payloads = [bytearray(rng.integers(0, 256, 18).astype(np.uint8).tobytes()) for _ in range(2)]
    frames += [data(dmr_l2.info_bits_rate34(p), 8) for p in payloads]
    half = bytearray(rng.integers(0, 256, 12).astype(np.uint8).tobytes())
    frames.append(data(dmr_l2.info_bits_bptc(half), 7))
    csbk = bytearray([0x80 | 0x3D, 0, 0x40, 3]) + DST.to_bytes(3, "big") + SRC.to_bytes(3, "big")     # preamble CSBK
    frames.append(data(dmr_l2.info_bits_bptc(dmr_l2.crc_block(csbk, 0xA5A5)), 3))
    return frames, payloads, half


def test_receiver_to_layer2_end_to_end(qrl_ctx):
    """IQ of a properly encoded call -> gr_demod_dmr chain -> DMO slicer -> layer 2, all on the handle's stream, in three ragged calls"""
    import torch
    import qradiolink_amd as q
    rng = np.random.default_rng(2024)
    frames, payloads, half = _call(rng)
    x, _ = sig.make_4fsk(levels=sig.dmr_levels(frames), seed=3, cfo=20.0)
    n = x.size & ~1
    iq = np.stack([x[:n], np.roll(x[:n], 2000)])
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=2, max_chunk=n)
    dem.enable_dmo_sink(cap_frames=16)
    dem.enable_dmo_l2(audio_fec=True)
    d = torch.from_numpy(iq).cuda()
    cuts = [0, 233334, 233334 + 401110, n]
    got = [[], []]
    for a, b in zip(cuts[:-1], cuts[1:]):
        dem.process(d[:, a:b].contiguous())
        cnt, l2 = dem.dmo_counts.cpu().numpy(), dem.dmo_l2.cpu().numpy()
        for s in range(2):
            assert not l2[s, min(int(cnt[s]), 16):].any()
            got[s].extend(l2[s, i].tobytes() for i in range(min(int(cnt[s]), 16)))
    dem.close()
    for s in range(2):
        sliced = orc.DmoSink().process(orc.demod_dmr_port3(iq[s]))
        assert len(sliced) == len(frames)
        want = [bytes(dmr_l2.record(bytes([t, fn, cc, 0]) + burst + bytes(3), 1)) for t, fn, cc, burst in sliced]
        assert got[s] == want, "stream %d: records differ from the restatement of the oracle's slicer records" % s
        recs = np.frombuffer(b"".join(want), np.uint8).reshape(-1, 80)
        assert list(recs[:, 3]) == [1, 0xF0] + [0xF1] * 5 + [2, 6, 8, 8, 7, 3] and recs[:, 4].all()
        for i in (0, 7, 8, 12):     # LC header, terminator, data header, CSBK: the IDs that were sent
            assert int.from_bytes(recs[i, 12:16].tobytes(), "little") == SRC and int.from_bytes(recs[i, 16:20].tobytes(), "little") == DST
        assert list(recs[[0, 7, 8, 12], 2]) == [CC] * 4 and list(recs[2:7, 2]) == [CC] * 5 and list(recs[2:7, 7]) == [1, 3, 3, 2, 0]
        # the slicer reads a burst's last dibit one lap early (tests/test_dmo_sink.py): BPTC corrects that bit; of a rate 3/4 burst it is the
        # last point sent, which carries tribit 47 = the top three bits of payload byte 0, and the search may settle on another tribit there
        for k in range(2):
            assert recs[9 + k, 54:71].tobytes() == bytes(payloads[k][1:]) and (recs[9 + k, 53] ^ payloads[k][0]) & 0x1F == 0
        assert recs[11, 53:65].tobytes() == bytes(half)
        assert recs[12, 9] == 0x3D and not recs[1:7, 5].any()
