"""Each scenario of tests/golden/ref/dmr_sink.npz reaches the branch it is named for: asserted from the REFERENCE's recorded records and
private state alone (the sink, the call layer and their core headers do not run here), so that the byte-for-byte tests of test_dmr_sink.py /
test_gpu_dmr_sink.py are known to compare the branches they claim to.  The last test is of another kind: it runs the project's oracle DMR
modulator and receiver (tests/orc.py), to show that the signal of the device test behind the demodulator carries sync words the sink can find.

Dropped: flush() in the middle of a data or voice-sync burst.  The reference then builds the DMRFrame from a _bit_buffer shorter than 288
bits and packFrame reads past its end (src/DMR/dmrframe.cpp:370-384 on the vector copied at :58): what it returns is whatever the heap
holds, so there is nothing to record.  flush() in the middle of a voice burst and in the middle of the search are defined and are here."""
import numpy as np

import dmr_rx
import dmr_sink

G = dmr_sink.load_golden()
NONE, VOICE = 0, 3
# a state row: per context (state, bits to receive, frames to receive, downlink, buffer size), then _next_slot


def S(name):
    return dmr_sink.scenario(G, name)


def test_1_downlink_alternates_the_slots():
    x, e = S("downlink_header_terminator")
    assert list(e["info"][:, 2]) == [1, 2, 1, 2, 1, 2] and e["info"][:, 0].all() and e["info"][:, 1].all() and not e["frames"][:, 0].any()
    assert [dmr_sink.end_bit(i) for i in e["info"]] == [288 * k for k in range(1, 7)]
    assert len(set(e["info"][:, 3])) > 1 and len(set(e["info"][:, 4])) > 1          # LCSS and AT both vary


def test_2_voice_superframe_numbers_its_bursts():
    _, e = S("voice_superframe")
    ts1 = e["info"][:, 2] == 1
    assert list(e["frames"][ts1, 0]) == [0, 2, 1, 1, 1, 1, 1, 0] and list(e["frames"][ts1, 1]) == [0, 0, 1, 2, 3, 4, 5, 0]
    assert not e["frames"][~ts1, 0].any() and (~ts1).sum() == 8


def test_3_a_searching_context_starves_the_others_voice_call():
    x, e = S("voice_both_slots")
    st = e["states"]
    starved = [c for c in range(len(st)) if st[c, 0] == NONE and st[c, 10] == 0 and st[c, 5] == VOICE and st[c, 7] == 5 and st[c, 4] >= 2 * 288]
    assert len(starved) > 5 and len(e["frames"]) < len(x.bits) // 288
    # and the erase at work()'s entry ran: the searching buffer shrank by 288 between two calls
    assert any(int(st[c + 1, 4]) == int(st[c, 4]) + x.cuts[c + 1] - 288 and st[c, 4] >= 864 for c in range(len(st) - 1))


def test_4_ms_sourced_sync():
    _, e = S("ms_sourced")
    assert list(e["frames"][:, 0]) == [0, 2, 0] and not e["info"][:, :5].any() and e["info"][:, 5:8].any()


def test_5_one_wrong_tact_bit():
    _, e = S("tact_bit_wrong")
    assert list(e["info"][:, 1]) == [0, 0, 0, 0, 1] and list(e["info"][:, 2]) == [0, 0, 0, 0, 2] and e["info"][:, 0].all()


def test_6_one_wrong_sync_bit_gives_no_burst():
    x, e = S("sync_bit_wrong")
    assert len(x.bits) == 3 * 288 and [dmr_sink.end_bit(i) for i in e["info"]] == [576, 864]


def test_7_sync_at_179_clears_and_at_180_is_taken():
    x, e = S("sync_at_179")
    assert [dmr_sink.end_bit(i) for i in e["info"]] == [575, 863]
    done = np.cumsum(x.cuts)
    c = int(np.nonzero(done >= 179)[0][0])
    assert e["states"][c, 0] == NONE and e["states"][c, 4] == done[c] - 179 and not e["counts"][:c + 1].any()   # the buffer began again at the sync
    _, e = S("sync_at_180")
    assert [dmr_sink.end_bit(i) for i in e["info"]] == [288, 576, 864]


def test_8_long_quiet_run():
    a, ea = S("long_quiet_one_call")
    b, eb = S("long_quiet_many_calls")
    assert np.array_equal(a.bits, b.bits) and len(a.cuts) == 1 and len(b.cuts) > 10 and not dmr_sink.has_sync(a.bits[:3 * 288 + 300])
    assert np.array_equal(ea["frames"], eb["frames"]) and np.array_equal(ea["info"], eb["info"]) and len(ea["frames"]) == 4
    st = eb["states"]
    assert any(st[c, 4] >= 864 and int(st[c + 1, 4]) == int(st[c, 4]) + b.cuts[c + 1] - 288 for c in range(len(st) - 1))   # trimmed under many calls
    assert dmr_sink.end_bit(ea["info"][0]) == 3 * 288 + 300 + 288                                                         # and never under one


def test_9_tiny_calls_across_a_sync_word_and_a_burst_end():
    x, e = S("tiny_calls")
    done = np.cumsum(x.cuts)
    call_at = lambda bit: int(np.nonzero(done >= bit)[0][0])       # the call that consumes the bit-th bit
    ends = [dmr_sink.end_bit(i) for i in e["info"]]
    assert {0, 1, 7} <= set(x.cuts)
    assert any(x.cuts[call_at(b)] <= 7 for b in ends) and any(x.cuts[call_at(b - 108)] <= 7 for b in ends)
    assert any(call_at(b - 108 - 47) != call_at(b - 108) for b in ends)      # a sync word that began in an earlier call


def test_10_five_bursts_under_a_cap_of_two():
    x, e = S("cap_two")
    assert x.cap == 2 and list(e["counts"]) == [5]


def test_11_flush_and_reset():
    x, e = S("flush_mid_voice")
    assert e["states"][0, 0] == VOICE and e["states"][0, 4] == 100 and e["states"][0, 10] == 0 and x.ops == {1: dmr_sink.FLUSH}
    after = e["call_of"] == 1
    assert e["frames"][after][0, 0] == 1 and e["info"][after][0, 1] == 0      # the voice burst went on from the flush: 288 bits from there, no CACH in front
    x, e = S("flush_in_search")
    assert e["states"][0, 0] == NONE and e["states"][0, 4] == 100 and [dmr_sink.end_bit(i) for i in e["info"]] == [576, 864]
    x, e = S("reset_mid_burst")
    assert e["states"][0, 0] == VOICE and e["states"][0, 4] == 100 and x.ops == {1: dmr_sink.RESET}


def test_12_tags_on_both_bits_of_a_symbol():
    x, e = S("tags")
    assert {t[0] & 1 for t in x.tags} == {0, 1} and len(e["timing"]) == 8
    assert any(int(t[2]) > 1700000000 * 10 ** 9 for t in e["timing"])


def R(name):
    x, want = dmr_sink.rx_scenario(G, name)
    return x, want, dmr_rx.flags(want)


REFUSED, OK = dmr_rx.VALID | dmr_sink.SLOT_REFUSED, dmr_rx.VALID | dmr_rx.PROCESSED


def test_13_fixed_timeslot():
    x, want, f = R("fixed_slot_1_calls_on_both")
    two = x.slots[:, 2] == 2
    assert (f[two] == REFUSED).all() and ((f[~two] & OK) == OK).all() and two.sum() == 8 and not want[:, 5].any()


def test_14_promiscuous_lock_and_release():
    x, want, f = R("promiscuous_slot_lock")
    assert list(want[:14:2, 5]) == [2] * 7 and (f[1:14:2] == REFUSED).all()              # locked to slot 2, slot 1 refused
    assert f[14] & dmr_rx.TERMINATOR and want[14, 5] == 0                                # released
    assert list(want[16:23, 5]) == [1] * 7 and ((f[16:] & OK) == OK).all() and list(want[24:31, 5]) == [2] * 7


def test_15_undecoded_cach():
    x, want, f = R("undecoded_cach_in_a_call")
    bad = x.slots[:, 1] == 0
    assert bad.sum() == 3 and (f[bad] == REFUSED).all() and ((f[~bad] & OK) == OK).all()


def test_16_the_order_of_the_checks():
    x, want, f = R("order_audio_fixed")
    assert list(f[:2]) == [dmr_rx.VALID] * 2 and (f[3:] & dmr_rx.AUDIO).all()        # passed the timeslot, refused by the colour code
    x, want, f = R("order_promiscuous")
    assert f[0] & dmr_rx.AUDIO and tuple(want[0, [3, 5]]) == (0, 2)                  # the audio call took the timeslot lock alone
    assert f[1] == REFUSED and tuple(want[1, [3, 5]]) == (5, 2)                      # the colour code locked, then the timeslot refused
    assert f[2] == dmr_rx.VALID and tuple(want[2, [3, 5]]) == (5, 2)                 # the colour code refused first
    assert f[3] == REFUSED                                                           # audio: the timeslot refused first


def test_17_mode_switched_with_the_state_carried():
    x, want, f = R("mode_switched")
    assert [r[3] for r in x.reconfig] == [dmr_sink.MODE_REPEATER, dmr_sink.MODE_DMO, dmr_sink.MODE_REPEATER]
    assert not x.slots[:8, 1].any() and ((f[:8] & OK) == OK).all()                   # DMO: an undecoded CACH does not matter
    assert list(want[8:12, 5]) == [2] * 4 and list(want[12:15, 5]) == [2] * 3 and want[12, 2] == 2   # the lock and the call survive the switch to DMO
    assert f[15] & dmr_rx.TERMINATOR and want[15, 5] == 0 and (f[24:] == REFUSED).all()


def test_the_oracle_receiver_delivers_an_exact_sync_word_on_each_slot():
    """the streams of test_gpu_dmr_sink.py's test behind the demodulator, through the oracle's DMR modulator and receiver at the test's
    level: port 2 holds exact BS sync words behind CACHs of both timeslots, so the sink has bursts to find there"""
    import orc
    for row in dmr_sink.radio_rows(G):
        bits = orc.demod_dmr(orc.mod_dmr(row) * np.float32(dmr_sink.RADIO_LEVEL))["bits_a"]
        tc = dmr_sink.sync_slots(bits)
        assert tc.count(0) >= 1 and tc.count(1) >= 1, tc
