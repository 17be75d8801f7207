"""The scenarios of tests/golden/ref/m17_link.npz reach the branches they are there for.  Everything here is asserted from the reference's own
recorded records and states; no code of the project runs.  A scenario that stopped reaching its branch (another frame builder, another
reference) fails here, not silently in the comparisons."""
import numpy as np

import m17_link as M

G = M.load_golden()
F = M


def _s(name):
    _, inp, want, states, can_rx, all_can, reconfig = M.scenario(G, name)
    return inp, want, M.flags(want), states


def _has(fl, bit):
    return (fl & bit) != 0


def test_lsf_then_stream():
    _, want, fl, states = _s("lsf_then_stream")
    assert want[0, 2] == 1 and fl[0] == F.FRAME | F.LSF_VALID | F.INFO | F.LOCKED
    assert all(want[1:9, 2] == 2) and all(_has(fl[1:9], F.AUDIO)) and not any(_has(fl[1:9], F.INFO))
    assert _has(fl[6], F.LSF_FROM_LICH) and int(_has(fl, F.LSF_FROM_LICH).sum()) == 1          # the sixth segment completes a round
    assert want[9, 2] == 0xFF and fl[9] == F.FRAME | F.INFO | F.END                             # unlocked, reset: the LSF is cleared
    assert M.texts(want[0]) == ("YO8RZZ", "AB1CDE") and M.texts(want[9]) == ("YO8RZZ", "AB1CDE")
    assert bytes(states[9][:6]) == b"\xff" * 6 and not states[9][6:30].any() and states[9][60] == 0 and states[9][61] == 0
    assert [int(r[4]) | int(r[5]) << 8 for r in want[1:9]] == list(range(8)) and [int(r[6]) for r in want[1:9]] == [0, 1, 2, 3, 4, 5, 0, 1]
    for i in range(1, 9):
        assert np.array_equal(want[i, 48:64], M.payload_of(i - 1))


def test_late_entry_locks_when_the_round_completes_from_every_phase():
    for phase in range(6):
        _, want, fl, states = _s("late_entry_phase_%d" % phase)
        assert not any(_has(fl[:5], F.LSF_VALID | F.AUDIO | F.INFO | F.LOCKED)) and all(_has(fl[:5], F.LICH_OK))
        assert fl[5] == F.FRAME | F.LSF_VALID | F.INFO | F.AUDIO | F.LICH_OK | F.LSF_FROM_LICH | F.LOCKED
        assert int(_has(fl[:9], F.INFO).sum()) == 1 and all(_has(fl[6:9], F.AUDIO))
        assert int(want[0, 6]) == phase and [int(r[7]) for r in want[:6]][-1] == 0 and int(want[4, 7]) != 0x3F
        assert M.texts(want[5]) == ("N0CALL-9", "W1AW/P") and want[5, 3] == 5


def test_uncorrectable_golay_word_stalls_the_map():
    _, want, fl, _ = _s("lich_golay_uncorrectable")
    assert not _has(fl[3], F.LICH_OK) and all(_has(fl[[0, 1, 2, 4, 5]], F.LICH_OK))
    assert int(want[5, 7]) == 0x37 and not any(_has(fl[:9], F.LSF_VALID))                     # six frames in, segment 3 is missing
    assert int(want[8, 7]) == 0x37 and _has(fl[9], F.LSF_FROM_LICH) and int(want[9, 6]) == 3 and int(want[9, 7]) == 0
    assert _has(fl[9], F.INFO) and _has(fl[10], F.AUDIO)


def test_completed_round_with_a_bad_crc_keeps_the_lsf():
    _, want, fl, states = _s("lich_round_bad_crc")
    assert int(want[5, 7]) == 0x1F and int(want[6, 7]) == 0 and not _has(fl[6], F.LSF_FROM_LICH)      # the round completed and was dropped
    assert all(_has(fl[1:15], F.AUDIO)) and M.texts(want[7]) == ("YO8RZZ", "AB1CDE")
    assert bytes(states[6][30:36]) == b"\xff" * 6 and not states[6][36:60].any()               # the image cleared: clear() leaves 0xFF
    assert int(_has(fl, F.LSF_FROM_LICH).sum()) == 1 and _has(fl[12], F.LSF_FROM_LICH) and M.texts(want[15]) == ("N0CALL-9", "W1AW/P")


def test_damaged_lsf_frame_stops_the_audio_until_a_round_restores_it():
    _, want, fl, _ = _s("damaged_lsf_over_valid")
    assert fl[4] == F.FRAME | F.LOCKED and want[4, 2] == 1                                     # still locked, the LSF gone
    assert not any(_has(fl[5:7], F.AUDIO | F.LSF_VALID)) and all(_has(fl[1:4], F.AUDIO))
    assert _has(fl[7], F.LSF_FROM_LICH | F.AUDIO) and not _has(fl[7], F.INFO)                  # restored; no second INFO: the lock held
    assert all(_has(fl[7:13], F.AUDIO))


def test_segment_numbers_6_and_7():
    for seg in (6, 7):
        _, want, fl, _ = _s("segment_%d" % seg)
        assert int(want[2, 6]) == seg and _has(fl[2], F.LICH_OK) and int(want[2, 7]) == 0x03 | (1 << seg)
        assert not any(_has(fl[:10], F.LSF_FROM_LICH)) and int(want[9, 7]) == 0x3F | (1 << seg)       # every segment in, and the map is not 0x3F
        assert _has(fl[10], F.INFO) and int(want[12, 7]) & (1 << seg)                          # an LSF frame locks; the map keeps the bit
        assert _has(fl[13], F.END) and int(want[13, 7]) == 0                                   # the EOT's reset() clears it
        assert _has(fl[19], F.LSF_FROM_LICH)                                                   # and a round completes again


def test_can_filter():
    for name, audio, end in (("can_filter_all", True, True), ("can_filter_other", False, False), ("can_filter_match", True, True)):
        _, want, fl, _ = _s(name)
        assert _has(fl[0], F.INFO) and want[0, 3] == 5
        assert all(_has(fl[1:5], F.AUDIO) == audio) and all(_has(fl[1:5], F.LSF_VALID | F.LOCKED))
        assert _has(fl[5], F.INFO) and bool(_has(fl[5], F.END)) == end
        if not audio:
            assert not want[1:5, 48:64].any()
    _, want, fl, _ = _s("can_filter_late_entry")
    assert _has(fl[5], F.INFO) and not any(_has(fl, F.AUDIO | F.END)) and _has(fl[8], F.INFO)


def test_eot_with_an_invalid_lsf_does_nothing():
    _, want, fl, states = _s("eot_invalid_lsf")
    assert fl[0] == F.FRAME and want[0, 2] == 0xFF
    assert fl[4] == F.FRAME and int(want[4, 7]) == 0x07 and states[4][60] == 0x07              # no reset(): the map is kept
    assert np.array_equal(states[4], states[3])
    assert _has(fl[7], F.LSF_FROM_LICH) and int(want[7, 6]) == 5                               # and the round completes with the segments from before it
    assert _has(fl[10], F.END) and fl[11] == F.FRAME


def test_two_calls_back_to_back():
    _, want, fl, _ = _s("two_calls")
    assert M.texts(want[0]) == ("YO8RZZ", "AB1CDE") and M.texts(want[9]) == ("DL1ABC.M", "BROADCAST") and want[9, 3] == 15
    assert int(_has(fl, F.END).sum()) == 2 and int(_has(fl, F.INFO).sum()) == 4
    assert M.texts(want[10]) == ("DL1ABC.M", "BROADCAST") and _has(fl[10], F.AUDIO)


def test_frame_number_wrap_and_eos():
    _, want, fl, _ = _s("frame_number_wrap")
    assert [int(r[4]) | int(r[5]) << 8 for r in want[1:9]] == [2044, 2045, 2046, 2047, 0, 1, 2, 3 | 0x8000]


def test_destinations_and_callsign_texts():
    _, want, fl, _ = _s("destinations")
    assert all(_has(fl[:12], F.INFO))
    assert [M.texts(r)[1] for r in want[:5]] == ["AB1CDE", "BROADCAST", "ECHO", "INFO", "UNLINK"]
    assert [bytes(r[14:20]) for r in want[:5]] == [M.DESTINATIONS[t] for t in range(5)]
    assert [M.texts(r)[1] for r in want[5:8]] == ["ECHO", "INFO", "UNLINK"] and bytes(want[5, 14:20]) == bytes([0x12, 0x34, 0x7D, 0xD8, 0x0E, 0x00])
    assert len(M.texts(want[8])[1]) == 10 and len(M.texts(want[9])[0]) == 10 and len(M.texts(want[9])[1]) == 10
    assert M.texts(want[10]) == ("AxBx0", "A")                                                 # 'x' where a digit is 0
    assert M.texts(want[11]) == ("", "") and _has(fl[11], F.LSF_VALID) and _has(fl[12], F.AUDIO)


def test_passed_over_records():
    inp, want, fl, states = _s("passed_over")
    assert not want[3].any() and not want[4].any() and np.array_equal(states[3], states[2]) and np.array_equal(states[4], states[2])
    assert int(inp[3, 4]) == 47 and inp[4, :4].tobytes() == bytes([0xAA, 0xED, 0x89, 0x00])
    assert _has(fl[5], F.AUDIO) and int(want[5, 4]) == 2


def test_reconfigured():
    _, want, fl, _ = _s("reconfigured")
    assert all(_has(fl[1:5], F.AUDIO)) and not any(_has(fl[7:11], F.AUDIO)) and all(_has(fl[13:17], F.AUDIO))
    assert _has(fl[5], F.END) and not _has(fl[11], F.END) and _has(fl[17], F.END)
    assert [tuple(r) for r in G["reconfig"][:, 1:]] == [(6, 0, 0), (12, 9, 1)]


def test_transmit_calls_cover_the_issue():
    names = list(G["tx_names"])
    assert [int(G["tx_desc"][names.index("type_%d" % t), 21]) for t in range(5)] == [0, 1, 2, 3, 4]
    by = {n: G["tx_desc"][i] for i, n in enumerate(names)}
    assert by["empty_both"][9] == 0 and by["empty_both"][19] == 0 and by["nine_characters"][9] == 9 and by["ten_characters"][9] == 10
    assert bytes(by["lower_case"][:6]) == b"yo8rzz" and bytes(by["punctuation"][:7]) == b"A-B/C.D"
    assert {int(d[20]) for d in G["tx_desc"]} >= {0, 15} and int(G["tx_n"][names.index("long_call")]) == 2050
    assert all(bytes(s[:48]) == b"\x77" * 48 and bytes(s[48:50]) == b"\x55\xf7" for s in G["tx_start"])
    assert all(bytes(e[:2]) == b"\xff\x5d" and bytes(e[48:]) == b"\x55\x5d" * 8 for e in G["tx_end"])
    # what the reference's receiver makes of the reference's LSF frames: the addresses the descriptors ask for
    recs = np.stack([M.fs_record(s[48:]) for s in G["tx_start"]])
    lsf = M.decode_records(recs)[:, 2:32]
    assert bytes(lsf[names.index("ten_characters"), 0:12]) == bytes(12)                          # more than nine characters: the zero address
    assert bytes(lsf[names.index("empty_both"), 0:12]) == b"\xff" * 6 + bytes(6)
    assert bytes(lsf[names.index("empty_destination"), 0:6]) == b"\xff" * 6 and bytes(lsf[names.index("type_1"), 0:6]) == b"\xff" * 6
    assert bytes(lsf[names.index("type_4"), 0:6]) == M.DESTINATIONS[4] and bytes(lsf[names.index("type_0"), 0:6]) == M.call6("AB1CDE")
    assert bytes(lsf[names.index("lower_case"), 6:12]) == M.call6(value=35 * 40 ** 2)      # "yo8rzz": only the 8 counts, the lower-case letters are digit 0
    assert all(((int(l[12]) << 8 | int(l[13])) & 0x7F) == 5 for l in lsf) and [int(l[12]) << 8 | int(l[13]) for l in lsf[:5]] == [5 | t << 7 for t in range(5)]
