"""The scenarios of tests/golden/ref/dmr_rx.npz reach the branches they are named for: asserted from the recorded reference records alone,
so that a scenario cannot pass by doing nothing.  The voice bursts of a superframe are FN 0..5: FN 1..4 carry the four fragments, so an
embedded LC completes on FN 4."""
import os

import numpy as np

import dmr_rx
from dmr_rx import (VALID, PROCESSED, HEADER_VOICE, HEADER_DATA, TERMINATOR, END_BEEP, AUDIO, EMBEDDED, TALKER_ALIAS, GPS, UNKNOWN_FLCO, IDLE,
                    LATE_ENTRY, AUDIO_STATE, DATA_STATE, flags, ids, alias_of)

G = dmr_rx.load_golden()


def S(name):
    _, inp, want, cc, prom, reconfig = dmr_rx.scenario(G, name)
    return inp, want, flags(want), cc, prom


def has(f, bit):
    return (f & bit) != 0


def test_the_golden_is_small_and_complete():
    assert os.path.getsize(dmr_rx.GOLDEN) <= 1 << 17          # the size class of dmr_tx.npz
    assert len(G["names"]) == len(set(G["names"])) >= 16
    f = flags(G["expected"])
    assert np.bitwise_or.reduce(f.reshape(-1)) == (1 << 11) - 1, "a flag no scenario raises"
    assert set(G["expected"][..., 2].reshape(-1)) == {IDLE, LATE_ENTRY, AUDIO_STATE, DATA_STATE}
    for k in range(len(G["names"])):
        assert not G["expected"][k, int(G["counts"][k]):].any() and not G["inputs"][k, int(G["counts"][k]):].any()
    assert (G["expected"][..., 5:8] == 0).all() and (G["expected"][..., 29:32] == 0).all() and (G["expected"][..., 100:] == 0).all()


def test_whole_call():
    inp, want, f, cc, prom = S("whole_call")
    assert list(inp[:, 0]) == [0, 0] + [2 if k % 6 == 0 else 1 for k in range(31)] + [0, 0]
    assert f[0] == VALID | PROCESSED | HEADER_VOICE | END_BEEP and f[1] == VALID | PROCESSED | HEADER_VOICE      # the beep only from idle
    assert has(f[2:33], AUDIO).all() and (want[:33, 2] == AUDIO_STATE).all()
    done = np.nonzero(has(f, EMBEDDED))[0]
    assert list(done) == [2 + 6 * s + 4 for s in range(5)] and list(want[done, 16]) == [0, 4, 5, 6, 7]
    assert bytes(want[done[0], 17:26]) == dmr_rx.OWN and ids(want[done[0]]) == (dmr_rx.A, dmr_rx.B_)
    ta = np.nonzero(has(f, TALKER_ALIAS))[0]
    assert list(ta) == [done[4]] and alias_of(want[ta[0]]) == (1, 27, dmr_rx.TEXT)
    assert f[33] == VALID | PROCESSED | TERMINATOR | END_BEEP and f[34] == VALID | PROCESSED and (want[33:, 2] == IDLE).all()
    assert (want[:33, 3] == 1).all() and (want[33:, 3] == 0).all() and ids(want[34]) == (0, 0)


def test_late_entry_differs_between_promiscuous_and_fixed():
    _, p, fp, _, prom = S("late_entry_promiscuous")
    inp, x, fx, cc, fixed = S("late_entry_fixed")
    _, z, fz, cc0, _ = S("late_entry_fixed_zero")
    assert np.array_equal(inp, S("late_entry_promiscuous")[0]) and (prom, fixed, cc, cc0) == (1, 0, 1, 0)
    # promiscuous: _color_code_RX is 0 and stays 0, the check passes, voice A opens the call
    assert p[0, 2] == LATE_ENTRY and has(fp[:12], AUDIO).all() and (p[:12, 3] == 0).all()
    assert has(fp[4], EMBEDDED) and ids(p[4]) == (1234567, 7654321) and p[4, 4] == 3 and ids(p[10]) == (dmr_rx.A, dmr_rx.B_) and p[10, 4] == 0
    assert fp[12] == VALID | PROCESSED | TERMINATOR | END_BEEP
    # a fixed colour code: a voice burst is checked with _color_code_RX = 0, so every one is refused, and so is nothing else
    assert (fx[:12] == VALID).all() and (x[:, 2] == IDLE).all() and fx[12] == VALID | PROCESSED
    # ... unless the fixed colour code is 0; then the terminator of colour code 1 is refused
    assert z[0, 2] == LATE_ENTRY and has(fz[:12], AUDIO).all() and fz[12] == VALID and z[12, 2] == LATE_ENTRY


def test_late_entry_in_mid_superframe():
    inp, want, f, _, _ = S("late_entry_mid_superframe")
    assert list(inp[:3, 1]) == [3, 4, 5] and not has(f[:3], EMBEDDED | AUDIO).any() and (want[:3, 2] == IDLE).all()     # LCSS 3, 2 with nothing begun
    assert want[3, 2] == LATE_ENTRY and has(f[7], EMBEDDED) and ids(want[7]) == (1234567, 7654321)


def test_damaged_fragments():
    inp, want, f, _, _ = S("damaged_fragments")
    done = [bool(has(f[6 * s + 4], EMBEDDED)) for s in range(10)]
    assert done == [True, False, True, False, True, False, True, False, False, True]
    assert not has(f[[i for i in range(60) if i % 6 != 4]], EMBEDDED).any()
    srcs = [ids(want[6 * s + 4])[0] for s in range(10)]
    assert srcs == [101, 101, 103, 103, 105, 105, 107, 107, 107, 110]       # a refusal leaves the last delivery in place
    # (superframe 7: a parity bit and a data bit of one row are two errors like any other; 8: the row is corrected and the parity row is wrong)
    assert bytes(want[4, 17:26]) == dmr_rx.lc(0, 101, 9)                    # seven errors, one per row, all corrected


def test_reset_in_mid_assembly():
    inp, want, f, _, _ = S("reset_in_mid_assembly")
    assert list(inp[:, 1]) == [0, 1, 2, 0, 3, 4, 5, 0, 1, 2, 1, 2, 3, 4, 5, 0]
    assert np.nonzero(has(f, EMBEDDED))[0].tolist() == [13]          # not at 5: voice A cleared the two fragments; at 13 the LC begun by the second LCSS 1
    assert ids(want[13]) == (1234567, 7654321) and ids(want[12]) == (0, 0)


def test_terminators():
    inp, want, f, _, _ = S("terminators")
    assert f[0] == VALID | PROCESSED and want[0, 2] == IDLE                       # while idle: no signal
    assert f[8] == VALID | PROCESSED and want[8, 2] == AUDIO_STATE and ids(want[8]) == (dmr_rx.A, dmr_rx.B_)   # no ids: passed over
    assert has(f[9], AUDIO)
    assert f[10] == VALID and want[10, 2] == AUDIO_STATE                          # another colour code: refused
    assert has(f[11], AUDIO)
    assert f[12] == VALID | PROCESSED | TERMINATOR | END_BEEP and f[13] == VALID | PROCESSED and want[12, 2] == IDLE


def test_promiscuous_lock():
    inp, want, f, _, prom = S("promiscuous_lock")
    assert prom == 1 and want[0, 3] == 3 and f[0] == VALID | PROCESSED            # a CSBK locks the colour code
    assert has(f[1], HEADER_VOICE) and (want[:8, 3] == 3).all()
    assert f[8] == VALID and f[9] == VALID and ids(want[8]) == (dmr_rx.A, dmr_rx.B_)          # the other call's header and CSBK
    assert has(f[10:16], AUDIO).all() and ids(want[14]) == (1234567, 7654321)     # its voice passes: it is checked with _color_code_RX
    assert f[16] == VALID and want[16, 2] == AUDIO_STATE                          # its terminator does not
    assert has(f[17], TERMINATOR) and want[17, 3] == 0
    assert has(f[18], HEADER_VOICE) and want[18, 3] == 5 and has(f[25], TERMINATOR)


def test_talker_alias():
    _, want, f, _, _ = S("alias_formats_0_2")
    got = [alias_of(r) for r in want[has(f, TALKER_ALIAS)]]
    seven = bytes([1]) + bytes(range(0x41, 0x41 + 20))
    assert got == [(0, 20, seven[:21]), (2, 10, "Țară nouă".encode().ljust(13, b"\0"))]   # 7-bit: 21 bytes hold 24 characters >= 20; UTF-8: 6 + 7 >= 10
    _, want, f, _, _ = S("alias_format_3")
    at = np.nonzero(has(f, TALKER_ALIAS))[0]
    got = [alias_of(want[i]) for i in at]
    assert got[0] == (3, 10, "Ионеску Ад".encode("utf-16-be")) and len(got[0][2]) == 2 * 10
    assert got[1] == (3, 31, bytes(range(1, 63))) and len(got[1][2]) == 2 * 31
    assert at[0] == 1 + 6 * 2 + 4           # not in block 1 at 13 bytes >= 10: format 3 waits for twice the length
    _, want, f, _, _ = S("alias_corners")
    at = np.nonzero(has(f, TALKER_ALIAS))[0]
    emb = np.nonzero(has(f, EMBEDDED))[0]
    assert len(emb) == 3 + 1 + 4 + 4 + 2 + 2 + 2
    got = [alias_of(want[i]) for i in at]
    assert got == [(1, 6, b"ABCDEF"), (1, 0, b"GHIJKL"), (1, 13, b"after the end"), (1, 27, dmr_rx.TEXT)]
    assert at[0] == emb[3]                   # the three blocks in front brought nothing; the header alone completes length 6
    assert at[1] == emb[8] and at[2] == emb[13]      # the second alias of the first call is passed over whole; length 0 ends in its header
    assert at[3] == emb[17]                  # header, block 1, terminator, header of the next call, block 2 and 3: the 13 bytes survive the terminator, 27 are reached in block 3


def test_gps_and_unknown_flco():
    _, want, f, _, _ = S("gps_and_unknown_flco")
    emb = np.nonzero(has(f, EMBEDDED))[0]
    assert [int(want[i, 16]) for i in emb] == [8, 0x30, 1]              # 0x81: the FLCO is six bits
    assert has(f[emb[0]], GPS) and bytes(want[emb[0], 17:26]) == bytes([8, 0, 0x05, 0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC])
    assert has(f[emb[1]], UNKNOWN_FLCO) and has(f[emb[2]], UNKNOWN_FLCO) and not has(f[emb[1:]], GPS).any()
    assert all(ids(want[i]) == (dmr_rx.A, dmr_rx.B_) for i in emb)


def test_data():
    inp, want, f, _, _ = S("data")
    assert f[0] == VALID | PROCESSED | HEADER_DATA and want[0, 2] == DATA_STATE and ids(want[0]) == (dmr_rx.A, dmr_rx.B_)
    assert (f[1:3] == VALID | PROCESSED).all()
    assert not has(f[3:9], AUDIO).any() and (want[3:9, 2] == DATA_STATE).all() and has(f[7], EMBEDDED)      # voice in state DATA: no audio
    assert f[9] == VALID | PROCESSED | TERMINATOR | END_BEEP
    assert f[10] == VALID and want[10, 2] == IDLE and has(f[11], HEADER_DATA) and ids(want[11]) == (dmr_rx.C_, 1)


def test_pass_through():
    """A voice burst whose getVoice() fails cannot be made: DMRFrame::getVoice returns false only for a frame whose type is neither voice
    nor voice sync, and addFrames calls processAudio only for the data types the constructor gives exactly those two frame types."""
    inp, want, f, _, _ = S("pass_through")
    assert f[0] == VALID | PROCESSED and f[1] == VALID              # a CSBK of the colour code, and one of another
    assert f[6] == 0 and np.array_equal(want[6, 2:16], want[5, 2:16])          # validate() refuses it: nothing moves
    assert inp[8, 0] == 3 and f[8] == VALID | PROCESSED             # a frame type the class does not know: valid, and no call for it
    assert has(f[9], EMBEDDED) and ids(want[9]) == (1234567, 7654321)           # the assembly went on across both


def test_reconfigured():
    _, want, f, cc, prom = S("reconfigured")
    assert list(np.nonzero(has(f, HEADER_VOICE))[0]) == [0, 8, 16] and list(np.nonzero(has(f, TERMINATOR))[0]) == [7, 15, 23]
    assert [int(want[i, 3]) for i in (0, 8, 16)] == [1, 5, 7]
