"""The named DMO scenarios of tests/sig.py reach the slicer branches they are named for: asserted on the CPU from the oracle's records and
state alone (orc.demod_dmr_port3 -> orc.DmoSink, with DmoSink.peek for the state), and every scenario is run through the reference's own
gr_dmr_dmo_sink as well where oracle/_ref is built, so the branches are pinned and not only restated.  tests/test_gpu_dmo_adverse.py
runs the same streams through k_dmo_sink."""
import ctypes as C
import os

import numpy as np
import pytest

import orc
import sig
import test_gpu_dmo_adverse as G
from test_dmo_sink import _same
from test_ref_blocks import REF, _ref_dmo

RECV_NONE, RECV_DATA, RECV_VOICE = 0, 1, 3
DATA, VOICE, VOICE_SYNC = 0, 1, 2
IMPAIRED = ["impaired%d" % k for k in range(len(sig.DMO_IMPAIRED))]


@pytest.fixture(scope="module")
def runs():
    """per scenario: (frames sent, port 3 of the oracle's chain, the oracle's records)"""
    out = {}
    for name in list(sig.DMO_SCENARIOS) + IMPAIRED:
        frames, x = sig.dmo_iq(name)
        p3 = orc.demod_dmr_port3(x)
        out[name] = (frames, p3, orc.DmoSink().process(p3))
    return out


def test_data_call_continues_and_drops_the_terminator(runs):
    """DATA CONTINUATION and TERMINATOR IN THE WRONG STATE: 5 records, all typed data -- the header (0x06), the continuations 0x07, 0x08,
    0x0A, the CSBK; the 0x02 burst between them is not written (the machine is in RECV_DATA) and does not reset the machine either"""
    frames, p3, recs = runs["data_call"]
    assert len(frames) == 6 and len(recs) == 5
    assert [r[0] for r in recs] == [DATA] * 5 and all(r[2] == 1 for r in recs)
    assert all(_same(r[3], f) for r, f in zip(recs, frames[:4] + frames[5:]))
    assert not any(_same(r[3], frames[4]) for r in recs)
    # the state on the way: RECV_DATA from the header until the CSBK resets it
    snk, states = orc.DmoSink(), []
    for s in range(0, p3.size, 60):
        if snk.process(p3[s:s + 60]):
            states.append(snk.peek("state"))
    assert states == [RECV_DATA] * 4 + [RECV_NONE]


def test_long_voice_call_wraps_the_frame_number(runs):
    """FRAME NUMBER WRAP: 10 records (header, voice sync, 7 voice, terminator); behind the sync the frame numbers run 1, 2, 3, 4, 5, 0, 1"""
    frames, _, recs = runs["long_voice_call"]
    assert [r[0] for r in recs] == [DATA, VOICE_SYNC] + [VOICE] * 7 + [DATA]
    assert [r[1] for r in recs[2:9]] == [1, 2, 3, 4, 5, 0, 1] and recs[1][1] == 0 and recs[9][1] == 0
    assert all(_same(r[3], f) for r, f in zip(recs, frames))


def test_lost_sync_resets_and_reacquires(runs):
    """LOST SYNC: 17 records.  Header, voice sync and the two voice frames (syncCount 1, 2); then one "voice" record per slot period of
    silence while syncCount runs 3 .. 12, i.e. ten of them; the slot that takes syncCount to 13 runs dmo_reset BEFORE the state is looked
    at, so it writes nothing and nothing follows until the new call: 4 + 10 = 14 records with the first colour code, then the new call's
    header, voice sync and voice frame with the second, acquired through the first = true path (all four averages re-seeded at the new,
    smaller deviation and the new centre) at the ring position that the running sample index gives"""
    frames, p3, recs = runs["lost_sync"]
    assert len(recs) == 17
    assert [r[0] for r in recs] == [DATA, VOICE_SYNC] + [VOICE] * 12 + [DATA, VOICE_SYNC, VOICE]
    assert [r[1] for r in recs[2:14]] == [1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 0]
    assert [r[2] for r in recs] == [1] * 14 + [2] * 3
    assert all(_same(r[3], f) for r, f in zip(recs[:4] + recs[14:], frames))
    # the machine has let go before the new call starts, and holds other averages after it than before
    quiet = 5 * (sig.DMO_LEAD_SYMBOLS + 17 * sig.DMO_SLOT_SYMBOLS)
    snk = orc.DmoSink()
    assert len(snk.process(p3[:quiet])) == 14
    assert (snk.peek("state"), snk.peek("syncCount"), snk.peek("endPtr"), snk.peek("syncPtr")) == (RECV_NONE, 0, 9999, 0)
    before = snk.peek("threshold").copy()
    snk.process(p3[quiet:])
    after = snk.peek("threshold")
    assert snk.peek("state") == RECV_VOICE and np.all(after < 0.8 * before) and np.all(after > 0.6 * before)      # levels x 0.7
    assert np.all(np.abs(snk.peek("centre")) > 0.02)                                                                # the DC offset


def test_drifting_level_fills_the_four_averages_differently(runs):
    """UNEQUAL AVERAGES: when the last frame is cut, the four centre / threshold slots hold four different values each"""
    frames, p3, recs = runs["drifting_level"]
    assert len(recs) == 10 and all(_same(r[3], f) for r, f in zip(recs, frames))
    assert [r[0] for r in recs] == [DATA, VOICE_SYNC] + [VOICE] * 5 + [VOICE_SYNC, VOICE, DATA]
    snk = orc.DmoSink()
    snk.process(p3)
    for field in ("centre", "threshold"):
        v = snk.peek(field)
        assert len(set(v.tolist())) == 4, (field, v)
    th = snk.peek("threshold")
    assert th.max() > 1.3 * th.min()


def test_after_reset_drops_orphan_continuations(runs):
    """DATA CONTINUATION, the other side, and LOST SYNC's ring position: 6 records of 9 bursts -- the CSBK; not the 0x07 and 0x0A behind it
    (RECV_NONE: no header has opened a data call); header, 0x08, CSBK; voice header and terminator; not the 0x07 behind the terminator.
    The second burst sits 172 symbols behind the first, off the 288-symbol slot grid, and is acquired right behind the CSBK's reset"""
    frames, p3, recs = runs["after_reset"]
    assert len(frames) == 9 and len(recs) == 6 and [r[0] for r in recs] == [DATA] * 6
    assert all(_same(r[3], frames[i]) for r, i in zip(recs, (0, 3, 4, 5, 6, 7)))
    snk, states = orc.DmoSink(), []
    for s in range(0, p3.size, 60):
        if snk.process(p3[s:s + 60]):
            states.append(snk.peek("state"))
    assert states == [RECV_NONE, RECV_DATA, RECV_DATA, RECV_NONE, RECV_VOICE, RECV_NONE]


def _pretest(p3):
    """the Hamming pre-test of correlateSync restated with numpy: True where the 24 signs of the sample's phase are within 2 bits of a sync word"""
    s = (np.asarray(p3) > 0).astype(np.uint32)
    sh = np.zeros(s.size, np.uint32)
    for i in range(24):
        sh[115:] |= s[115 - 5 * i:s.size - 5 * i] << i
    bits = lambda v: np.unpackbits(v.view(np.uint8)).reshape(-1, 32).sum(axis=1)
    return (bits(sh ^ np.uint32(0x0076286E)) <= 2) | (bits(sh ^ np.uint32(0x0089D791)) <= 2)


def test_impaired_group_loses_syncs_and_bits(runs):
    """REJECTIONS: under noise and fades at least three streams give fewer records than bursts were sent (a voice call only loses records
    where a sync is refused while the machine is in RECV_NONE: the header of the call), every stream still gives some, records differ from
    what was sent, and in a stream that lost its header the Hamming pre-test DID pass inside that burst: with no sync accepted (none was:
    a frame would have been cut 269 samples later) maxCorr is 0, so the burst was refused by `corr > maxCorr` or by `errs > 3`"""
    fewer, differ = [], 0
    for name in IMPAIRED:
        frames, p3, recs = runs[name]
        assert len(frames) == 10 and 1 <= len(recs) <= 10, name
        differ += sum(not any(_same(r[3], f) for f in frames) for r in recs)
        if len(recs) < len(frames):
            fewer.append(name)
    assert len(fewer) >= 3 and differ >= 1, (fewer, differ)
    refused = 0
    for name in fewer:
        frames, p3, recs = runs[name]
        if recs[0][0] != VOICE_SYNC:
            continue
        # the first record is the voice sync: the header before it was lost.  Its slot: one period before the first frame cut
        snk, k = orc.DmoSink(), 0
        while not snk.process(p3[k:k + 1]):
            k += 1
        lost = slice(k - 1440 - 660, k - 1440 + 1)
        refused += int(_pretest(p3)[lost].any())
    assert refused >= 1


def test_slot_lanes_of_the_gpu_batch():
    """WINDOW WRAP: the three delays written into tests/test_gpu_dmo_adverse.py put the first sync at ring slots 0, 1 and 1439 (the GPU
    test asserts the same; here it runs without a GPU)"""
    for b, (slot, delay) in G.SLOT_LANES.items():
        name, seed, d, cfo = G.lane(b)
        assert d == delay and name == "long_voice_call"
        first, slots = G.first_sync_slot(orc.demod_dmr_port3(sig.dmo_iq(name, seed=seed, delay=d, cfo=cfo)[1]))
        assert first == slot and len(slots) >= 9 and all((s - slot + 1) % 1440 <= 2 for s in slots), (b, slots)


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/libqrl_ref.so not built (make -C oracle ref needs /root/reference)")
@pytest.mark.parametrize("name", list(sig.DMO_SCENARIOS) + IMPAIRED)
def test_scenarios_oracle_equals_the_reference_block(runs, name):
    """the reference's gr_dmr_dmo_sink itself on every scenario's port 3, in ragged calls: identical records"""
    ref = C.CDLL(REF)
    ref.ref_dmo_sink.restype = C.c_size_t
    _, p3, recs = runs[name]
    assert _ref_dmo(ref, p3, 997) == recs
