"""DMR layer 2 transmit on the CPU: the recorded bursts of tests/golden/ref/dmr_tx.npz against the live reference where it is present
(DMRFrame and the MMDVM encoders per record; DMRControl, compiled unmodified against tests/host/dmr_ctl_stub, per call), the reference's own
validate() on what it built, the voice sequencing as a function of the burst index, the package's host helpers, and
qradiolink_amd/csrc/dmr_tx_core.hpp, the code the kernels call, under the address and undefined-behaviour sanitizers
(tests/host/test_dmr_tx_core.cpp) byte for byte against the same bursts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dmr_l2
import dmr_tx
import qradiolink_amd as q

ROOT = dmr_tx.ROOT
G = dmr_tx.load_golden()
RECORDS, BURSTS, CALLS, VOICE = G["records"], G["bursts"], G["calls"], G["call_voice"]
NV = dmr_tx.CALL_VOICE


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = dmr_tx.load_ref(tmp_path_factory.mktemp("dmr_tx_ref"))
    if r is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r


@pytest.fixture(scope="module")
def rx_ref(tmp_path_factory):
    r = dmr_l2.load_ref(tmp_path_factory.mktemp("dmr_l2_ref"))
    if r is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r


def test_golden_holds_what_it_claims():
    kind, fn, cc, dt = RECORDS[:, 0], RECORDS[:, 1], RECORDS[:, 2], RECORDS[:, 3]
    assert {0, 1, 2, 3, 4, 5, 7, 8} <= set(kind) and {6, 9, 255} <= set(kind)
    lc = kind == dmr_tx.K_LC
    assert {1, 2} <= set(dt[lc]) and set(dt[lc]) - {1, 2}, "both LC masks, and a data type the LC encoder refuses"
    for k in (dmr_tx.K_LC, dmr_tx.K_CSBK, dmr_tx.K_DATA_HEADER, dmr_tx.K_RATE12, dmr_tx.K_RATE34, dmr_tx.K_VOICE_SYNC, dmr_tx.K_VOICE):
        assert {0, 1, 15} <= set(cc[kind == k]), "kind %d lacks a colour code" % k
    for k in (dmr_tx.K_LC, dmr_tx.K_VOICE):
        lcs = RECORDS[kind == k, 4:13]
        assert {0, 3} <= set(lcs[:, 0]) and {0, 0xC2} <= set(lcs[:, 1])
        ids = {int.from_bytes(bytes(r[a:a + 3]), "big") for r in lcs for a in (3, 6)}
        assert {0, 1, 0xFFFFFF} <= ids
    assert set(range(6)) <= set(fn[kind == dmr_tx.K_VOICE]) and max(fn[kind == dmr_tx.K_VOICE]) > 5
    hdr = RECORDS[kind == dmr_tx.K_DATA_HEADER]
    assert (((hdr[:, 16] & 15) == 0) & ((hdr[:, 25] & 1) == 1)).any(), "no UDT header whose byte 9 get() changes"
    # the calls: colour codes, both call types, both FIDs, the corner ids, the alias lengths with high bytes, both modes
    assert {0, 1, 15} <= set(CALLS[:, 8]) and {0, 3} == set(CALLS[:, 6]) and {0, 0xC2} == set(CALLS[:, 7])
    ids = {int.from_bytes(bytes(c[a:a + 3]), "big") for c in CALLS for a in (0, 3)}
    assert {0, 1, 0xFFFFFF} <= ids
    lengths = {int(np.nonzero(c[9:36])[0].max()) + 1 if c[9:36].any() else 0 for c in CALLS}
    assert set(dmr_tx.ALIAS_LENGTHS) <= lengths and (CALLS[:, 9:36] >= 0x80).any()
    assert set(G["call_repeater"]) == {0, 1}
    assert NV == 31 and (G["call_nslots"] == 3 * G["call_repeater"] + 2 + NV + 4).all()
    assert (G["call_extra"] == 5).all()   # the reference ends a call at a superframe boundary: five more voice bursts before the terminator
    assert os.path.getsize(dmr_tx.GOLDEN) <= 1 << 20


def test_golden_is_fresh(ref):
    g = dmr_tx.record_golden(ref)
    assert sorted(g) == sorted(G)
    for k in g:
        assert np.array_equal(g[k], G[k]), k


def test_the_reference_validates_and_returns_what_was_encoded(rx_ref):
    kind, cc, dt = RECORDS[:, 0], RECORDS[:, 2] & 15, RECORDS[:, 3] & 15
    data = np.nonzero((kind >= 1) & (kind <= 5) & ~((kind == 1) & (dt != 1) & (dt != 2)))[0]
    rec = rx_ref.records(dmr_tx.dmo_records(BURSTS[data], dmr_l2.FT_DATA), 1)
    assert (rec[:, 4] == 1).all(), "validate() refuses bursts %s" % data[rec[:, 4] != 1][:10]
    assert np.array_equal(rec[:, 2], cc[data]) and np.array_equal(rec[:, 3], dt[data])
    assert np.array_equal(rec[:, 20:53], BURSTS[data]), "validate() regenerates other bytes"
    for j, i in enumerate(data):
        r, pay = RECORDS[i], rec[j, 53:80]
        if kind[i] == dmr_tx.K_LC:
            assert bytes(pay[:9]) == bytes(r[4:13])
            assert (rec[j, 9], rec[j, 10]) == (r[4] & 0x3F, r[5])
            assert int.from_bytes(bytes(rec[j, 12:16]), "little") == int.from_bytes(bytes(r[10:13]), "big")
            assert int.from_bytes(bytes(rec[j, 16:20]), "little") == int.from_bytes(bytes(r[7:10]), "big")
        elif kind[i] == dmr_tx.K_CSBK:
            assert bytes(pay[:10]) == bytes(r[16:26]) and rec[j, 9] == r[16] & 0x3F and rec[j, 10] == r[17]
        elif kind[i] == dmr_tx.K_DATA_HEADER:
            want = bytearray(r[16:26])
            if want[0] & 15 == 0:
                want[9] &= 0xFE
            assert bytes(pay[:10]) == bytes(want)
        elif kind[i] == dmr_tx.K_RATE12:
            assert rec[j, 8] == 12 and bytes(pay[:12]) == bytes(r[16:28])
        else:
            assert rec[j, 8] == 18 and bytes(pay[:18]) == bytes(r[16:34])
    voice = np.nonzero((kind == dmr_tx.K_VOICE_SYNC) | (kind == dmr_tx.K_VOICE))[0]
    ft = np.where(kind[voice] == dmr_tx.K_VOICE, dmr_l2.FT_VOICE, dmr_l2.FT_VOICE_SYNC)
    inp = dmr_tx.dmo_records(BURSTS[voice], 0, fn=RECORDS[voice, 1], cc=cc[voice])
    inp[:, 0] = ft
    rec = rx_ref.records(inp, 0)
    assert np.array_equal(rec[:, 53:80], RECORDS[voice, 16:43]) and np.array_equal(rec[:, 2], cc[voice])
    fn = RECORDS[voice, 1].astype(int)
    lcss = np.where(ft == dmr_l2.FT_VOICE, np.select([fn == 1, fn == 4, (fn == 2) | (fn == 3)], [1, 2, 3], 0), 0)
    assert np.array_equal(rec[:, 7], lcss) and not rec[:, 6].any()


def test_embedded_fragments_of_a_call_reassemble_to_the_lc_of_their_superframe():
    for m in range(CALLS.shape[0]):
        frames = dmr_tx.call_voice_frames(G, m)
        rule = q.dmr_voice_call_records(CALLS[m], NV)
        for s in range(NV // 6):
            lc, crc = dmr_tx.embedded_lc(frames[6 * s + 1:6 * s + 5])
            assert lc == bytes(rule[6 * s + 1, 4:13]), "call %d superframe %d" % (m, s)
            assert crc == sum(lc) % 31
        own = bytes([CALLS[m, 6], CALLS[m, 7], 0]) + bytes(CALLS[m, 3:6]) + bytes(CALLS[m, 0:3])
        assert bytes(rule[1, 4:13]) == own and bytes(rule[30, 4:13]) == own          # superframe 0 again behind superframe 4
        alias = bytes(CALLS[m, 9:36])
        assert bytes(rule[7, 4:13]) == bytes([4, 0, 0x76]) + alias[0:6]
        for s in (2, 3, 4):
            assert bytes(rule[6 * s + 1, 4:13]) == bytes([3 + s, 0]) + alias[6 * (s - 1):6 * (s - 1) + 7]


def test_the_sequencing_is_a_function_of_the_burst_index():
    """first = 0, n = 31 against cuts of 1, 5, 6 and 19 bursts"""
    for m in (0, 3, CALLS.shape[0] - 1):
        whole = q.dmr_voice_call_records(CALLS[m], NV)
        parts, first = [], 0
        for n in (1, 5, 6, 19):
            parts.append(q.dmr_voice_call_records(CALLS[m], n, first))
            first += n
        assert first == NV and np.array_equal(np.concatenate(parts), whole)
        assert list(whole[:, 1]) == [k % 6 for k in range(NV)]
        assert list(whole[:, 0]) == [dmr_tx.K_VOICE if k % 6 else dmr_tx.K_VOICE_SYNC for k in range(NV)]


def test_host_rule_and_call_layout_equal_the_reference_s_control(ref):
    """q.dmr_call_slots' records, encoded by the reference's frame classes one by one, are the frames its DMRControl sends for the call"""
    for m in range(CALLS.shape[0]):
        records, runs = q.dmr_call_slots(CALLS[m], VOICE[m], repeater=bool(G["call_repeater"][m]))
        n = int(G["call_nslots"][m])
        assert records.shape == (n, 48)
        assert np.array_equal(ref.bursts(records), G["call_frames"][m, :n]), "call %d" % m
        assert runs == [(0, 20 * (72 * i + 33), 39 * 20) for i in range(n)]
    _, runs = q.dmr_call_slots(CALLS[0], VOICE[0, :6], slot_bytes=33)
    assert runs == []
    _, runs = q.dmr_call_slots(CALLS[0], VOICE[0, :6], slot_bytes=36, stream=3, first_byte=720)
    assert runs[0] == (3, 20 * (720 + 33), 60) and runs[1] == (3, 20 * (720 + 36 + 33), 60) and len(runs) == 2 + 6 + 4


def test_descriptor_helper_is_the_golden_layout():
    d = q.dmr_call_descriptor(1234567, 91, group=True, fid=0, color_code=1, alias=b"YO8RZZ Adrian")
    assert np.array_equal(d, CALLS[-1])
    d = q.dmr_call_descriptor(0xFFFFFF, 1, group=False, fid=0xC2, color_code=15, alias=bytes(range(200, 240)))
    assert bytes(d[:9]) == bytes([255, 255, 255, 0, 0, 1, 3, 0xC2, 15]) and bytes(d[9:36]) == bytes(range(200, 227)) and not d[36:].any()


def _flat_file(path):
    m = CALLS.shape[0]
    want = np.stack([dmr_tx.call_voice_frames(G, i) for i in range(m)])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", RECORDS.shape[0]) + RECORDS.tobytes() + BURSTS.tobytes())
        f.write(struct.pack("<II", m, NV) + CALLS.tobytes() + VOICE.tobytes() + want.tobytes())


def test_core_header_equals_the_golden_under_the_sanitizers(tmp_path):
    exe, data = str(tmp_path / "test_dmr_tx_core"), str(tmp_path / "golden.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_dmr_tx_core.cpp"), "-o", exe])
    _flat_file(data)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d records, %d calls of %d voice bursts" % (RECORDS.shape[0], CALLS.shape[0], NV)), r.stdout
