"""DMR layer 2 on the CPU: the restatement of tests/dmr_l2.py against the reference's recorded records (tests/golden/ref/dmr_l2.npz) and,
where the reference is present, against its live classes on fresh input; the scenario set's own conditions; the generated code tables
against the reference's decoders; and qradiolink_amd/csrc/dmr_l2_core.hpp, the code the kernels call, under the address and
undefined-behaviour sanitizers (tests/host/test_dmr_l2_core.cpp) byte for byte against the same records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dmr_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS, AUDIO_FEC, GROUP, RECORDS = dmr_l2.load_golden()
CONSTS = np.load(dmr_l2.GOLDEN)["consts"]
CHECKED_TYPES = (1, 2, 3, 4, 5, 6)   # the data types behind an RS(12,9) or CRC-CCITT check


@pytest.fixture(scope="module")
def restated():
    """the restatement's record and side information for every golden input, computed once"""
    out, info = [], []
    for i in range(INPUTS.shape[0]):
        d = {}
        out.append(bytes(dmr_l2.record(INPUTS[i].tobytes(), int(AUDIO_FEC[i]), d)))
        info.append(d)
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 80), info


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = dmr_l2.load_ref(tmp_path_factory.mktemp("dmr_l2_ref"))
    if r is None:
        pytest.skip("the reference's sources / oracle/_ref/libqrl_ref.so are not here")
    return r


def test_restatement_equals_the_golden(restated):
    mine, _ = restated
    bad = np.nonzero((mine != RECORDS).any(axis=1))[0]
    assert bad.size == 0, "records %s differ from the reference's" % bad[:10]


def test_record_constants_are_the_reference_s():
    import qradiolink_amd  # noqa: F401  (the header is the package's)
    hdr = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    assert "#define QRL_DMR_DT_VOICE_SYNC 0x%02X" % CONSTS[0] in hdr and "#define QRL_DMR_DT_VOICE 0x%02X" % CONSTS[1] in hdr
    assert list(CONSTS[2:5]) == [dmr_l2.FT_DATA, dmr_l2.FT_VOICE, dmr_l2.FT_VOICE_SYNC]
    voice = INPUTS[:, 0] != 0
    assert set(RECORDS[voice, 3]) == {int(CONSTS[0]), int(CONSTS[1])}


def test_data_type_scenarios_hold_what_they_claim():
    data = GROUP == 0
    cc_dt = RECORDS[data, 2].astype(int) * 16 + RECORDS[data, 3]
    assert set(RECORDS[data, 3]) == set(range(16)) and len(set(RECORDS[data, 2])) >= 8
    assert len(set(cc_dt)) >= 128
    for dt in CHECKED_TYPES:
        v = RECORDS[data & (RECORDS[:, 3] == dt), 4]
        assert 0 in v and 1 in v, "data type %d lacks an outcome" % dt
    # idle, rate 1, reserved: refused, the burst untouched, no IDs, no payload
    rest = data & (RECORDS[:, 3] > 8)
    assert rest.sum() >= 7 * 8 and not RECORDS[rest, 4:20].any() and not RECORDS[rest, 53:].any()
    assert np.array_equal(RECORDS[rest, 20:53], INPUTS[rest, 4:37])
    # every opcode branch of the CSBK parser and every data-packet format validated at least once
    csbk = data & (RECORDS[:, 3] == 3) & (RECORDS[:, 4] == 1)
    assert {op for op, _ in dmr_l2.CSBK_CASES} <= set(RECORDS[csbk, 9])
    hdr = data & (RECORDS[:, 3] == 6) & (RECORDS[:, 4] == 1)
    assert set(dmr_l2.DPF_CASES) <= set(RECORDS[hdr, 53] & 15)
    udt = hdr & ((RECORDS[:, 53] & 15) == 0)
    assert (RECORDS[udt, 62] & 1).any(), "no UDT header whose regenerated burst differs from a clean input"
    mbc = data & ((RECORDS[:, 3] == 4) | (RECORDS[:, 3] == 5))
    assert 1 in RECORDS[mbc, 4] and 0 in RECORDS[mbc, 4]


def test_rate34_scenarios_hold_what_they_claim(restated):
    _, info = restated
    st = [info[i] for i in np.nonzero((INPUTS[:, 0] == 0) & (RECORDS[:, 3] == 8))[0]]
    assert sum(1 for s in st if s["fail_pos"] == 999) >= 16                  # clean
    assert any(s["goes"] == 1 and s["rounds"] == 1 for s in st)             # repaired in one round
    assert any(s["rounds"] >= 10 for s in st)                               # garbage
    assert any(s["fail_pos"] == 0 for s in st)                              # failing position 0
    # A round in which no candidate advances cannot be built: the points before the failing position are a valid path, the state there
    # accepts 8 of the 16 candidates, and each of those passes the position, so the best position of a round is at least one past it (and
    # never 0).  Half of the survivors also match the next point's low bit, and so on: a round gains about four positions, 49 positions
    # take at most 13 rounds of the 20, and the second go and the rejection stay out of reach too (docs/MEASUREMENT.md, "DMR layer 2").
    assert not any(s["stuck"] for s in st) and all(s["goes"] <= 1 for s in st) and max(s["rounds"] for s in st) <= 13


def test_voice_scenarios_hold_what_they_claim(restated):
    _, info = restated
    voice = np.nonzero(GROUP == 2)[0]
    paths = set()
    for i in voice:
        paths |= info[i].get("paths", set())
    # Both substitutions occur: the uncorrectable A word (error count 10) and the threshold rule.  Of the threshold rule only the clause
    # errsA + errsB >= 6 with errsA >= 2 can fire: over all 2^24 A words a decode that passes changes at most three bits (a passing
    # three-bit correction has even parity, and a syndrome of weight < 3 is its own error pattern), so errsA >= 4 has no input.
    assert paths == {"a_bad", "rule_ab6"}
    assert set(INPUTS[voice, 0]) == {1, 2} and set(INPUTS[voice, 1]) == set(range(6))
    assert set(AUDIO_FEC[voice]) == {0, 1}
    assert not RECORDS[voice][AUDIO_FEC[voice] == 0][:, 5].any()
    assert RECORDS[voice, 5].max() >= 10 and (RECORDS[voice, 8] == 27).all()


def test_restatement_equals_the_live_reference_on_fresh_input(ref):
    inputs, af, _ = dmr_l2.build_scenarios(ref, seed=977)
    pick = np.arange(0, inputs.shape[0], 3)
    assert np.array_equal(dmr_l2.records(inputs[pick], af[pick]), ref.records(inputs[pick], af[pick]))


def test_golden_is_fresh(ref):
    inputs, af, group = dmr_l2.build_scenarios(ref)
    assert np.array_equal(inputs, INPUTS) and np.array_equal(af, AUDIO_FEC) and np.array_equal(group, GROUP)
    assert np.array_equal(ref.records(inputs, af), RECORDS)
    assert list(CONSTS) == [ref.const(i) for i in range(8)]


def test_generated_tables_are_the_reference_s(ref):
    """every syndrome of the three table decoders, the RS(12,9) and CRC checks, the encoders of both Golay codes and the trellis"""
    rng = np.random.RandomState(5)
    g19, qr, g23 = dmr_l2.coset_leaders(19, 11, 0xC75, 5), dmr_l2.coset_leaders(15, 8, 0x139, 4), dmr_l2.coset_leaders(23, 11, 0xC75, 3)
    for syn in range(2048):
        d = bytearray([(syn >> 11) & 0xFF, (syn >> 3) & 0xFF, (syn << 5) & 0xFF])
        assert ref.lib.ref_golay2087_decode(ref.buf(d)) == (g19[syn] >> 11) & 0xFF
        assert ref.lib.ref_golay23127_decode(syn) == g23[syn] >> 11
    for syn in range(256):
        d = bytearray([(syn >> 7) & 0xFF, (syn << 1) & 0xFF])
        assert ref.lib.ref_qr1676_decode(ref.buf(d)) == ((syn ^ qr[syn]) >> 7) & 0xFF
    for data in range(0, 4096, 7):
        assert ref.lib.ref_golay24128_encode(data) == dmr_l2.golay24_word(data)
        assert ref.lib.ref_golay23127_encode(data) >> 1 == dmr_l2.golay23_word(data)
    for _ in range(64):
        d = bytearray(rng.randint(0, 256, 12).astype(np.uint8).tobytes())
        par = dmr_l2.rs129_parity(d[:9])
        d[9:12] = bytes([par[2], par[1], par[0]])
        assert ref.lib.ref_rs129_check(ref.buf(d)) == 1
        crc = dmr_l2.crc_ccitt(d[:10])
        d[10:12] = bytes([crc >> 8, crc & 0xFF])
        assert ref.lib.ref_crc_ccitt162_check(ref.buf(d)) == 1
        pay, burst, bits = bytearray(rng.randint(0, 256, 18).astype(np.uint8).tobytes()), bytearray(33), [0] * 264
        ref.into("ref_trellis_encode", burst, ref.buf(pay))
        dmr_l2.trellis_encode(pay, bits)
        assert dmr_l2.to_bytes(bits) == burst


def _flat_file(path):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", INPUTS.shape[0]) + INPUTS.tobytes() + AUDIO_FEC.tobytes() + RECORDS.tobytes())


def test_core_header_equals_the_golden_under_the_sanitizers(tmp_path):
    exe, data = str(tmp_path / "test_dmr_l2_core"), str(tmp_path / "golden.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_dmr_l2_core.cpp"), "-o", exe])
    _flat_file(data)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d records" % INPUTS.shape[0]), r.stdout
