"""DMR layer 2 transmit for the tests: the reference's own frame layer and DMRControl behind tests/host/dmr_tx_ref.cpp (load_ref, where the
reference is present), the scenario set that tools/make_dmr_tx_golden.py records into tests/golden/ref/dmr_tx.npz, and small helpers the
CPU and GPU tests share.  The TX record and the call descriptor are those of include/qrl_hip.h."""
import ctypes as C
import os
import subprocess

import numpy as np

import dmr_l2

ROOT = dmr_l2.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref", "dmr_tx.npz")
REFERENCE, REF_LIB = dmr_l2.REFERENCE, dmr_l2.REF_LIB
STUB = os.path.join(ROOT, "tests", "host", "dmr_ctl_stub")
# every stand-in class gets a name of its own: oracle/_ref/libqrl_ref.so holds other classes called QString, Settings, DMRControl ...
RENAMED = ("QObject", "QString", "QByteArray", "QVector", "QSysInfo", "Settings", "Logger", "DMRUtils", "DMRControl")

TX_REC, CALL_REC, BURST = 48, 40, 33
K_EMPTY, K_LC, K_CSBK, K_DATA_HEADER, K_RATE12, K_RATE34, K_VOICE_SYNC, K_VOICE = 0, 1, 2, 3, 4, 5, 7, 8
CALL_VOICE = 31          # voice bursts of a golden call: superframes 0..4 and the wrap back to 0
CALL_SLOTS_MAX = 3 + 2 + CALL_VOICE + 4
SEED = 40961


class Ref:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.ref_dmr_tx_record.argtypes = [u8p, u8p]
        lib.ref_dmr_tx_record.restype = None
        lib.ref_dmr_tx_call.argtypes = [u8p, C.c_int, C.c_int, u8p, u8p, C.POINTER(C.c_int)]

    @staticmethod
    def buf(data):
        return (C.c_uint8 * len(data)).from_buffer(data)

    def bursts(self, records):
        records = np.ascontiguousarray(records, np.uint8).reshape(-1, TX_REC)
        out = np.zeros((records.shape[0], BURST), np.uint8)
        for i in range(records.shape[0]):
            src, dst = bytearray(records[i].tobytes()), bytearray(BURST)
            self.lib.ref_dmr_tx_record(self.buf(src), self.buf(dst))
            out[i] = np.frombuffer(bytes(dst), np.uint8)
        return out

    def call(self, call, repeater, voice):
        """-> (frames [slots, 33], extra): the whole call as DMRControl / gr_modem::transmitDMR send it, and the number of voice bursts the
        reference would still have sent between the last codec frame and the terminator"""
        voice = np.ascontiguousarray(voice, np.uint8).reshape(-1, 27)
        src, v = bytearray(np.asarray(call, np.uint8).tobytes()), bytearray(voice.tobytes()) or bytearray(1)
        out, extra = bytearray((3 + 2 + voice.shape[0] + 4) * BURST), C.c_int(0)
        n = self.lib.ref_dmr_tx_call(self.buf(src), int(repeater), voice.shape[0], self.buf(v), self.buf(out), C.byref(extra))
        assert n > 0, "DMRControl gave no frame"
        return np.frombuffer(bytes(out), np.uint8)[:n * BURST].reshape(n, BURST).copy(), extra.value


def load_ref(build_dir):
    """the reference behind tests/host/dmr_tx_ref.cpp, compiled into build_dir together with its src/DMR/dmrcontrol.cpp; None where the
    reference is absent"""
    if not (os.path.isdir(os.path.join(REFERENCE, "src", "MMDVM")) and os.path.isfile(REF_LIB)):
        return None
    so = os.path.join(str(build_dir), "libdmr_tx_ref.so")
    subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC"] + ["-D%s=dmr_tx_ref_%s" % (n, n) for n in RENAMED]
                          + [os.path.join(ROOT, "tests", "host", "dmr_tx_ref.cpp"), os.path.join(REFERENCE, "src", "DMR", "dmrcontrol.cpp"),
                             "-I" + STUB, "-I" + REFERENCE, "-I" + os.path.join(REFERENCE, "src", "MMDVM"), "-I" + os.path.join(ROOT, "oracle", "gr_stub"),
                             "-o", so, "-L" + os.path.dirname(REF_LIB), "-lqrl_ref", "-Wl,-rpath," + os.path.dirname(REF_LIB)])
    return Ref(C.CDLL(so))


# ------------------------------------------------------------------------------------------------------------------ the scenario set
COLOUR_CODES = (0, 1, 15, 7, 10)
IDS = (0, 1, 0xFFFFFF, 0x2345A7)
ALIAS_LENGTHS = (0, 6, 7, 26, 27)


def record(kind, fn=0, cc=0, dt=0, lc=None, payload=b""):
    r = np.zeros(TX_REC, np.uint8)
    r[0], r[1], r[2], r[3] = kind, fn, cc, dt
    if lc is not None:
        r[4:13] = np.frombuffer(bytes(lc), np.uint8)
    r[16:16 + len(payload)] = np.frombuffer(bytes(payload), np.uint8)
    return r


def lc_bytes(flco, fid, options, dst, src):
    return bytes([flco, fid, options, (dst >> 16) & 255, (dst >> 8) & 255, dst & 255, (src >> 16) & 255, (src >> 8) & 255, src & 255])


def descriptor(src, dst, group, fid, cc, alias):
    d = np.zeros(CALL_REC, np.uint8)
    d[0:3] = [(src >> 16) & 255, (src >> 8) & 255, src & 255]
    d[3:6] = [(dst >> 16) & 255, (dst >> 8) & 255, dst & 255]
    d[6], d[7], d[8] = 0 if group else 3, fid, cc
    d[9:9 + len(alias)] = np.frombuffer(bytes(alias), np.uint8)
    return d


def build_records(seed=SEED):
    """-> [n, 48] TX records: every kind, both LC masks and a data type the LC encoder refuses, the colour codes, group / private, FID 0 /
    0xC2, the corner ids, random payloads, FN 0..5 and out of range, PF / R bits and options in the LC, reserved and unknown kinds"""
    rng = np.random.RandomState(seed)
    rb = lambda n: rng.randint(0, 256, n).astype(np.uint8).tobytes()
    recs = []
    lcs = [lc_bytes(flco, fid, 0, dst, src) for flco in (0, 3) for fid in (0, 0xC2) for dst in IDS[:3] for src in IDS[:3]]
    lcs += [lc_bytes(4, 0, 0x76, 0x414243, 0x444546), lc_bytes(0x80 | 5, 0x10, 0x91, 0x808182, 0xFEFF00), lc_bytes(0x40 | 7, 0, 0xFF, 0, 0)]
    lcs += [rb(9) for _ in range(8)]
    for i, lc in enumerate(lcs):
        cc = COLOUR_CODES[i % len(COLOUR_CODES)]
        for dt in (1, 2):
            recs.append(record(K_LC, cc=cc, dt=dt, lc=lc))
        for fn in (0, 1, 2, 3, 4, 5, 6, 7, 255):
            recs.append(record(K_VOICE, fn=fn, cc=cc, lc=lc, payload=rb(27)))
    for dt in (0, 3, 9, 15):
        recs.append(record(K_LC, cc=1, dt=dt, lc=lcs[1]))
    for cc in COLOUR_CODES:
        for rep in range(6):
            csbk = bytearray(rb(10))
            csbk[0] = (csbk[0] & 0xC0) | dmr_l2.CSBK_CASES[(rep + cc) % len(dmr_l2.CSBK_CASES)][0]
            recs.append(record(K_CSBK, cc=cc, dt=3, payload=csbk))
            hdr = bytearray(rb(10))
            hdr[0] = (hdr[0] & 0xF0) | dmr_l2.DPF_CASES[(rep + cc) % len(dmr_l2.DPF_CASES)]
            if rep == 0:
                hdr[0], hdr[9] = hdr[0] & 0xF0, hdr[9] | 1          # a UDT header whose bit 0 of byte 9 get() clears
            recs.append(record(K_DATA_HEADER, cc=cc, dt=6, payload=hdr))
            recs.append(record(K_RATE12, cc=cc, dt=7, payload=rb(12)))
            recs.append(record(K_RATE34, cc=cc, dt=8, payload=rb(18)))
            recs.append(record(K_VOICE_SYNC, fn=rep, cc=cc, lc=rb(9), payload=rb(27)))
        recs.append(record(K_CSBK, cc=cc, dt=4, payload=rb(10)))          # a slot type other than the kind's usual one
        recs.append(record(K_RATE12, cc=cc, dt=0, payload=rb(12)))
        recs.append(record(K_EMPTY, cc=cc, dt=int(rng.randint(16)), lc=rb(9), payload=rb(27)))
    for kind in (6, 9, 10, 0x80, 255):
        recs.append(record(kind, fn=1, cc=3, dt=1, lc=rb(9), payload=rb(27)))
    recs.append(record(K_VOICE, fn=1, cc=0xF3, lc=lcs[0], payload=rb(27)))   # only the colour code's low four bits are sent
    recs.append(record(K_RATE12, cc=0x2F, dt=0x17, payload=rb(12)))
    return np.stack(recs)


def build_calls(seed=SEED + 1):
    """-> calls [m, 40], repeater [m], voice [m, CALL_VOICE, 27]"""
    rng = np.random.RandomState(seed)
    calls, rep = [], []
    k = 0
    for length in ALIAS_LENGTHS:
        for group in (True, False):
            alias = rng.randint(1, 256, length).astype(np.uint8)
            if length:
                alias[::2] |= 0x80
            calls.append(descriptor(IDS[k % 4], IDS[(k // 2 + 1) % 4], group, 0xC2 if k % 3 == 1 else 0, COLOUR_CODES[k % 3], alias))
            rep.append(k % 2)
            k += 1
    calls.append(descriptor(1234567, 91, True, 0, 1, b"YO8RZZ Adrian"))      # a text alias, zero bytes behind it
    rep.append(0)
    voice = rng.randint(0, 256, (len(calls), CALL_VOICE, 27)).astype(np.uint8)
    return np.stack(calls), np.array(rep, np.uint8), voice


def record_golden(ref):
    records = build_records()
    calls, repeater, voice = build_calls()
    frames = np.zeros((calls.shape[0], CALL_SLOTS_MAX, BURST), np.uint8)
    nslots, extra = np.zeros(calls.shape[0], np.int32), np.zeros(calls.shape[0], np.int32)
    for m in range(calls.shape[0]):
        f, e = ref.call(calls[m], repeater[m], voice[m])
        frames[m, :f.shape[0]], nslots[m], extra[m] = f, f.shape[0], e
    return dict(records=records, bursts=ref.bursts(records), calls=calls, call_repeater=repeater, call_voice=voice, call_frames=frames,
                call_nslots=nslots, call_extra=extra)


def load_golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def call_voice_frames(g, m):
    """the CALL_VOICE voice bursts of golden call m"""
    first = 3 * int(g["call_repeater"][m]) + 2
    return g["call_frames"][m, first:first + CALL_VOICE]


def dmo_records(bursts, ftype, fn=None, cc=None):
    """33-byte bursts -> the 40-byte records of the DMO slicer's mailbox (frame type, FN, colour code, 0, burst, 3 zero bytes)"""
    bursts = np.asarray(bursts, np.uint8).reshape(-1, BURST)
    rec = np.zeros((bursts.shape[0], 40), np.uint8)
    rec[:, 0] = ftype
    if fn is not None:
        rec[:, 1] = fn
    if cc is not None:
        rec[:, 2] = cc
    rec[:, 4:37] = bursts
    return rec


def embedded_lc(fragments):
    """four 33-byte voice bursts B..E of a superframe -> the 9 LC bytes and the 5-bit checksum their embedded fragments carry, by the rule
    of ETSI TS 102 361-1 B.2.1 (column de-interleave, data bits of the seven rows; no error correction: the test's bursts are clean)"""
    raw = []
    for b in fragments:
        bits = np.unpackbits(np.asarray(b, np.uint8))
        raw += list(bits[116:148])
    data = [0] * 128
    pos = 0
    for a in range(128):
        data[pos] = raw[a]
        pos += 16
        if pos > 127:
            pos -= 127
    lc, crc = [], 0
    for r in range(7):
        lc += data[16 * r:16 * r + (11 if r < 2 else 10)]
        if r >= 2:
            crc = (crc << 1) | data[16 * r + 10]
    return bytes(np.packbits(np.array(lc, np.uint8)).tolist()), crc


# ------------------------------------------------------------------------------------------------------------------ the radio loopback
RADIO_CALLS, RADIO_VOICE = (0, 2), 12          # the golden calls (DMO mode) and the voice bursts per call the radio loopback sends


def radio_call(g, m, n_voice=RADIO_VOICE):
    """-> (bytes [slots * 72], frames [slots, 33], zero runs [(T, count)]) of golden call m cut to n_voice voice bursts: 2 LC headers, the
    voice bursts, 2 terminators, 2 empty frames in 72-byte slots, and the tag gr_dmr_source puts on the first idle byte of each"""
    first, n = 3 * int(g["call_repeater"][m]), int(g["call_nslots"][m])
    frames = np.concatenate([g["call_frames"][m, first:first + 2 + n_voice], g["call_frames"][m, n - 4:n]])
    slots = np.zeros((frames.shape[0], 72), np.uint8)
    slots[:, :33] = frames
    return slots.reshape(-1), frames, [(20 * (72 * i + 33), 39 * 20) for i in range(frames.shape[0])]


def check_radio_records(g, rec, m, zero_runs, n_voice=RADIO_VOICE):
    """rec [n, 80]: the layer-2 records (audio FEC off) of what a DMR receiver delivered of radio_call(g, m).  The condition of the
    loopback: from some burst on every voice burst of the call with no gap, including a complete superframe (here: from the first burst
    on; the two LC headers are lead-in enough).  And every delivered burst decodes to what was encoded -- without zero runs in full; with
    them only in front of the burst's last 24 symbols, which the reference's gr_zero_idle_bursts blanks: its window opens 123 items of
    24 ksps before the burst's end (61 from its history of 1439 items against a slot of 1440, 62 from the pulse filter's delay, which it
    subtracts), so data bursts may fail validate() there and a voice burst keeps only the codec bytes that lie in front."""
    call, sent_voice = g["calls"][m], g["call_voice"][m, :n_voice]
    _, frames, _ = radio_call(g, m, n_voice)
    voice, data = rec[rec[:, 0] != 0], rec[rec[:, 0] == 0]
    # which sent burst a delivered one is: its first 13 bytes are far from anything the radio path damages
    which = [int(np.nonzero((frames[2:2 + n_voice, :13] == v[20:33]).all(axis=1))[0][0]) for v in voice]
    assert which == list(range(which[0], n_voice)), "a gap: %s" % which
    assert n_voice - which[0] >= 6 + (6 - which[0] % 6) % 6, "no complete superframe"
    assert which[0] == 0
    assert list(voice[:, 1]) == [k % 6 for k in which] and list(voice[:, 0]) == [1 if k % 6 else 2 for k in which]
    assert list(voice[:, 7]) == [(0, 1, 3, 3, 2, 0)[k % 6] for k in which] and (voice[voice[:, 0] == 1, 2] == call[8] & 15).all()
    own = bytes([call[6], call[7], 0]) + bytes(call[3:6]) + bytes(call[0:3])
    alias = bytes(call[9:36])
    lcs = [own, bytes([4, 0, 0x76]) + alias[:6]]
    for sf in range(n_voice // 6):
        lc, crc = embedded_lc(voice[6 * sf + 1:6 * sf + 5, 20:53])
        assert lc == lcs[sf] and crc == sum(lc) % 31, "superframe %d" % sf
    assert list(data[:, 3]) == [1, 1, 2] and (data[:, 2] == call[8] & 15).all()   # both headers, one terminator; empty frames carry no sync
    if zero_runs:
        assert np.array_equal(voice[:, 53:72], sent_voice[:, :19])    # 24.6 symbols and the pulse filter's reach: the last 8 codec bytes
        return
    # the slicer reads a burst's last dibit one lap early (tests/test_dmo_sink.py): BPTC corrects it, of a codec frame it is the last two bits
    assert np.array_equal(voice[:, 53:79], sent_voice[:, :26]) and not ((voice[:, 79] ^ sent_voice[:, 26]) & 0xFC).any()
    assert rec[:, 4].all()
    assert [bytes(d[53:62]) for d in data] == [own, own, own[:1] + b"\0" + own[2:]]      # the terminator's LC carries FID 0
    for d in data:
        assert int.from_bytes(bytes(d[12:16]), "little") == int.from_bytes(bytes(call[0:3]), "big")
        assert int.from_bytes(bytes(d[16:20]), "little") == int.from_bytes(bytes(call[3:6]), "big")
