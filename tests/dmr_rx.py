"""DMR receive call layer for the tests: the reference's own DMRControl behind tests/host/dmr_rx_ref.cpp (load_ref, where the reference is
present), the scalar core behind tests/host/dmr_rx_core_shim.cpp (load_core), the scenario set that tools/make_dmr_rx_golden.py records into
tests/golden/ref/dmr_rx.npz, and small helpers the CPU and GPU tests share.  The records are those of include/qrl_hip.h.  A scenario is
built as TX records (tests/dmr_tx.py), turned into bursts by the reference's own encoders, damaged where the scenario says so, and wrapped
into the 40-byte records of the DMO slicer's mailbox."""
import ctypes as C
import os
import subprocess

import numpy as np

import dmr_l2
import dmr_tx

ROOT = dmr_l2.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref", "dmr_rx.npz")
REFERENCE, REF_LIB = dmr_l2.REFERENCE, dmr_l2.REF_LIB
STUBS = (os.path.join(ROOT, "tests", "host", "dmr_rx_stub"), os.path.join(ROOT, "tests", "host", "dmr_ctl_stub"))

REC, STATE_BYTES, STATE_PUBLIC, TA_MAX = 128, 128, 12, 68
VALID, PROCESSED, HEADER_VOICE, HEADER_DATA, TERMINATOR, END_BEEP, AUDIO, EMBEDDED, TALKER_ALIAS, GPS, UNKNOWN_FLCO = (1 << i for i in range(11))
IDLE, LATE_ENTRY, AUDIO_STATE, DATA_STATE = 0, 1, 2, 3
AUDIO_FEC = 1


def flags(rec):
    rec = np.asarray(rec, np.uint8)
    return rec[..., 0].astype(np.int32) | (rec[..., 1].astype(np.int32) << 8)


def ids(rec):
    """(source, destination) of a record"""
    return int.from_bytes(bytes(rec[8:12]), "little"), int.from_bytes(bytes(rec[12:16]), "little")


def alias_of(rec):
    """(format, length field, bytes) of a record with TALKER_ALIAS"""
    return int(rec[26]), int(rec[27]), bytes(rec[32:32 + int(rec[28])])


# ------------------------------------------------------------------------------------------------------------------ the reference, the core
class Ref:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.ref_dmr_rx_new.restype = C.c_void_p
        lib.ref_dmr_rx_new.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.ref_dmr_rx_set_config.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.ref_dmr_rx_free.argtypes = [C.c_void_p]
        lib.ref_dmr_rx_step.argtypes = [C.c_void_p, u8p, u8p]
        lib.ref_dmr_rx_alias_pending.argtypes = [C.c_void_p, u8p, C.c_int]
        lib.ref_embedded_decode.argtypes = [C.POINTER(C.c_uint32), u8p, C.POINTER(C.c_int)]

    def run(self, inputs, cc, promiscuous, pending=None):
        """[n, 40] slicer records of one stream through a fresh DMRControl -> [n, 128]; pending, a list, receives the number of alias bytes
        the control holds after every burst"""
        inputs = np.ascontiguousarray(inputs, np.uint8).reshape(-1, 40)
        h = self.lib.ref_dmr_rx_new(int(cc), int(promiscuous), AUDIO_FEC)
        out = np.zeros((inputs.shape[0], REC), np.uint8)
        try:
            for i in range(inputs.shape[0]):
                src, dst = bytearray(inputs[i].tobytes()), bytearray(REC)
                rc = self.lib.ref_dmr_rx_step(h, dmr_tx.Ref.buf(src), dmr_tx.Ref.buf(dst))
                assert rc == 0, "burst %d: the shim's two DMRControl objects disagree (%d)" % (i, rc)
                out[i] = np.frombuffer(bytes(dst), np.uint8)
                if pending is not None:
                    scratch = bytearray(256)
                    pending.append(self.lib.ref_dmr_rx_alias_pending(h, dmr_tx.Ref.buf(scratch), 256))
        finally:
            self.lib.ref_dmr_rx_free(h)
        return out

    def embedded(self, frag):
        """four fragments (ints, first bit highest) -> (isValid(), getFLCO(), m_data as nine bytes)"""
        f, d, flco = (C.c_uint32 * 4)(*[int(x) for x in frag]), bytearray(9), C.c_int(0)
        ok = self.lib.ref_embedded_decode(f, dmr_tx.Ref.buf(d), C.byref(flco))
        return bool(ok), flco.value, bytes(d)


def load_ref(build_dir):
    """the reference behind tests/host/dmr_rx_ref.cpp, compiled into build_dir together with its src/DMR/dmrcontrol.cpp; None where the
    reference is absent"""
    if not (os.path.isdir(os.path.join(REFERENCE, "src", "MMDVM")) and os.path.isfile(REF_LIB)):
        return None
    so = os.path.join(str(build_dir), "libdmr_rx_ref.so")
    subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC"] + ["-D%s=dmr_rx_ref_%s" % (n, n) for n in dmr_tx.RENAMED]
                          + [os.path.join(ROOT, "tests", "host", "dmr_rx_ref.cpp"), os.path.join(REFERENCE, "src", "DMR", "dmrcontrol.cpp")]
                          + ["-I" + s for s in STUBS]
                          + ["-I" + REFERENCE, "-I" + os.path.join(REFERENCE, "src", "MMDVM"), "-I" + os.path.join(ROOT, "oracle", "gr_stub"),
                             "-o", so, "-L" + os.path.dirname(REF_LIB), "-lqrl_ref", "-Wl,-rpath," + os.path.dirname(REF_LIB)])
    return Ref(C.CDLL(so))


class Core:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.core_dmr_rx_run.argtypes = [C.c_int, C.c_int, C.c_int, u8p, u8p, C.c_size_t, u8p, u8p]
        lib.core_dmr_rx_run_l2.argtypes = [C.c_int, C.c_int, u8p, u8p, C.c_size_t, u8p, C.c_int]
        lib.core_dmr_rx_run_l2.restype = None
        lib.core_embedded_decode.argtypes = [C.POINTER(C.c_uint32), u8p]

    def run(self, inputs, cc, promiscuous, state=None):
        """-> (out [n, 128], l2 [n, 80], state bytearray, the most alias bytes the state held)"""
        inputs = np.ascontiguousarray(inputs, np.uint8).reshape(-1, 40)
        n = inputs.shape[0]
        state = bytearray(STATE_BYTES) if state is None else state
        src, l2, out = bytearray(inputs.tobytes()) or bytearray(1), bytearray(80 * n or 1), bytearray(REC * n or 1)
        most = self.lib.core_dmr_rx_run(int(cc), int(promiscuous), AUDIO_FEC, dmr_tx.Ref.buf(state), dmr_tx.Ref.buf(src), n, dmr_tx.Ref.buf(l2),
                                        dmr_tx.Ref.buf(out))
        return (np.frombuffer(bytes(out), np.uint8)[:REC * n].reshape(n, REC).copy(), np.frombuffer(bytes(l2), np.uint8)[:80 * n].reshape(n, 80).copy(),
                state, most)

    def embedded(self, frag):
        """-> (embedded_lc_decode's code: 0 row, 1 column parity, 2 checksum, 3 good; the nine bytes it wrote)"""
        f, d = (C.c_uint32 * 4)(*[int(x) for x in frag]), bytearray(9)
        code = self.lib.core_embedded_decode(f, dmr_tx.Ref.buf(d))
        return code, bytes(d)


def load_core(build_dir):
    so = os.path.join(str(build_dir), "libdmr_rx_core.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "dmr_rx_core_shim.cpp"),
                           "-o", so])
    return Core(C.CDLL(so))


# ------------------------------------------------------------------------------------------------------------------ the embedded LC by rule
H15 = (0x1AF, 0x35E, 0x6BC, 0x4D7)     # ETSI TS 102 361-1 B.3.5: the data bits of the four Hamming (15,11,3) parities


def embedded_matrix(lc9, crc=None):
    """nine LC bytes -> the 8 x 16 matrix of ETSI TS 102 361-1 B.2.1 as rows of bits; crc replaces the 5-bit checksum"""
    bits = [int(b) for b in np.unpackbits(np.frombuffer(bytes(lc9), np.uint8))]
    crc = sum(bytes(lc9)) % 31 if crc is None else crc
    rows, pos = [], 0
    for r in range(7):
        n = 11 if r < 2 else 10
        d = bits[pos:pos + n]
        pos += n
        if r >= 2:
            d.append((crc >> (6 - r)) & 1)
        row = d + [sum(d[j] for j in range(11) if (m >> j) & 1) & 1 for m in H15]
        rows.append(row + [sum(row) & 1])
    rows.append([sum(rows[r][c] for r in range(7)) & 1 for c in range(16)])
    return rows


def matrix_fragments(rows):
    """the matrix read by columns -> four 32-bit fragments, first bit highest"""
    raw = [rows[a % 8][a // 8] for a in range(128)]
    return [int("".join(str(b) for b in raw[32 * k:32 * k + 32]), 2) for k in range(4)]


def put_fragment(burst, frag):
    """the 32 embedded bits of a voice burst B..F (bits 116..147) replaced"""
    bits = np.unpackbits(np.asarray(burst, np.uint8))
    bits[116:148] = [(frag >> (31 - j)) & 1 for j in range(32)]
    return np.packbits(bits)


def get_fragment(burst):
    bits = np.unpackbits(np.asarray(burst, np.uint8))
    return int("".join(str(int(b)) for b in bits[116:148]), 2)


# ------------------------------------------------------------------------------------------------------------------ the scenario set
K = dmr_tx


def lc(flco, src, dst, fid=0, options=0):
    return K.lc_bytes(flco, fid, options, dst, src)


def voice27(k):
    return bytes([(k * 7 + 1) & 255] * 27)


class Stream:
    """a stream under construction: TX records, the frame type the slicer gives each, and what is done to each burst afterwards"""

    def __init__(self, name, cc, promiscuous, reconfig=None):
        self.name, self.cc, self.promiscuous, self.reconfig = name, cc, promiscuous, reconfig
        self.tx, self.ftype, self.post = [], [], []

    def add(self, rec, ftype, post=None):
        self.tx.append(rec)
        self.ftype.append(ftype)
        self.post.append(post)
        return self

    def header(self, l, cc):
        return self.add(K.record(K.K_LC, cc=cc, dt=1, lc=l), 0)

    def terminator(self, l, cc):
        return self.add(K.record(K.K_LC, cc=cc, dt=2, lc=l), 0)

    def csbk(self, cc):
        return self.add(K.record(K.K_CSBK, cc=cc, dt=3, payload=bytes([0x04, 0, 0, 0, 0, 0, 9, 0, 0, 7])), 0)

    def data_header(self, cc, src, dst):
        pay = bytes([0x02, 0x00]) + dst.to_bytes(3, "big") + src.to_bytes(3, "big") + bytes([0x02, 0x00])
        return self.add(K.record(K.K_DATA_HEADER, cc=cc, dt=6, payload=pay), 0)

    def rate12(self, cc, dt=7):
        return self.add(K.record(K.K_RATE12, cc=cc, dt=dt, payload=bytes(range(12))), 0)

    def voice(self, fn, l, cc, post=None):
        k = len(self.tx)
        if fn == 0:
            return self.add(K.record(K.K_VOICE_SYNC, fn=0, cc=cc, payload=voice27(k)), 2, post)
        return self.add(K.record(K.K_VOICE, fn=fn, cc=cc, lc=l, payload=voice27(k)), 1, post)

    def superframe(self, l, cc, fns=(0, 1, 2, 3, 4, 5), flips=(), crc=None):
        """voice bursts FN fns of a superframe that carries l.  flips: (row, column) of matrix bits to invert; crc: a checksum to send in
        place of the right one (the rows and the column parity are made for it)"""
        frags = matrix_fragments(embedded_matrix(l, crc)) if crc is not None else None
        for fn in fns:
            ops = []
            if frags is not None and 1 <= fn <= 4:
                ops.append(lambda b, f=frags[fn - 1]: put_fragment(b, f))
            for r, c in flips:
                a = 8 * c + r
                if a // 32 == fn - 1:
                    ops.append(lambda b, j=116 + a % 32: flip_bit(b, j))
            self.voice(fn, l, cc, (lambda b, ops=ops: apply_all(b, ops)) if ops else None)
        return self


def flip_bit(burst, j):
    b = np.array(burst, np.uint8)
    b[j >> 3] ^= 0x80 >> (j & 7)
    return b


def apply_all(burst, ops):
    for op in ops:
        burst = op(burst)
    return burst


def alias_lcs(df, dl, data, blocks=3):
    """the LCs of a talker alias: the header (format df, length field dl; the low bit of its options byte is data[0]'s for 7-bit text) and
    `blocks` blocks over data"""
    data = bytes(data) + bytes(64)
    out = [bytes([4, 0, (df << 6) | (dl << 1) | (data[0] & 1 if df == 0 else 0)]) + data[1 if df == 0 else 0:][:6]]
    at = 7 if df == 0 else 6
    for k in range(blocks):
        out.append(bytes([5 + k % 3, 0]) + data[at:at + 7])
        at += 7
    return out


A, B_, C_ = 0x2345A7, 91, 0xFFFFFF     # ids
OWN = lc(0, A, B_)
PRIVATE = lc(3, 1234567, 7654321, fid=0xC2)
TEXT = b"YO8RZZ Adrian".ljust(27, b"\0")


def build_streams():
    s = []
    # 1 whole call: two headers, 31 voice bursts (the call's LC, alias header, blocks 1..3, the wrap), two terminators
    st = Stream("whole_call", 1, 0).header(OWN, 1).header(OWN, 1)
    for l in [OWN] + alias_lcs(1, 27, TEXT):
        st.superframe(l, 1)
    st.voice(0, OWN, 1).terminator(OWN, 1).terminator(OWN, 1)
    s.append(st)
    # 2 late entry from voice A: promiscuous, a fixed colour code other than 0, colour code 0
    for name, cc, prom in (("late_entry_promiscuous", 1, 1), ("late_entry_fixed", 1, 0), ("late_entry_fixed_zero", 0, 0)):
        s.append(Stream(name, cc, prom).superframe(PRIVATE, 1).superframe(OWN, 1).terminator(OWN, 1))
    # 3 late entry in mid-superframe: LCSS 3, LCSS 2, then a whole superframe
    s.append(Stream("late_entry_mid_superframe", 4, 1).superframe(OWN, 4, fns=(3, 4, 5)).superframe(PRIVATE, 4).terminator(PRIVATE, 4))
    # 4 damaged fragments; every superframe carries another source, so a delivery shows in the state as well
    st = Stream("damaged_fragments", 2, 1)
    st.superframe(lc(0, 101, 9), 2, flips=[(0, 0), (1, 10), (2, 11), (3, 15), (4, 5), (5, 14), (6, 7)])      # one per row: corrected
    st.superframe(lc(0, 102, 9), 2, flips=[(2, 3), (2, 7)])                                                # two in one row: refused
    st.superframe(lc(0, 103, 9), 2)
    st.superframe(lc(0, 104, 9), 2, flips=[(7, 5)])                                                        # the parity row alone: column parity
    st.superframe(lc(0, 105, 9), 2)
    st.superframe(lc(0, 106, 9), 2, crc=(sum(lc(0, 106, 9)) % 31) ^ 1)                                     # a consistent matrix, wrong checksum
    st.superframe(lc(0, 107, 9), 2)
    st.superframe(lc(0, 108, 9), 2, flips=[(4, 12), (4, 2)])                                               # a parity bit and a data bit of a row
    st.superframe(lc(0, 109, 9), 2, flips=[(3, 6), (7, 6)])                                                # corrected in the row, then the column fails
    st.superframe(lc(0, 110, 9), 2)
    s.append(st.terminator(lc(0, 110, 9), 2))
    # 5 voice A in the middle of an assembly (reset), and a second LCSS 1 in mid-assembly
    st = Stream("reset_in_mid_assembly", 6, 1).superframe(OWN, 6, fns=(0, 1, 2)).superframe(OWN, 6, fns=(0,)).superframe(OWN, 6, fns=(3, 4, 5))
    st.superframe(OWN, 6, fns=(0, 1, 2)).superframe(PRIVATE, 6, fns=(1, 2, 3, 4, 5))
    s.append(st.terminator(PRIVATE, 6))
    # 6 terminators: while idle, with no ids, of another colour code, the real one
    st = Stream("terminators", 1, 0).terminator(OWN, 1).header(OWN, 1).superframe(OWN, 1).terminator(lc(0, 0, 0), 1).voice(0, OWN, 1)
    s.append(st.terminator(OWN, 2).voice(0, OWN, 1).terminator(OWN, 1).terminator(OWN, 1))
    # 7 promiscuous lock: the first call's colour code holds until its terminator
    st = Stream("promiscuous_lock", 9, 1).csbk(3).header(OWN, 3).superframe(OWN, 3)
    st.header(PRIVATE, 5).csbk(5).superframe(PRIVATE, 5).terminator(PRIVATE, 5)
    s.append(st.terminator(OWN, 3).header(PRIVATE, 5).superframe(PRIVATE, 5).terminator(PRIVATE, 5))
    # 8 talker alias
    seven = bytes([1]) + bytes(range(0x41, 0x41 + 20))
    st = Stream("alias_formats_0_2", 1, 0).header(OWN, 1)
    for l in alias_lcs(0, 20, seven):                     # 7-bit: complete at 8 n / 7 >= 20, in block 2
        st.superframe(l, 1)
    st.terminator(OWN, 1).header(OWN, 1)
    for l in alias_lcs(2, 10, "Țară nouă".encode()[:13].ljust(27, b"\0")):   # UTF-8: complete in block 1
        st.superframe(l, 1)
    s.append(st.terminator(OWN, 1))
    wide = "Ионеску Ад".encode("utf-16-be")
    st = Stream("alias_format_3", 1, 0).header(OWN, 1)
    for l in alias_lcs(3, 10, wide):                      # UTF-16: complete at 20 bytes, in block 2
        st.superframe(l, 1)
    st.terminator(OWN, 1).header(OWN, 1)
    for l in alias_lcs(3, 31, bytes(range(1, 64)), blocks=8):   # the largest need: 62 bytes, eight blocks
        st.superframe(l, 1)
    s.append(st.terminator(OWN, 1))
    st = Stream("alias_corners", 1, 0).header(OWN, 1)
    for l in alias_lcs(1, 27, TEXT)[1:]:                  # blocks with no header: nothing is collected
        st.superframe(l, 1)
    st.superframe(alias_lcs(1, 6, b"ABCDEF")[0], 1)       # a length the header alone satisfies
    for l in alias_lcs(1, 27, TEXT):                      # a second alias in the same call
        st.superframe(l, 1)
    st.terminator(OWN, 1).header(OWN, 1)
    for l in alias_lcs(1, 0, b"GHIJKLMNOPQRS"):           # length 0: the header completes it, the blocks are passed over
        st.superframe(l, 1)
    st.terminator(OWN, 1).header(OWN, 1)
    for l in alias_lcs(1, 13, b"after the end")[:2]:      # an alias again after a terminator
        st.superframe(l, 1)
    st.terminator(OWN, 1).header(OWN, 1).superframe(alias_lcs(1, 27, TEXT)[0], 1).superframe(alias_lcs(1, 27, TEXT)[1], 1)
    st.terminator(OWN, 1).header(OWN, 1)                  # a terminator leaves a half-collected alias where it is: block 2 goes on from it
    st.superframe(alias_lcs(1, 27, TEXT)[2], 1).superframe(alias_lcs(1, 27, TEXT)[3], 1)
    s.append(st.terminator(OWN, 1))
    # 9, 10 embedded GPS info, and FLCOs the switch does not know
    st = Stream("gps_and_unknown_flco", 1, 0).header(OWN, 1).superframe(bytes([8, 0, 0x05, 0x12, 0x34, 0x56, 0x78, 0x9A, 0xBC]), 1)
    s.append(st.superframe(bytes([0x30, 0x10, 1, 2, 3, 4, 5, 6, 7]), 1).superframe(bytes([0x81, 0, 9, 8, 7, 6, 5, 4, 3]), 1).terminator(OWN, 1))
    # 11 data: header, rate 1/2 blocks, voice bursts
    st = Stream("data", 1, 0).data_header(1, A, B_).rate12(1).rate12(1).superframe(PRIVATE, 1).terminator(PRIVATE, 1)
    s.append(st.data_header(2, A, B_).data_header(1, C_, 1))
    # 12 pass-through: a CSBK, a burst validate() refuses between two fragments, a frame type the class does not know
    st = Stream("pass_through", 1, 0).csbk(1).csbk(2).header(OWN, 1).superframe(PRIVATE, 1, fns=(0, 1, 2)).rate12(1, dt=9)
    st.superframe(PRIVATE, 1, fns=(3,)).add(K.record(K.K_RATE12, cc=1, dt=7, payload=bytes(12)), 3).superframe(PRIVATE, 1, fns=(4, 5))
    s.append(st.terminator(PRIVATE, 1))
    # set_config between calls: a fixed colour code, then the other call's, then promiscuous, switched where `reconfig` says
    st = Stream("reconfigured", 1, 0, reconfig=[(8, 5, 0), (16, 1, 1)]).header(OWN, 1).superframe(OWN, 1).terminator(OWN, 1).header(PRIVATE, 5)
    s.append(st.superframe(PRIVATE, 5).terminator(PRIVATE, 5).header(OWN, 7).superframe(OWN, 7).terminator(OWN, 7))
    return s


def slicer_records(stream, tx_ref):
    bursts = tx_ref.bursts(np.stack(stream.tx))
    for i, post in enumerate(stream.post):
        if post is not None:
            bursts[i] = post(bursts[i])
    tx = np.stack(stream.tx)
    rec = dmr_tx.dmo_records(bursts, 0, fn=tx[:, 1], cc=tx[:, 2])
    rec[:, 0] = stream.ftype
    return rec


def reference_records(ref, inputs, cc, promiscuous, reconfig):
    """the stream through the reference, its configuration switched at the slots reconfig = [(slot, colour code, promiscuous)] names"""
    if not reconfig:
        return ref.run(inputs, cc, promiscuous)
    h = ref.lib.ref_dmr_rx_new(int(cc), int(promiscuous), AUDIO_FEC)
    out = np.zeros((inputs.shape[0], REC), np.uint8)
    change = {slot: (c, p) for slot, c, p in reconfig}
    try:
        for i in range(inputs.shape[0]):
            if i in change:
                ref.lib.ref_dmr_rx_set_config(h, *change[i])
            src, dst = bytearray(inputs[i].tobytes()), bytearray(REC)
            assert ref.lib.ref_dmr_rx_step(h, dmr_tx.Ref.buf(src), dmr_tx.Ref.buf(dst)) == 0
            out[i] = np.frombuffer(bytes(dst), np.uint8)
    finally:
        ref.lib.ref_dmr_rx_free(h)
    return out


def record_golden(ref, tx_ref):
    streams = build_streams()
    n = max(len(s.tx) for s in streams)
    inputs, expected = np.zeros((len(streams), n, 40), np.uint8), np.zeros((len(streams), n, REC), np.uint8)
    counts, config = np.zeros(len(streams), np.int32), np.zeros((len(streams), 2), np.int32)
    reconfig = np.zeros((0, 4), np.int32)
    for k, s in enumerate(streams):
        rec = slicer_records(s, tx_ref)
        inputs[k, :rec.shape[0]], counts[k], config[k] = rec, rec.shape[0], (s.cc, s.promiscuous)
        expected[k, :rec.shape[0]] = reference_records(ref, rec, s.cc, s.promiscuous, s.reconfig)
        for slot, c, p in s.reconfig or []:
            reconfig = np.concatenate([reconfig, np.array([[k, slot, c, p]], np.int32)])
    return dict(names=np.array([s.name for s in streams]), inputs=inputs, counts=counts, config=config, reconfig=reconfig, expected=expected)


def load_golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def scenario(g, name):
    """-> (index, inputs [n, 40], expected [n, 128], colour code, promiscuous, [(slot, colour code, promiscuous)])"""
    k = list(g["names"]).index(name)
    n = int(g["counts"][k])
    return k, g["inputs"][k, :n], g["expected"][k, :n], int(g["config"][k, 0]), int(g["config"][k, 1]), [tuple(int(v) for v in r[1:]) for r in g["reconfig"] if r[0] == k]


def plain(g):
    """the indices of the scenarios that keep one configuration"""
    moved = {int(r[0]) for r in g["reconfig"]}
    return [k for k in range(len(g["names"])) if k not in moved]
