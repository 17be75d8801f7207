"""M17 link layer for the tests: the reference's own gr_modem / M17FrameDecoder / M17Transmitter behind tests/host/m17_link_ref.cpp (load_ref,
where the reference is present), the scalar core behind tests/host/m17_link_core_shim.cpp (load_core), the scenario set that
tools/make_m17_link_golden.py records into tests/golden/ref/m17_link.npz, and small helpers the CPU and GPU tests share.  The records are
those of include/qrl_hip.h.  A receive scenario is built as 40-byte frame records (the layout of qrl_m17_decode_frames), turned into frames
by the oracle's encoder (oracle/orc_framefec.c, pinned against the reference's M17FrameEncoder), damaged where the scenario says so, and
wrapped into the 56-byte records of the frame synchroniser.  What the frames mean is never restated here: every expectation is the
reference's."""
import ctypes as C
import os
import subprocess

import numpy as np

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref", "m17_link.npz")
REFERENCE = "/root/reference"
REF_SOURCES = ("gr_modem.cpp", "M17/M17/M17Transmitter.cpp", "M17/M17/M17FrameDecoder.cpp", "M17/M17/M17LinkSetupFrame.cpp", "M17/M17/M17Callsign.cpp",
               "M17/M17/M17Golay.cpp", "M17/M17/M17FrameEncoder.cpp", "bursttimer.cpp")      # (gr_modem owns an M17FrameEncoder and a BurstTimer)

FS_REC, DEC_REC, REC, STATE_BYTES, STATE_PUBLIC, CALL_BYTES, START_BYTES, END_BYTES = 56, 40, 64, 64, 16, 32, 96, 64
FRAME, LSF_VALID, INFO, AUDIO, END, LICH_OK, LSF_FROM_LICH, LOCKED = (1 << i for i in range(8))
FT_LSF, FT_STREAM, FT_EOT = 0x55F7, 0xFF5D, 0x555D555D


def _buf(b):
    return (C.c_uint8 * len(b)).from_buffer(b)


def flags(rec):
    rec = np.asarray(rec, np.uint8)
    return rec[..., 0].astype(np.int32) | (rec[..., 1].astype(np.int32) << 8)


def texts(rec):
    """(source text, destination text) of a record"""
    return bytes(rec[21:21 + int(rec[20])]).decode("latin-1"), bytes(rec[32:32 + int(rec[31])]).decode("latin-1")


def public_state(state62):
    """the 16 public bytes from the reference's recorded state (lsf, lsfFromLich, map, lock): locked, lsf.valid(), CAN, map, source, destination"""
    s = np.asarray(state62, np.uint8)
    lsf = bytes(s[:30])
    out = np.zeros(STATE_PUBLIC, np.uint8)
    out[0], out[1] = s[61], int(crc16(lsf[:28]) == (lsf[28] << 8 | lsf[29]))
    out[2], out[3] = (((lsf[12] << 8) | lsf[13]) >> 7) & 15, s[60]
    out[4:10], out[10:16] = s[6:12], s[0:6]
    return out


# ------------------------------------------------------------------------------------------------------------------ the reference, the core
class Ref:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.ref_m17_new.restype = C.c_void_p
        lib.ref_m17_new.argtypes = [C.c_int, C.c_int]
        lib.ref_m17_free.argtypes = [C.c_void_p]
        lib.ref_m17_set_rx.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.ref_m17_state.argtypes = [C.c_void_p, u8p]
        lib.ref_m17_step.argtypes = [C.c_void_p, u8p, u8p]
        lib.ref_m17_rx_frame_length.argtypes = [C.c_void_p]
        lib.ref_m17_tx_frame_length.argtypes = [C.c_void_p]
        lib.ref_m17_set_tx.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        lib.ref_m17_tx_start.argtypes = [C.c_void_p]
        lib.ref_m17_tx_audio.argtypes = [C.c_void_p, u8p]
        lib.ref_m17_tx_end.argtypes = [C.c_void_p]
        lib.ref_m17_tx_take.argtypes = [C.c_void_p, u8p, C.c_size_t]
        lib.ref_m17_tx_take.restype = C.c_size_t

    def run(self, inputs, can_rx, decode_all_can, reconfig=()):
        """[n, 56] synchroniser records of one stream through a fresh gr_modem, its settings switched at the slots reconfig =
        [(slot, can_rx, decode_all_can)] names -> (records [n, 64], the decoder's state after every frame [n, 62])"""
        inputs = np.ascontiguousarray(inputs, np.uint8).reshape(-1, FS_REC)
        h = self.lib.ref_m17_new(int(can_rx), int(decode_all_can))
        out, states = np.zeros((inputs.shape[0], REC), np.uint8), np.zeros((inputs.shape[0], 62), np.uint8)
        change = {slot: (c, a) for slot, c, a in reconfig}
        try:
            assert self.lib.ref_m17_rx_frame_length(h) == 46
            for i in range(inputs.shape[0]):
                if i in change:
                    self.lib.ref_m17_set_rx(h, *change[i])
                src, dst, st = bytearray(inputs[i].tobytes()), bytearray(REC), bytearray(62)
                rc = self.lib.ref_m17_step(h, _buf(src), _buf(dst))
                assert rc == 0, "frame %d: the recorder's cross-checks failed (%d)" % (i, rc)
                self.lib.ref_m17_state(h, _buf(st))
                out[i], states[i] = np.frombuffer(bytes(dst), np.uint8), np.frombuffer(bytes(st), np.uint8)
        finally:
            self.lib.ref_m17_free(h)
        return out, states

    def call(self, source, destination, can, destination_type, payloads):
        """a whole transmission -> (start bytes, the stream frames' bytes, end bytes) as gr_mod_base::set_data received them"""
        payloads = np.ascontiguousarray(payloads, np.uint8).reshape(-1, 16)
        h = self.lib.ref_m17_new(0, 1)
        scratch = bytearray(256)
        try:
            assert self.lib.ref_m17_tx_frame_length(h) == 16
            self.lib.ref_m17_set_tx(h, source, destination, int(can), int(destination_type))
            self.lib.ref_m17_tx_start(h)
            start = bytes(scratch[:self.lib.ref_m17_tx_take(h, _buf(scratch), 256)])
            frames = []
            for p in payloads:
                one = bytearray(p.tobytes())
                self.lib.ref_m17_tx_audio(h, _buf(one))
                frames.append(bytes(scratch[:self.lib.ref_m17_tx_take(h, _buf(scratch), 256)]))
            self.lib.ref_m17_tx_end(h)
            end = bytes(scratch[:self.lib.ref_m17_tx_take(h, _buf(scratch), 256)])
        finally:
            self.lib.ref_m17_free(h)
        return np.frombuffer(start, np.uint8), np.frombuffer(b"".join(frames), np.uint8), np.frombuffer(end, np.uint8)


def load_ref(build_dir):
    """the reference behind tests/host/m17_link_ref.cpp, compiled into build_dir together with its own sources; None where the reference is absent"""
    src = os.path.join(REFERENCE, "src")
    if not all(os.path.isfile(os.path.join(src, f)) for f in REF_SOURCES):
        return None
    so = os.path.join(str(build_dir), "libm17_link_ref.so")
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-Dnanosleep=qrl_stub_nanosleep",
                           os.path.join(ROOT, "tests", "host", "m17_link_ref.cpp")] + [os.path.join(src, f) for f in REF_SOURCES]
                          + ["-I" + os.path.join(oracle, "qt_stub"), "-I" + os.path.join(oracle, "gr_stub"), "-I" + REFERENCE,
                             "-I" + os.path.join(src, "MMDVM"), "-I" + os.path.join(src, "M17"), "-o", so])
    return Ref(C.CDLL(so))


class Core:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.core_m17_fresh.argtypes = [u8p]
        lib.core_m17_rx_run.argtypes = [C.c_int, C.c_int, u8p, u8p, u8p, C.c_size_t, u8p, C.c_int]
        lib.core_m17_rx_run.restype = None
        lib.core_m17_public.argtypes = [u8p, u8p]
        lib.core_m17_call_record.argtypes = [C.c_int, u8p, C.c_uint32, u8p, u8p]

    def fresh(self):
        st = bytearray(STATE_BYTES)
        self.lib.core_m17_fresh(_buf(st))
        return st

    def run(self, inputs, can_rx, decode_all_can, state=None, reps=1):
        """[n, 56] synchroniser records -> (out [n, 64], state bytearray); the decode stage is the oracle's"""
        inputs = np.ascontiguousarray(inputs, np.uint8).reshape(-1, FS_REC)
        n = inputs.shape[0]
        state = self.fresh() if state is None else state
        dec = decode_records(inputs)
        src, d, out = bytearray(inputs.tobytes()) or bytearray(1), bytearray(dec.tobytes()) or bytearray(1), bytearray(REC * n or 1)
        self.lib.core_m17_rx_run(int(can_rx), int(decode_all_can), _buf(state), _buf(src), _buf(d), n, _buf(out), reps)
        return np.frombuffer(bytes(out), np.uint8)[:REC * n].reshape(n, REC).copy(), state

    def public(self, state):
        out = bytearray(STATE_PUBLIC)
        self.lib.core_m17_public(_buf(bytearray(state)), _buf(out))
        return np.frombuffer(bytes(out), np.uint8)

    def call_records(self, desc, payloads, first=0):
        """the 40-byte records of stream frames first .. of a call"""
        payloads = np.ascontiguousarray(payloads, np.uint8).reshape(-1, 16)
        d, out = bytearray(np.asarray(desc, np.uint8).tobytes()), np.zeros((payloads.shape[0], DEC_REC), np.uint8)
        for i, p in enumerate(payloads):
            rec = bytearray(DEC_REC)
            self.lib.core_m17_call_record(1, _buf(d), first + i, _buf(bytearray(p.tobytes())), _buf(rec))
            out[i] = np.frombuffer(bytes(rec), np.uint8)
        return out

    def call_start(self, desc):
        d, rec = bytearray(np.asarray(desc, np.uint8).tobytes()), bytearray(DEC_REC)
        self.lib.core_m17_call_record(0, _buf(d), 0, None, _buf(rec))
        return np.concatenate([np.full(48, 0x77, np.uint8), encode_frames(np.frombuffer(bytes(rec), np.uint8).reshape(1, DEC_REC))[0]])

    def call_end(self, desc, first):
        d, rec = bytearray(np.asarray(desc, np.uint8).tobytes()), bytearray(DEC_REC)
        self.lib.core_m17_call_record(2, _buf(d), int(first), None, _buf(rec))
        return np.concatenate([encode_frames(np.frombuffer(bytes(rec), np.uint8).reshape(1, DEC_REC))[0], np.array([0x55, 0x5D] * 8, np.uint8)])


def load_core(build_dir):
    so = os.path.join(str(build_dir), "libm17_link_core.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "m17_link_core_shim.cpp"),
                           "-o", so])
    return Core(C.CDLL(so))


# ------------------------------------------------------------------------------------------------------------------ frames
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def encode_frames(records):
    """[n, 40] frame records -> [n, 48] frames (the oracle's M17 frame encoder)"""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, DEC_REC)
    out = np.zeros((records.shape[0], 48), np.uint8)
    for i in range(records.shape[0]):
        orc.lib.orc_m17_encode_frame(_p(np.ascontiguousarray(records[i])), _p(out[i]))
    return out


def decode_records(inputs):
    """the decode stage on the CPU: [n, 56] synchroniser records -> [n, 40] decode records (the oracle's M17 frame decoder on the frames the
    device decodes: LSF and stream frames of 46 bytes; zeros elsewhere)"""
    inputs = np.ascontiguousarray(inputs, np.uint8).reshape(-1, FS_REC)
    out = np.zeros((inputs.shape[0], DEC_REC), np.uint8)
    head = inputs[:, :8].copy().view("<u4")
    for i in range(inputs.shape[0]):
        if (int(head[i, 1]) & 0xFFFF) == 46 and int(head[i, 0]) in (FT_LSF, FT_STREAM):
            frame = np.concatenate([np.array([int(head[i, 0]) >> 8, int(head[i, 0]) & 255], np.uint8), inputs[i, 8:54]])
            orc.lib.orc_m17_decode_frame(_p(frame), _p(out[i]))
    return out


def fs_record(frame=None, ftype=None, nbytes=46, modem_sync=8):
    """a 48-byte frame (its sync word names the type), or 46 bytes behind an explicit frame type -> the synchroniser's 56-byte record"""
    rec = np.zeros(FS_REC, np.uint8)
    if ftype is None:
        ftype, body = (int(frame[0]) << 8) | int(frame[1]), np.asarray(frame[2:48], np.uint8)
    else:
        body = np.asarray(frame if frame is not None else [0x55, 0x5D] * 23, np.uint8)
    rec[0:8] = np.array([ftype, nbytes | (modem_sync << 16)], "<u4").view(np.uint8)
    rec[8:54] = body
    return rec


def crc16(data):
    crc = 0xFFFF
    for b in bytes(data):
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x5935 if crc & 0x8000 else crc << 1) & 0xFFFF
    return crc


ALPHABET = "xABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-/."


def call6(text=None, value=None):
    """six address bytes: a base-40 value, big endian"""
    if value is None:
        value = 0
        for ch in reversed(text):
            value = value * 40 + ALPHABET.index(ch)
    return int(value).to_bytes(6, "big")


def make_lsf(src, dst, can=0, good_crc=True, meta=bytes(14)):
    """30 LSF bytes: destination, source (six bytes each, or text), type (stream, voice, CAN), META, CRC"""
    src = call6(src) if isinstance(src, str) else bytes(src)
    dst = call6(dst) if isinstance(dst, str) else bytes(dst)
    body = dst + src + (5 | (can << 7)).to_bytes(2, "big") + bytes(meta)
    crc = crc16(body) ^ (0 if good_crc else 0x0101)
    return body + crc.to_bytes(2, "big")


def lsf_frame(lsf):
    rec = np.zeros(DEC_REC, np.uint8)
    rec[0] = 1
    rec[2:32] = np.frombuffer(bytes(lsf), np.uint8)
    return encode_frames(rec)[0]


def stream_frame(lsf, k, payload=None, eos=False, seg=None, lich=None):
    """stream frame k of a call with the LSF lsf: frame number k & 0x7FF, the LICH segment seg (k % 6) of lsf, or five bytes `lich` given"""
    rec = np.zeros(DEC_REC, np.uint8)
    seg = k % 6 if seg is None else seg
    fn = (k & 0x7FF) | (0x8000 if eos else 0)
    rec[0], rec[1], rec[2], rec[3] = 2, 1, fn >> 8, fn & 255
    rec[4:20] = payload_of(k) if payload is None else np.frombuffer(bytes(payload), np.uint8)
    rec[32:37] = np.frombuffer(bytes(lich) if lich is not None else bytes(lsf)[5 * seg:5 * seg + 5], np.uint8)
    rec[37] = seg
    return encode_frames(rec)[0]


def payload_of(k, salt=0):
    return np.array([(salt * 31 + k * 7 + j * 3 + 1) & 255 for j in range(16)], np.uint8)


def flip_body_bits(frame, bits):
    """bits of the frame's 368 code bits as they stand in front of the interleaver (0..95: the LICH's four Golay words) inverted"""
    f = np.array(frame, np.uint8)
    for i in bits:
        d = (45 * i + 92 * i * i) % 368
        f[2 + (d >> 3)] ^= 0x80 >> (d & 7)
    return f


# ------------------------------------------------------------------------------------------------------------------ the receive scenarios
class Stream:
    def __init__(self, name, can_rx=0, decode_all_can=1, reconfig=None):
        self.name, self.can_rx, self.decode_all_can, self.reconfig = name, can_rx, decode_all_can, reconfig or []
        self.rec = []

    def lsf(self, lsf, damage=False):
        f = lsf_frame(lsf)
        if damage:
            f = np.array(f)
            f[6:30] ^= 0xFF        # 192 of the 368 code bits inverted: the Viterbi cannot give back the LSF
        self.rec.append(fs_record(f))
        return self

    def frames(self, lsf, ks, eos_last=False, **kw):
        ks = list(ks)
        for k in ks:
            self.rec.append(fs_record(stream_frame(lsf, k, eos=eos_last and k == ks[-1], **kw)))
        return self

    def frame(self, f):
        self.rec.append(fs_record(f))
        return self

    def eot(self):
        self.rec.append(fs_record(ftype=FT_EOT))
        return self

    def raw(self, rec):
        self.rec.append(rec)
        return self


A_LSF = make_lsf("YO8RZZ", "AB1CDE", can=0)
B_LSF = make_lsf("N0CALL-9", "W1AW/P", can=5)
C_LSF = make_lsf("DL1ABC.M", bytes([0xFF] * 6), can=15)
BAD_LSF = make_lsf("BAD", "CRC", can=2, good_crc=False)
DESTINATIONS = {0: call6("AB1CDE"), 1: bytes([0xFF] * 6), 2: bytes([0, 0, 0, 0x0E, 0xD8, 0x7D]), 3: bytes([0, 0, 0, 0x0E, 0xCD, 0xB9]),
                4: bytes([0, 0, 0x45, 0x4F, 0x77, 0x45])}


def build_streams():
    s = []
    # an LSF, then stream frames, then the EOT
    s.append(Stream("lsf_then_stream").lsf(A_LSF).frames(A_LSF, range(8)).eot())
    # late entry with no LSF, from every phase of the LICH round robin
    for phase in range(6):
        s.append(Stream("late_entry_phase_%d" % phase).frames(B_LSF, range(phase, phase + 9)).eot())
    # one segment's Golay word uncorrectable: the map stalls, the next round completes it
    st = Stream("lich_golay_uncorrectable").frames(A_LSF, range(0, 3))
    st.frame(flip_body_bits(stream_frame(A_LSF, 3), [24, 27, 31, 40]))           # four errors in the second Golay word of segment 3
    s.append(st.frames(A_LSF, range(4, 11)).eot())
    # a completed round with a bad CRC: the LSF is kept, the map cleared
    s.append(Stream("lich_round_bad_crc").lsf(A_LSF).frames(BAD_LSF, range(0, 6)).frames(B_LSF, range(6, 14)).eot())
    # a damaged LSF frame over a valid LSF: audio stops until a LICH round restores it
    s.append(Stream("damaged_lsf_over_valid").lsf(A_LSF).frames(A_LSF, range(0, 3)).lsf(A_LSF, damage=True).frames(A_LSF, range(3, 11)).eot())
    # segment numbers 6 and 7
    for seg in (6, 7):
        st = Stream("segment_%d" % seg).frames(A_LSF, range(0, 2)).frames(A_LSF, [2], seg=seg, lich=b"\x11\x22\x33\x44\x55")
        s.append(st.frames(A_LSF, range(3, 10)).lsf(A_LSF).frames(A_LSF, range(10, 12)).eot().frames(B_LSF, range(0, 7)).eot())
    # the CAN filter
    s.append(Stream("can_filter_all", can_rx=3, decode_all_can=1).lsf(B_LSF).frames(B_LSF, range(4)).eot())
    s.append(Stream("can_filter_other", can_rx=3, decode_all_can=0).lsf(B_LSF).frames(B_LSF, range(4)).eot())
    s.append(Stream("can_filter_match", can_rx=5, decode_all_can=0).lsf(B_LSF).frames(B_LSF, range(4)).eot())
    s.append(Stream("can_filter_late_entry", can_rx=3, decode_all_can=0).frames(B_LSF, range(8)).eot())
    # EOT with an invalid LSF: nothing happens, no reset -- the half-collected round completes afterwards
    s.append(Stream("eot_invalid_lsf").eot().frames(A_LSF, range(0, 3)).eot().frames(A_LSF, range(3, 8)).eot().eot())
    # two calls back to back with different callsigns
    s.append(Stream("two_calls").lsf(A_LSF).frames(A_LSF, range(7)).eot().lsf(C_LSF).frames(C_LSF, range(7)).eot())
    # frame number wrap and the EOS bit
    s.append(Stream("frame_number_wrap").lsf(A_LSF).frames(A_LSF, range(2044, 2052), eos_last=True).eot())
    # destinations: what each destination_type writes, all 0xFF, the byte patterns getDestination() does name, ten characters; a digit-0 source
    st = Stream("destinations")
    for t in range(5):
        st.lsf(make_lsf("YO8RZZ", DESTINATIONS[t], can=t))
    st.lsf(make_lsf("YO8RZZ", bytes([0x12, 0x34, 0x7D, 0xD8, 0x0E, 0x00]), can=6))      # bytes 2..5 little endian = 0x000ED87D
    st.lsf(make_lsf("YO8RZZ", bytes([0x00, 0x00, 0xB9, 0xCD, 0x0E, 0x00]), can=7))
    st.lsf(make_lsf("YO8RZZ", bytes([0xAB, 0xCD, 0x45, 0x77, 0x4F, 0x45]), can=8))
    st.lsf(make_lsf("YO8RZZ", call6(value=40 ** 9 + 12345), can=9))                      # ten characters
    st.lsf(make_lsf(call6(value=0xFFFFFFFFFFFE), call6(value=40 ** 9 + 2 * 40 ** 8 + 39), can=10))
    st.lsf(make_lsf(call6(value=1 + 0 * 40 + 2 * 1600 + 0 * 64000 + 27 * 2560000), "A", can=11))   # digit 0 inside a source: "AxBx0"
    st.lsf(make_lsf(bytes(6), bytes(6), can=12))                                         # the zero address: an empty text
    s.append(st.frames(make_lsf(bytes(6), bytes(6), can=12), range(2)).eot())
    # records the link layer passes over: another size, another frame type
    st = Stream("passed_over").lsf(A_LSF).frames(A_LSF, range(2))
    st.raw(fs_record(stream_frame(A_LSF, 2), nbytes=47)).raw(fs_record(stream_frame(A_LSF, 2)[2:], ftype=0x89EDAA))
    s.append(st.frames(A_LSF, range(2, 4)).eot())
    # set_config between calls
    st = Stream("reconfigured", can_rx=5, decode_all_can=0, reconfig=[(6, 0, 0), (12, 9, 1)]).lsf(B_LSF).frames(B_LSF, range(4)).eot()
    s.append(st.lsf(B_LSF).frames(B_LSF, range(4)).eot().lsf(A_LSF).frames(A_LSF, range(4)).eot())
    return s


def record_golden(ref):
    streams = build_streams()
    n = max(len(s.rec) for s in streams)
    S = len(streams)
    inputs, expected, states = np.zeros((S, n, FS_REC), np.uint8), np.zeros((S, n, REC), np.uint8), np.zeros((S, n, 62), np.uint8)
    counts, config, reconfig = np.zeros(S, np.int32), np.zeros((S, 2), np.int32), np.zeros((0, 4), np.int32)
    for k, s in enumerate(streams):
        rec = np.stack(s.rec)
        inputs[k, :rec.shape[0]], counts[k], config[k] = rec, rec.shape[0], (s.can_rx, s.decode_all_can)
        expected[k, :rec.shape[0]], states[k, :rec.shape[0]] = ref.run(rec, s.can_rx, s.decode_all_can, s.reconfig)
        for slot, c, a in s.reconfig:
            reconfig = np.concatenate([reconfig, np.array([[k, slot, c, a]], np.int32)])
    g = dict(names=np.array([s.name for s in streams]), inputs=inputs, counts=counts, config=config, reconfig=reconfig, expected=expected,
             states=states)
    g.update(record_tx_golden(ref))
    return g


# ------------------------------------------------------------------------------------------------------------------ the transmit scenarios
# (name, source, destination, CAN, destination_type, frames)
TX_CALLS = [("type_0", "YO8RZZ", "AB1CDE", 0, 0, 7), ("type_1", "YO8RZZ", "AB1CDE", 1, 1, 1), ("type_2", "YO8RZZ", "", 2, 2, 2), ("type_3", "YO8RZZ", "X", 3, 3, 5),
            ("type_4", "YO8RZZ", "AB1CDE", 4, 4, 6), ("empty_both", "", "", 0, 0, 0), ("empty_destination", "N0CALL", "", 15, 0, 3),
            ("nine_characters", "ABCDEFGH9", "Z9Y8X7W6V", 15, 0, 2), ("ten_characters", "ABCDEFGHIJ", "0123456789", 7, 0, 2),
            ("lower_case", "yo8rzz", "Ab1cDe", 0, 0, 2), ("punctuation", "A-B/C.D", "-/.", 9, 0, 2), ("unknown_characters", "A B_C", "#", 9, 0, 1),
            ("long_call", "YO8RZZ", "W1AW", 5, 0, 2050)]


def descriptor(source, destination, can, destination_type):
    import qradiolink_amd as q
    return q.m17_call_descriptor(source, destination, can, destination_type)


def tx_payloads(t, n):
    return np.stack([payload_of(k, salt=t + 1) for k in range(n)]) if n else np.zeros((0, 16), np.uint8)


def record_tx_golden(ref):
    desc, starts, ends, flat, pays, off = [], [], [], [], [], [0]
    for t, (name, src, dst, can, dtype, n) in enumerate(TX_CALLS):
        start, frames, end = ref.call(src.encode(), dst.encode(), can, dtype, tx_payloads(t, n))
        assert start.size == START_BYTES and frames.size == 48 * n and end.size == END_BYTES, (name, start.size, frames.size, end.size)
        desc.append(descriptor(src, dst, can, dtype))
        starts.append(start)
        ends.append(end)
        flat.append(frames)
        pays.append(tx_payloads(t, n).reshape(-1))
        off.append(off[-1] + frames.size)
    return dict(tx_names=np.array([c[0] for c in TX_CALLS]), tx_desc=np.stack(desc), tx_n=np.array([c[5] for c in TX_CALLS], np.int32),
                tx_start=np.stack(starts), tx_end=np.stack(ends), tx_frames=np.concatenate(flat), tx_payloads=np.concatenate(pays), tx_off=np.array(off, np.int64))


def load_golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def scenario(g, name):
    """-> (index, inputs [n, 56], expected [n, 64], states [n, 62], can_rx, decode_all_can, [(slot, can_rx, decode_all_can)])"""
    k = list(g["names"]).index(name)
    n = int(g["counts"][k])
    return (k, g["inputs"][k, :n], g["expected"][k, :n], g["states"][k, :n], int(g["config"][k, 0]), int(g["config"][k, 1]),
            [tuple(int(v) for v in r[1:]) for r in g["reconfig"] if r[0] == k])


def tx_call(g, name):
    """-> (index, descriptor, payloads [n, 16], start [96], frames [n, 48], end [64])"""
    t = list(g["tx_names"]).index(name)
    n = int(g["tx_n"][t])
    a, b = int(g["tx_off"][t]) // 3, int(g["tx_off"][t + 1]) // 3
    return t, g["tx_desc"][t], g["tx_payloads"][a:b].reshape(n, 16), g["tx_start"][t], g["tx_frames"][int(g["tx_off"][t]):int(g["tx_off"][t + 1])].reshape(n, 48), g["tx_end"][t]


def plain(g):
    """the indices of the scenarios that keep one configuration"""
    moved = {int(r[0]) for r in g["reconfig"]}
    return [k for k in range(len(g["names"])) if k not in moved]
