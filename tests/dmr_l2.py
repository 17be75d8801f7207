"""DMR layer 2 for the tests: an independent restatement of the 80-byte record of qrl_dmr_l2_decode (include/qrl_hip.h), written from the
air-interface rules (ETSI TS 102 361-1 annex B, the AMBE+2 FEC) and the reference's documented choices, not from csrc/dmr_l2_core.hpp; the
reference's own classes behind tests/host/dmr_l2_ref.cpp (load_ref, where the reference is present); and the builders of the scenario set
that tools/make_dmr_l2_golden.py records into tests/golden/ref/dmr_l2.npz.

Code tables are built here by rule: a syndrome decoder's table holds, for every syndrome, the first error pattern that reaches it when the
patterns are walked by ascending weight and, within a weight, by ascending lists of bit indices."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref", "dmr_l2.npz")
REFERENCE = "/root/reference"
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libqrl_ref.so")

FT_DATA, FT_VOICE, FT_VOICE_SYNC = 0, 1, 2
INFO_BITS = list(range(98)) + list(range(166, 264))          # the 196 code bits of a data burst
SLOT_BITS = list(range(98, 108)) + list(range(156, 166))     # Golay(20,8) of the slot type
EMB_BITS = list(range(108, 116)) + list(range(148, 156))     # QR(16,7,6) of the EMB
VOICE_BITS = list(range(108)) + list(range(156, 264))        # the three codec frames


# ------------------------------------------------------------------------------------------------------------------ bits
def to_bits(data):
    return np.unpackbits(np.frombuffer(bytes(bytearray(data)), np.uint8)).tolist()


def to_bytes(bits):
    return bytearray(np.packbits(np.array(bits, np.uint8)).tobytes())


def poly_rem(p, n, r, gen):
    for b in range(n - 1, r - 1, -1):
        if (p >> b) & 1:
            p ^= gen << (b - r)
    return p


_leader_cache = {}


def coset_leaders(n, r, gen, maxw):
    key = (n, r, gen, maxw)
    if key not in _leader_cache:
        syn1 = [poly_rem(1 << i, n, r, gen) for i in range(n)]
        tab = {0: 0}
        for w in range(1, maxw + 1):
            for comb in itertools.combinations(range(n), w):
                s = 0
                for i in comb:
                    s ^= syn1[i]
                if s not in tab:
                    tab[s] = sum(1 << i for i in comb)
        _leader_cache[key] = [tab.get(s, 0) for s in range(1 << r)]
    return _leader_cache[key]


def popc(v):
    return bin(v).count("1")


# ------------------------------------------------------------------------------------------------------------------ small codes
def slot_type(bits):
    """Golay(20,8): 19 bits through the syndrome decoder, the 20th (overall parity) ignored -> (colour code, data type)"""
    code = 0
    for p in SLOT_BITS[:19]:
        code = (code << 1) | bits[p]
    code ^= coset_leaders(19, 11, 0xC75, 5)[poly_rem(code, 19, 11, 0xC75)]
    return (code >> 15) & 15, (code >> 11) & 15


def emb(bits):
    """QR(16,7,6): 15 bits through the syndrome decoder -> (colour code, PI, LCSS)"""
    code = 0
    for p in EMB_BITS[:15]:
        code = (code << 1) | bits[p]
    code ^= coset_leaders(15, 8, 0x139, 4)[poly_rem(code, 15, 8, 0x139)]
    return (code >> 11) & 15, (code >> 10) & 1, (code >> 8) & 3


def crc_ccitt(data10):
    crc = 0
    for byte in data10:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021 if crc & 0x8000 else crc << 1) & 0xFFFF
    return crc ^ 0xFFFF


_gf = None


def _gf_tables():
    global _gf
    if _gf is None:
        exp, log, v = [0] * 512, [0] * 256, 1
        for i in range(255):
            exp[i] = exp[i + 255] = v
            log[v] = i
            v <<= 1
            if v & 0x100:
                v ^= 0x11D
        _gf = (exp, log)
    return _gf


def gf_mul(a, b):
    exp, log = _gf_tables()
    return exp[log[a] + log[b]] if a and b else 0


def rs129_parity(msg9):
    """remainder of msg(x) x^3 by (x + a)(x + a^2)(x + a^3) over GF(256): [x^0, x^1, x^2] coefficients"""
    exp, _ = _gf_tables()
    g = [1]
    for r in (1, 2, 3):
        g = [(g[k - 1] if k else 0) ^ (gf_mul(g[k], exp[r]) if k < len(g) else 0) for k in range(len(g) + 1)]
    par = [0, 0, 0]
    for byte in msg9:
        d = byte ^ par[2]
        par = [gf_mul(g[0], d), par[0] ^ gf_mul(g[1], d), par[1] ^ gf_mul(g[2], d)]
    return par


# ------------------------------------------------------------------------------------------------------------------ BPTC(196,96)
H15 = [(0, 1, 2, 3, 5, 7, 8), (1, 2, 3, 4, 6, 8, 9), (2, 3, 4, 5, 7, 9, 10), (0, 1, 2, 4, 6, 7, 10)]   # ETSI B.3.3 Hamming (15,11,3)
H13 = [(0, 1, 3, 5, 6), (0, 1, 2, 4, 6, 7), (0, 1, 2, 3, 5, 7, 8), (0, 2, 4, 5, 8)]                      # ETSI B.3.2 Hamming (13,9,3)


def _hamming_fix(word, eqs, k):
    """one syndrome decode of a k + 4 bit word (list); True when a bit was flipped"""
    syn = [(sum(word[j] for j in eq) + word[k + p]) & 1 for p, eq in enumerate(eqs)]
    if not any(syn):
        return False
    for j in range(k + 4):
        col = [int(j in eq) for eq in eqs] if j < k else [int(j - k == p) for p in range(4)]
        if col == syn:
            word[j] ^= 1
            return True
    return False


def bptc_decode(bits):
    raw = [bits[p] for p in INFO_BITS]
    m = [raw[(a * 181) % 196] for a in range(196)]
    for _ in range(5):
        fixing = False
        for c in range(15):
            col = [m[1 + c + 15 * a] for a in range(13)]
            if _hamming_fix(col, H13, 9):
                fixing = True
                for a in range(13):
                    m[1 + c + 15 * a] = col[a]
        for r in range(9):
            row = m[1 + 15 * r:16 + 15 * r]
            if _hamming_fix(row, H15, 11):
                fixing = True
                m[1 + 15 * r:16 + 15 * r] = row
        if not fixing:
            break
    data = m[4:12]
    for r in range(1, 9):
        data += m[1 + 15 * r:12 + 15 * r]
    return to_bytes(data)


def bptc_encode(payload, bits):
    d = to_bits(payload)
    m = [0] * 196
    m[4:12] = d[:8]
    for r in range(1, 9):
        m[1 + 15 * r:12 + 15 * r] = d[8 + 11 * (r - 1):19 + 11 * (r - 1)]
    for r in range(9):
        for p, eq in enumerate(H15):
            m[1 + 15 * r + 11 + p] = sum(m[1 + 15 * r + j] for j in eq) & 1
    for c in range(15):
        for p, eq in enumerate(H13):
            m[1 + c + 15 * (9 + p)] = sum(m[1 + c + 15 * a] for a in eq) & 1
    for a in range(196):
        bits[INFO_BITS[(a * 181) % 196]] = m[a]


# ------------------------------------------------------------------------------------------------------------------ rate 3/4 trellis
def _bitrev3(v):
    return ((v & 1) << 2) | (v & 2) | (v >> 2)


# state s, tribit t -> constellation point (ETSI B.2.4): the tribit advanced by 2 per low state bit and 4 per high state bit, bit-reversed,
# in the upper three bits; the lowest bit of the point separates the states {2,3,4,5} from {0,1,6,7}
STATE = [[(_bitrev3((t + 2 * (s & 1) + 4 * (s >> 2)) & 7) << 1) | (((s >> 1) ^ (s >> 2)) & 1) for t in range(8)] for s in range(8)]
INVERSE = [[STATE[s].index(p) if p in STATE[s] else None for p in range(16)] for s in range(8)]
# constellation point p3 p2 p1 p0 -> the four transmitted bits (two dibits): an affine map over GF(2)
POINT_BITS = [(((p ^ (p >> 2) ^ (p >> 3)) & 1) << 3) | ((((p >> 1) ^ (p >> 2) ^ (p >> 3)) & 1) << 2) | ((((p >> 3) & 1) ^ 1) << 1)
              | (((p >> 1) ^ (p >> 3)) & 1) for p in range(16)]
BITS_POINT = [POINT_BITS.index(n) for n in range(16)]
# the transmitted order of the 49 points: every fourth, from 0, 1, 2, 3
SCHEDULE = [q for r in range(4) for q in range(r, 49, 4)]


def trellis_points(bits):
    raw = [bits[p] for p in INFO_BITS]
    pts = [0] * 49
    for k in range(49):
        pts[SCHEDULE[k]] = BITS_POINT[(raw[4 * k] << 3) | (raw[4 * k + 1] << 2) | (raw[4 * k + 2] << 1) | raw[4 * k + 3]]
    return pts


def trellis_check(pts, tri, start=0):
    """first position whose point the state cannot send (tri[:start] is a valid prefix); 48 for a last tribit other than 0; 999 = passes"""
    state = tri[start - 1] if start else 0
    for i in range(start, 49):
        t = INVERSE[state][pts[i]]
        if t is None:
            return i
        tri[i] = t
        state = t
    return 48 if state else 999


def _payload_of(tri):
    v = 0    # tribit i lies in payload bits 141 - 3 i .. 143 - 3 i counted from the first bit, its high bit last
    for i in range(48):
        v |= _bitrev3(tri[i]) << (3 * i)
    return bytearray(v.to_bytes(18, "big"))


def trellis_decode(bits, stats=None):
    """-> payload (18 bytes) or None.  stats: fail_pos, rounds, goes, stuck (a round in which no candidate got past position 0)"""
    pts = trellis_points(bits)
    tri = [0] * 49
    first = trellis_check(pts, tri)
    st = {"fail_pos": first, "rounds": 0, "goes": 0, "stuck": False}
    if stats is not None:
        stats.update(st)
    if first == 999:
        return _payload_of(tri)
    for go, fail in ((1, first), (2, first - 1)):
        if fail < 0:
            break
        cur = list(pts)
        st["goes"] = go
        tri = [0] * 49
        for _ in range(20):
            st["rounds"] += 1
            best_pos, best_val = 0, 0
            trellis_check(cur, tri)      # the points before `fail` always pass: their tribits are the prefix every candidate shares
            for i in range(16):
                cur[fail] = i
                t2 = list(tri)
                pos = trellis_check(cur, t2, fail)
                if pos == 999:
                    if stats is not None:
                        stats.update(st)
                    return _payload_of(t2)
                if pos > best_pos:
                    best_pos, best_val = pos, i
            if best_pos == 0:
                st["stuck"] = True
            cur[fail] = best_val
            fail = best_pos
        if stats is not None:
            stats.update(st)
    return None


def trellis_encode(payload, bits):
    v = int.from_bytes(bytes(payload), "big")
    state, pts = 0, []
    for i in range(49):
        t = _bitrev3((v >> (3 * i)) & 7) if i < 48 else 0
        pts.append(STATE[state][t])
        state = t
    for k in range(49):
        n = POINT_BITS[pts[SCHEDULE[k]]]
        for j in range(4):
            bits[INFO_BITS[4 * k + j]] = (n >> (3 - j)) & 1


# ------------------------------------------------------------------------------------------------------------------ voice
def golay23_word(data):
    return (data << 11) | poly_rem(data << 11, 23, 11, 0xC75)


def golay24_word(data):
    w = golay23_word(data)
    return (w << 1) | (popc(w) & 1)


def ambe_prng(seed):
    pr, out = 16 * seed, 0
    for _ in range(23):
        pr = (173 * pr + 13849) & 0xFFFF
        out = (out << 1) | (pr >> 15)
    return out


def ambe_positions(frame):
    """bit positions of the A (24), B (23) and C (25) words of codec frame 0..2 of a voice burst"""
    pos = [4 * (j % 18) + j // 18 for j in range(72)]
    if frame == 1:
        pos = [p + 72 + (48 if p + 72 >= 108 else 0) for p in pos]
    if frame == 2:
        pos = [p + 192 for p in pos]
    return pos[:24], pos[24:47], pos[47:]


SILENCE = (0xF00292, 0x0E0B20, 0)   # the A, B and C words of the codec's silence frame (AMBE+2: B9 E8 81 52 61 73 00 2A 6B)


def ambe_regenerate(bits, paths=None):
    """CAMBEFEC::regenerateDMR on the bit list; paths collects 'a_bad', 'rule_a4', 'rule_ab6' as they occur"""
    g23 = coset_leaders(23, 11, 0xC75, 3)
    total = 0
    for f in range(3):
        pa, pb, pc = ambe_positions(f)
        a = int("".join(str(bits[p]) for p in pa), 2)
        b = int("".join(str(bits[p]) for p in pb), 2)
        c = int("".join(str(bits[p]) for p in pc), 2)
        syn = poly_rem(a >> 1, 23, 11, 0xC75)
        out = a ^ (g23[syn] << 1)
        if not (popc(syn) < 3 or popc(out) % 2 == 0):
            a2, b2, c2 = SILENCE
            total += 10
            if paths is not None:
                paths.add("a_bad")
        else:
            data = out >> 12
            a2 = golay24_word(data)
            p = ambe_prng(data)
            w = b ^ p
            w ^= g23[poly_rem(w, 23, 11, 0xC75)]
            b2 = golay23_word(w >> 11) ^ p
            c2 = c
            ea, eb = popc(a2 ^ a), popc(b2 ^ b)
            total += ea + eb
            if ea >= 4 or (ea + eb >= 6 and ea >= 2):
                if paths is not None:
                    paths.add("rule_a4" if ea >= 4 else "rule_ab6")
                a2, b2, c2 = SILENCE
        for word, width, where in ((a2, 24, pa), (b2, 23, pb), (c2, 25, pc)):
            for j, p in enumerate(where):
                bits[p] = (word >> (width - 1 - j)) & 1
    return total


# ------------------------------------------------------------------------------------------------------------------ the record
def _id(d, i):
    return (d[i] << 16) | (d[i + 1] << 8) | d[i + 2]


def record(rec_in, audio_fec, info=None):
    """the 80-byte record of one 40-byte mailbox record; info (a dict) receives the trellis statistics / voice paths"""
    rec_in = bytearray(rec_in)
    out = bytearray(80)
    ftype = rec_in[0]
    out[0], out[1] = rec_in[0], rec_in[1]
    bits = to_bits(rec_in[4:37])
    if ftype in (FT_VOICE, FT_VOICE_SYNC):
        out[3] = 0xF1 if ftype == FT_VOICE else 0xF0
        out[4] = 1
        if audio_fec:
            paths = set()
            out[5] = ambe_regenerate(bits, paths)
            if info is not None:
                info["paths"] = paths
        if ftype == FT_VOICE:
            out[2], out[6], out[7] = emb(bits)
        else:
            out[2] = rec_in[2]
        burst = to_bytes(bits)
        out[20:53] = burst
        out[8] = 27
        voice = burst[:14] + burst[20:33]
        voice[13] = (burst[13] & 0xF0) | (burst[19] & 0x0F)
        out[53:80] = voice
        return out
    if ftype != FT_DATA:
        out[2], out[3], out[4] = 255, 9, 1
        out[20:53] = rec_in[4:37]
        return out
    cc, dt = slot_type(bits)
    out[2], out[3] = cc, dt
    out[20:53] = rec_in[4:37]
    if dt > 8:
        return out
    if dt == 8:
        stats = {}
        payload = trellis_decode(bits, stats)
        if info is not None:
            info.update(stats)
        if payload is None:
            return out
        trellis_encode(payload, bits)
        out[4], out[8] = 1, 18
        out[20:53] = to_bytes(bits)
        out[53:71] = payload
        return out
    d = bptc_decode(bits)
    kept = bytearray(d)
    src = dst = flco = fid = 0
    if dt in (1, 2):
        mask = 0x96 if dt == 1 else 0x99
        par = rs129_parity(d[:9])
        if [d[9] ^ mask, d[10] ^ mask, d[11] ^ mask] != [par[2], par[1], par[0]]:
            return out
        flco, fid, dst, src = d[0] & 0x3F, d[1], _id(d, 3), _id(d, 6)
    elif dt in (3, 4, 5):
        # the reference checks CSBK, MBC header and MBC continuation alike under the CSBK mask
        crc = crc_ccitt(d[:10]) ^ 0xA5A5
        if (d[10] << 8) | d[11] != crc:
            return out
        flco, fid = d[0] & 0x3F, d[1]
        first, second = _id(d, 4), _id(d, 7)
        dst, src = first, second
        if flco == 0x38:
            dst = 0
        elif flco == 0x26 or (flco == 0x24 and d[3] != 0x80):
            src, dst = first, second
    elif dt == 6:
        crc = crc_ccitt(d[:10]) ^ 0xCCCC
        if (d[10] << 8) | d[11] != crc:
            return out
        dpf = d[0] & 0x0F
        if dpf != 0x0F:
            dst, src = _id(d, 2), _id(d, 5)
            if dpf == 0:
                flco = d[9] & 0x3F
                d[9] &= 0xFE
                crc = crc_ccitt(d[:10]) ^ 0xCCCC
                d[10], d[11] = crc >> 8, crc & 0xFF
    bptc_encode(d, bits)
    out[4], out[8], out[9], out[10] = 1, 12, flco, fid
    out[12:16] = src.to_bytes(4, "little")
    out[16:20] = dst.to_bytes(4, "little")
    out[20:53] = to_bytes(bits)
    out[53:65] = kept
    return out


def records(inputs, audio_fec):
    """[n, 40] uint8, [n] flags -> [n, 80] uint8"""
    inputs = np.asarray(inputs, np.uint8)
    audio_fec = np.broadcast_to(np.asarray(audio_fec), (inputs.shape[0],))
    return np.array([record(inputs[i].tobytes(), int(audio_fec[i])) for i in range(inputs.shape[0])], np.uint8).reshape(-1, 80)


def mailbox(inputs, counts, audio_fec):
    """[batch, cap, 40] mailbox, counts [batch] or None -> [batch, cap, 80]: slots at or past min(count, cap) are zero"""
    inputs = np.asarray(inputs, np.uint8)
    batch, cap = inputs.shape[:2]
    out = np.zeros((batch, cap, 80), np.uint8)
    for b in range(batch):
        n = cap if counts is None else min(int(counts[b]), cap)
        if n:
            out[b, :n] = records(inputs[b, :n], audio_fec)
    return out


# ------------------------------------------------------------------------------------------------------------------ transmit side
def emb_word(cc, pi, lcss):
    """the 16 EMB bits: QR(16,7,6) of colour code, PI and LCSS"""
    data = ((cc & 15) << 3) | ((pi & 1) << 2) | (lcss & 3)
    w = (data << 8) | poly_rem(data << 8, 15, 8, 0x139)
    w = (w << 1) | (popc(w) & 1)
    return [(w >> (15 - i)) & 1 for i in range(16)]


def lc_block(flco, fid, options, dst, src, data_type):
    """the 12 bytes of a voice LC header (data type 1) / terminator with LC (2): nine LC bytes + masked RS(12,9) parity"""
    d = bytearray([flco & 0x3F, fid, options]) + dst.to_bytes(3, "big") + src.to_bytes(3, "big")
    par, mask = rs129_parity(d), 0x96 if data_type == 1 else 0x99
    return d + bytearray([par[2] ^ mask, par[1] ^ mask, par[0] ^ mask])


def crc_block(d10, mask):
    """ten bytes + their masked CRC-CCITT (0xA5A5 CSBK, 0xCCCC data header)"""
    crc = crc_ccitt(d10) ^ mask
    return bytearray(d10) + bytearray([crc >> 8, crc & 0xFF])


def info_bits_bptc(block12):
    bits = [0] * 264
    bptc_encode(block12, bits)
    return [bits[p] for p in INFO_BITS]


def info_bits_rate34(payload18):
    bits = [0] * 264
    trellis_encode(payload18, bits)
    return [bits[p] for p in INFO_BITS]


def voice_bits(rng, middle48):
    """264 bits of a voice burst: three codec frames of valid A / B code words around the 48 middle bits given"""
    bits = [int(v) for v in rng.integers(0, 2, 264)]
    for f in range(3):
        pa, pb, _ = ambe_positions(f)
        data = int(rng.integers(4096))
        a, b = golay24_word(data), golay23_word(int(rng.integers(4096))) ^ ambe_prng(data)
        for j, p in enumerate(pa):
            bits[p] = (a >> (23 - j)) & 1
        for j, p in enumerate(pb):
            bits[p] = (b >> (22 - j)) & 1
    bits[108:156] = middle48
    return bits


# ------------------------------------------------------------------------------------------------------------------ the reference
class Ref:
    def __init__(self, lib):
        self.lib = lib
        u8p = C.POINTER(C.c_uint8)
        lib.ref_dmr_l2_record.argtypes = [u8p, C.c_int, u8p]
        for name in ("ref_trellis_encode", "ref_bptc_encode", "ref_bptc_decode"):
            getattr(lib, name).argtypes = [u8p, u8p]
        lib.ref_trellis_decode.argtypes = [u8p, u8p]
        lib.ref_fulllc_encode.argtypes = [u8p, C.c_int, u8p]
        lib.ref_csbk_build.argtypes = [C.c_int] * 6 + [C.c_uint32, C.c_uint32, C.c_int, u8p]
        lib.ref_dataheader_build.argtypes = [u8p, u8p]
        lib.ref_slottype_set.argtypes = [C.c_int, C.c_int, u8p]
        lib.ref_emb_set.argtypes = [C.c_int, C.c_int, C.c_int, u8p]
        for name in ("ref_golay24128_encode", "ref_golay23127_encode", "ref_golay23127_decode"):
            getattr(lib, name).argtypes = [C.c_uint32]
            getattr(lib, name).restype = C.c_uint32
        lib.ref_golay24128_decode.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        for name in ("ref_golay2087_decode", "ref_qr1676_decode", "ref_rs129_check", "ref_crc_ccitt162_check"):
            getattr(lib, name).argtypes = [u8p]
        lib.ref_ambe_regenerate.argtypes = [u8p]
        lib.ref_ambe_regenerate.restype = C.c_uint

    @staticmethod
    def buf(data):
        return (C.c_uint8 * len(data)).from_buffer(data)

    def record(self, rec_in, audio_fec):
        src, out = bytearray(rec_in), bytearray(80)
        self.lib.ref_dmr_l2_record(self.buf(src), int(audio_fec), self.buf(out))
        return out

    def records(self, inputs, audio_fec):
        inputs = np.asarray(inputs, np.uint8)
        audio_fec = np.broadcast_to(np.asarray(audio_fec), (inputs.shape[0],))
        return np.array([self.record(inputs[i].tobytes(), int(audio_fec[i])) for i in range(inputs.shape[0])], np.uint8).reshape(-1, 80)

    def const(self, which):
        return self.lib.ref_dmr_const(which)

    def into(self, name, burst, *args):
        """call an encoder that writes into a 33-byte burst (a bytearray, changed in place)"""
        getattr(self.lib, name)(*args, self.buf(burst))


def load_ref(build_dir):
    """the reference's classes behind tests/host/dmr_l2_ref.cpp, compiled into build_dir; None where the reference is absent"""
    if not (os.path.isdir(os.path.join(REFERENCE, "src", "MMDVM")) and os.path.isfile(REF_LIB)):
        return None
    so = os.path.join(str(build_dir), "libdmr_l2_ref.so")
    subprocess.check_call(["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "dmr_l2_ref.cpp"),
                           "-I" + REFERENCE, "-I" + os.path.join(REFERENCE, "src", "MMDVM"), "-I" + os.path.join(ROOT, "oracle", "gr_stub"), "-o", so,
                           "-L" + os.path.dirname(REF_LIB), "-lqrl_ref", "-Wl,-rpath," + os.path.dirname(REF_LIB)])
    return Ref(C.CDLL(so))


# ------------------------------------------------------------------------------------------------------------------ the scenario set
SEED = 20241
FLIP_LEVELS = (0, 2, 4, 8, 12)
# an opcode for every branch of CDMRCSBK::put (the last two take the default branch), and for radio check both values of byte 3
CSBK_CASES = [(0x38, 0), (0x04, 0), (0x05, 0), (0x3D, 0x11), (0x26, 0), (0x1F, 0x23), (0x2A, 0x07), (0x20, 0x01), (0x21, 0x02), (0x24, 0x80),
              (0x24, 0x00), (0x07, 0x55), (0x1C, 0x0F)]
DPF_CASES = [0x0, 0x1, 0x2, 0x3, 0xD, 0xE, 0xF, 0x5]


def flip(burst, positions, count, rng):
    for p in rng.choice(len(positions), count, replace=False):
        burst[positions[p] >> 3] ^= 0x80 >> (positions[p] & 7)


def _rec(ftype, fn, cc, burst):
    return bytes([ftype, fn, cc, 0]) + bytes(burst) + bytes(3)


def data_burst(ref, rng, dt, cc, variant):
    """a properly encoded burst of data type dt (9..15: random code bits), slot type and data sync included"""
    burst = bytearray(rng.randint(0, 256, 33).astype(np.uint8).tobytes())
    if dt in (0, 7):
        ref.into("ref_bptc_encode", burst, ref.buf(bytearray(rng.randint(0, 256, 12).astype(np.uint8).tobytes())))
    elif dt in (1, 2):
        ref.into("ref_fulllc_encode", burst, ref.buf(bytearray(rng.randint(0, 256, 9).astype(np.uint8).tobytes())), dt)
    elif dt in (3, 4, 5):
        op, cbf = CSBK_CASES[variant % len(CSBK_CASES)]
        # every third MBC burst carries the CRC of its own type, which the reference's check (CSBK mask) refuses
        own = dt if (dt != 3 and variant % 3 == 2) else 3
        ref.into("ref_csbk_build", burst, op, int(rng.randint(2)), int(rng.randint(2)), int(rng.randint(256)), int(rng.randint(256)), cbf,
                 int(rng.randint(1 << 24)), int(rng.randint(1 << 24)), own)
    elif dt == 6:
        d = bytearray(rng.randint(0, 256, 10).astype(np.uint8).tobytes())
        d[0] = (d[0] & 0xF0) | DPF_CASES[variant % len(DPF_CASES)]
        ref.into("ref_dataheader_build", burst, ref.buf(d))
    elif dt == 8:
        ref.into("ref_trellis_encode", burst, ref.buf(bytearray(rng.randint(0, 256, 18).astype(np.uint8).tobytes())))
    ref.into("ref_slottype_set", burst, cc, dt)
    return burst


def voice_burst(ref, rng, cc, pi, lcss):
    burst = bytearray(rng.randint(0, 256, 33).astype(np.uint8).tobytes())
    bits = to_bits(burst)
    for f in range(3):
        pa, pb, pc = ambe_positions(f)
        data = int(rng.randint(4096))
        a = ref.lib.ref_golay24128_encode(data)
        b = (ref.lib.ref_golay23127_encode(int(rng.randint(4096))) >> 1) ^ ambe_prng(data)
        for j, p in enumerate(pa):
            bits[p] = (a >> (23 - j)) & 1
        for j, p in enumerate(pb):
            bits[p] = (b >> (22 - j)) & 1
    burst = to_bytes(bits)
    ref.into("ref_emb_set", burst, cc, pi, lcss)
    return burst


def build_scenarios(ref, seed=SEED):
    """-> inputs [n, 40] uint8, audio_fec [n] uint8, group [n] uint8 (0 data types, 1 rate 3/4, 2 voice)"""
    rng = np.random.RandomState(seed)
    recs, af, group = [], [], []
    k = 0
    for variant in range(4):
        for dt in range(16):
            for cc in range(8):
                for level in FLIP_LEVELS:
                    burst = data_burst(ref, rng, dt, 2 * cc + (variant & 1), k)
                    flip(burst, INFO_BITS, level, rng)
                    flip(burst, SLOT_BITS, k % 4, rng)
                    recs.append(_rec(FT_DATA, 0, 0, burst)); af.append(k & 1); group.append(0)
                    k += 1
    # rate 3/4: clean, lightly damaged, garbage
    for level, count in ((0, 16), (1, 48), (2, 32), (3, 32), (4, 32), (40, 16)):
        for _ in range(count):
            burst = data_burst(ref, rng, 8, int(rng.randint(16)), 0)
            flip(burst, INFO_BITS, level, rng)
            recs.append(_rec(FT_DATA, 0, 0, burst)); af.append(1); group.append(1)
    for _ in range(96):
        burst = bytearray(rng.randint(0, 256, 33).astype(np.uint8).tobytes())
        ref.into("ref_slottype_set", burst, int(rng.randint(16)), 8)
        recs.append(_rec(FT_DATA, 0, 0, burst)); af.append(1); group.append(1)
    for first_point in range(16):       # a failing position of 0: the first point replaced by each of the 16
        burst = data_burst(ref, rng, 8, 1, 0)
        bits = to_bits(burst)
        for j in range(4):
            bits[j] = (POINT_BITS[first_point] >> (3 - j)) & 1
        recs.append(_rec(FT_DATA, 0, 0, to_bytes(bits))); af.append(1); group.append(1)
    # voice A..F: random flips over the codec frames, flips aimed at one frame's A and B words, EMB flips
    for level in (0, 1, 2, 3, 4, 6, 8, 10, 12, 16):
        for fn in range(6):
            for rep in range(6):
                cc, pi, lcss = int(rng.randint(16)), int(rng.randint(2)), int(rng.randint(4))
                burst = voice_burst(ref, rng, cc, pi, lcss)
                flip(burst, VOICE_BITS, level, rng)
                if fn:
                    flip(burst, EMB_BITS, rep % 4, rng)
                recs.append(_rec(FT_VOICE if fn else FT_VOICE_SYNC, fn, cc, burst)); af.append(0 if rep == 5 else 1); group.append(2)
    for na, nb in ((2, 4), (3, 3), (2, 5), (3, 4), (4, 0), (4, 1), (5, 0), (5, 2), (6, 0), (7, 1)):
        for rep in range(8):
            burst = voice_burst(ref, rng, 3, 0, 1)
            pa, pb, _ = ambe_positions(rep % 3)
            flip(burst, pa, na, rng)
            flip(burst, pb, nb, rng)
            recs.append(_rec(FT_VOICE, 1 + rep % 5, 3, burst)); af.append(1); group.append(2)
    return (np.frombuffer(b"".join(recs), np.uint8).reshape(-1, 40).copy(), np.array(af, np.uint8), np.array(group, np.uint8))


def load_golden():
    g = np.load(GOLDEN)
    return g["inputs"], g["audio_fec"], g["group"], g["records"]
