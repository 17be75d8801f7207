// dmr_l2_core.hpp — the stateless per-burst work of DMR layer 2, free of HIP: what the reference does to every burst its DMO sink returns
// (DMRFrame::DMRFrame / validate / runAudioFEC, reference src/DMR/dmrframe.cpp:36-253, and CDMREMB::putData, src/DMR/dmrcontrol.cpp:247).
//   slot type      Golay(20,8)                                   src/MMDVM/DMRSlotType.cpp:36-54, Golay2087.cpp:238-250
//   BPTC(196,96)   Hamming (13,9,3) columns / (15,11,3) rows     src/MMDVM/BPTC19696.cpp:44-347
//   full LC        RS(12,9) under the header / terminator mask   src/MMDVM/DMRFullLC.cpp:39-99, RS129.cpp:102-129
//   CSBK / MBC     CRC-CCITT under the CSBK mask, IDs by opcode  src/MMDVM/DMRCSBK.cpp:95-263
//   data header    CRC-CCITT under the header mask, IDs by DPF   src/MMDVM/DMRDataHeader.cpp:64-170
//   rate 3/4       trellis check, the two-go point search        src/MMDVM/DMRTrellis.cpp:50-374
//   voice          Golay(24,12) / (23,12) under the AMBE PRNG    src/MMDVM/AMBEFEC.cpp:476-575, :828-868, Golay24128.cpp:1083-1105
//   EMB            QR(16,7,6)                                    src/MMDVM/DMREMB.cpp:37-52, QR1676.cpp:104-115
// Plain inline functions behind a host / device macro: kernels_dmr_l2.hip calls them one lane per burst, tests/host/test_dmr_l2_core.cpp
// runs them on the CPU under the sanitizers.  Every table is made by rule at compile time (make_dmr_tables); tests/test_dmr_l2.py pins
// them against the reference's compiled classes.  Where the reference's result is a quirk (a CSBK mask on an MBC burst, bit 0 of byte 9
// of a UDT header, the reversed RS parity bytes) the quirk is reproduced, not corrected.
#pragma once
#include <cstdint>
#include <cstddef>

#if defined(__HIPCC__)
#define QRL_HD __host__ __device__
#define QRL_DMR_TABLE static __constant__
#else
#define QRL_HD
#define QRL_DMR_TABLE static constexpr
#endif

namespace qrl {
namespace dmr {

enum { REC_IN = 40, REC_OUT = 80, BURST = 33 };
enum { FT_DATA = 0, FT_VOICE = 1, FT_VOICE_SYNC = 2 };
// DMRFrame::getDataType(): the slot type's low nibble, or the class's two stand-in values for voice bursts
enum { DT_VOICE_PI_HEADER = 0, DT_VOICE_LC_HEADER = 1, DT_TERMINATOR_WITH_LC = 2, DT_CSBK = 3, DT_MBC_HEADER = 4, DT_MBC_CONTINUATION = 5,
       DT_DATA_HEADER = 6, DT_RATE_12_DATA = 7, DT_RATE_34_DATA = 8, DT_IDLE = 9, DT_VOICE_SYNC = 0xF0, DT_VOICE = 0xF1 };
// offsets into the 80-byte record
enum { R_FTYPE = 0, R_FN = 1, R_CC = 2, R_DTYPE = 3, R_VALID = 4, R_ERRS = 5, R_PI = 6, R_LCSS = 7, R_PLEN = 8, R_FLCO = 9, R_FID = 10,
       R_SRC = 12, R_DST = 16, R_BURST = 20, R_PAYLOAD = 53 };
enum { TRELLIS_OK = 999 };

// remainder of the polynomial p (top bit `top`) by the generator gen of degree r
QRL_HD constexpr uint32_t poly_rem(uint32_t p, int top, int r, uint32_t gen)
{
    for (int b = top; b >= r; --b) if ((p >> b) & 1u) p ^= gen << (b - r);
    return p;
}
QRL_HD constexpr unsigned popc32(uint32_t v) { unsigned c = 0; for (; v; v &= v - 1) ++c; return c; }

// ---- tables by rule ----
// Syndrome decoding tables hold the coset leader the classic table-building program finds: error patterns by ascending weight, within a
// weight by ascending lists of bit indices, the first pattern of a syndrome stays.  g2087 / qr keep only the bits the decoders return.
struct Tables {
    uint8_t g2087[2048];   // Golay(19,8) syndrome -> error pattern >> 11
    uint32_t g23[2048];    // Golay(23,12) syndrome -> error pattern
    uint8_t qr[256];       // QR(15,7) syndrome -> error pattern >> 7
    uint8_t gf_exp[512], gf_log[256], rs_poly[3];   // GF(256) / x^8+x^4+x^3+x^2+1; (x+a)(x+a^2)(x+a^3)
    uint8_t tr_seq[49];    // trellis interleave schedule: transmitted dibit pair k carries constellation point tr_seq[k]
    uint8_t con_point[16]; // four transmitted bits -> constellation point
    uint8_t con_bits[16];  // and back
};

template <int N, int R, int MAXW, typename T, int SHIFT>
constexpr void fill_coset_leaders(T* tab, uint32_t gen)
{
    bool have[1 << R] = {};
    uint32_t s1[N] = {};
    for (int i = 0; i < N; ++i) s1[i] = poly_rem((uint32_t)1 << i, N - 1, R, gen);
    have[0] = true; tab[0] = 0;
    auto put = [&](uint32_t syn, uint32_t pat) { if (!have[syn]) { have[syn] = true; tab[syn] = (T)(pat >> SHIFT); } };
    for (int w = 1; w <= MAXW; ++w)
        for (int a = 0; a < N; ++a) {
            const uint32_t sa = s1[a], pa = (uint32_t)1 << a;
            if (w == 1) { put(sa, pa); continue; }
            for (int b = a + 1; b < N; ++b) {
                const uint32_t sb = sa ^ s1[b], pb = pa | ((uint32_t)1 << b);
                if (w == 2) { put(sb, pb); continue; }
                for (int c = b + 1; c < N; ++c) {
                    const uint32_t sc = sb ^ s1[c], pc = pb | ((uint32_t)1 << c);
                    if (w == 3) { put(sc, pc); continue; }
                    for (int d = c + 1; d < N; ++d) {
                        const uint32_t sd = sc ^ s1[d], pd = pc | ((uint32_t)1 << d);
                        if (w == 4) { put(sd, pd); continue; }
                        for (int e = d + 1; e < N; ++e) put(sd ^ s1[e], pd | ((uint32_t)1 << e));
                    }
                }
            }
        }
}

constexpr Tables make_dmr_tables()
{
    Tables t{};
    fill_coset_leaders<19, 11, 5, uint8_t, 11>(t.g2087, 0xC75);
    fill_coset_leaders<23, 11, 3, uint32_t, 0>(t.g23, 0xC75);
    fill_coset_leaders<15, 8, 4, uint8_t, 7>(t.qr, 0x139);
    unsigned v = 1;
    for (int i = 0; i < 255; ++i) {
        t.gf_exp[i] = (uint8_t)v; t.gf_exp[i + 255] = (uint8_t)v; t.gf_log[v] = (uint8_t)i;
        v <<= 1;
        if (v & 0x100u) v ^= 0x11Du;
    }
    t.gf_exp[510] = 1; t.gf_exp[511] = 0;
    // (x + a)(x + a^2)(x + a^3), coefficients of x^0 .. x^2
    unsigned g[4] = {1, 0, 0, 0};
    for (int r = 1; r <= 3; ++r) {
        const unsigned root = t.gf_exp[r];
        for (int k = r; k >= 0; --k) {
            const unsigned lo = g[k] ? t.gf_exp[t.gf_log[g[k]] + t.gf_log[root]] : 0u;
            g[k] = (k ? g[k - 1] : 0u) ^ lo;
        }
    }
    for (int k = 0; k < 3; ++k) t.rs_poly[k] = (uint8_t)g[k];
    int k = 0;
    for (int r = 0; r < 4; ++r) for (int q = r; q < 49; q += 4) t.tr_seq[k++] = (uint8_t)q;
    // constellation: the four bits of the two dibits are an affine map of the point number over GF(2)
    for (unsigned p = 0; p < 16; ++p) {
        const unsigned p0 = p & 1u, p1 = (p >> 1) & 1u, p2 = (p >> 2) & 1u, p3 = (p >> 3) & 1u;
        const unsigned n = ((p0 ^ p2 ^ p3) << 3) | ((p1 ^ p2 ^ p3) << 2) | ((p3 ^ 1u) << 1) | (p1 ^ p3);
        t.con_bits[p] = (uint8_t)n; t.con_point[n] = (uint8_t)p;
    }
    return t;
}
QRL_DMR_TABLE Tables c_dmr = make_dmr_tables();

// ---- bits of a burst, MSB first ----
QRL_HD inline unsigned rd_bit(const uint8_t* p, unsigned i) { return (p[i >> 3] >> (7u - (i & 7u))) & 1u; }
QRL_HD inline void wr_bit(uint8_t* p, unsigned i, unsigned b)
{
    const uint8_t m = (uint8_t)(0x80u >> (i & 7u));
    p[i >> 3] = b ? (uint8_t)(p[i >> 3] | m) : (uint8_t)(p[i >> 3] & ~m);
}

// ---- Golay(20,8) of the slot type, QR(16,7,6) of the EMB ----
QRL_HD inline unsigned slot_type_decode(const uint8_t* d)   // colour code << 4 | data type
{
    const unsigned s0 = ((d[12] << 2) & 0xFCu) | ((d[13] >> 6) & 0x03u);
    const unsigned s1 = ((d[13] << 2) & 0xC0u) | ((d[19] << 2) & 0x3Cu) | ((d[20] >> 6) & 0x03u);
    const unsigned s2 = (d[20] << 2) & 0xF0u;
    const uint32_t code = (s0 << 11) + (s1 << 3) + (s2 >> 5);
    return ((code >> 11) ^ c_dmr.g2087[poly_rem(code, 18, 11, 0xC75)]) & 0xFFu;
}
QRL_HD inline unsigned emb_decode(const uint8_t* d)   // colour code << 4 | PI << 3 | LCSS << 1 | first parity bit
{
    const unsigned e0 = ((d[13] << 4) & 0xF0u) | ((d[14] >> 4) & 0x0Fu);
    const unsigned e1 = ((d[18] << 4) & 0xF0u) | ((d[19] >> 4) & 0x0Fu);
    const uint32_t code = (e0 << 7) + (e1 >> 1);
    return ((code >> 7) ^ c_dmr.qr[poly_rem(code, 14, 8, 0x139)]) & 0xFFu;
}

// ---- CRC-CCITT (x^16 + x^12 + x^5 + 1, zero start, inverted, high byte first) over bytes 0..9 of a 12-byte block ----
QRL_HD inline unsigned crc_ccitt10(const uint8_t* in)
{
    unsigned crc = 0;
    for (int i = 0; i < 10; ++i) {
        crc ^= (unsigned)in[i] << 8;
        for (int b = 0; b < 8; ++b) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
    }
    return ~crc & 0xFFFFu;
}

// ---- RS(12,9): parity[0..2] of CRS129::encode over nine bytes ----
QRL_HD inline unsigned gf_mul(unsigned a, unsigned b) { return (a && b) ? c_dmr.gf_exp[c_dmr.gf_log[a] + c_dmr.gf_log[b]] : 0u; }
QRL_HD inline void rs129_parity(const uint8_t* msg, uint8_t* parity)
{
    unsigned p0 = 0, p1 = 0, p2 = 0;
    for (int i = 0; i < 9; ++i) {
        const unsigned d = msg[i] ^ p2;
        p2 = p1 ^ gf_mul(c_dmr.rs_poly[2], d);
        p1 = p0 ^ gf_mul(c_dmr.rs_poly[1], d);
        p0 = gf_mul(c_dmr.rs_poly[0], d);
    }
    parity[0] = (uint8_t)p0; parity[1] = (uint8_t)p1; parity[2] = (uint8_t)p2;
}
QRL_HD inline bool rs129_check(const uint8_t* in)
{
    uint8_t p[3];
    rs129_parity(in, p);
    return in[9] == p[2] && in[10] == p[1] && in[11] == p[0];   // the reference keeps the parity bytes in reversed order
}

// ---- BPTC(196,96): the 13 x 15 matrix as 13 words, row r = matrix bits 1 + 15 r .. 15 + 15 r ----
// parity equations over the data bits (ETSI TS 102 361-1 B.3): bit j of mask p set = data bit j enters parity p
QRL_HD constexpr unsigned h15_mask(int p) { return p == 0 ? 0x01AFu : p == 1 ? 0x035Eu : p == 2 ? 0x06BCu : 0x04D7u; }
QRL_HD constexpr unsigned h13_mask(int p) { return p == 0 ? 0x006Bu : p == 1 ? 0x00D7u : p == 2 ? 0x01AFu : 0x0135u; }
// transmitted bit i (0 .. 195) of a burst: bits 0..97, then the low two bits of byte 20, then bytes 21..32
QRL_HD inline unsigned code_bit_pos(unsigned i) { return i < 98u ? i : i + 68u; }

QRL_HD inline void bptc_decode(const uint8_t* in, uint8_t* out)
{
    unsigned row[13];
    for (int r = 0; r < 13; ++r) {
        unsigned w = 0;
        for (int j = 0; j < 15; ++j) w |= rd_bit(in, code_bit_pos(((1u + 15u * r + j) * 181u) % 196u)) << j;
        row[r] = w;
    }
    bool fixing = false;
    int count = 0;
    do {
        fixing = false;
        // columns, Hamming (13,9,3), all 15 at once: plane p = the p-th syndrome bit of every column
        unsigned s[4];
        for (int p = 0; p < 4; ++p) {
            unsigned v = row[9 + p];
            for (int a = 0; a < 9; ++a) if ((h13_mask(p) >> a) & 1u) v ^= row[a];
            s[p] = v;
        }
        for (int a = 0; a < 13; ++a) {
            unsigned m = 0x7FFFu;
            for (int p = 0; p < 4; ++p) {
                const unsigned bit = a < 9 ? (h13_mask(p) >> a) & 1u : (unsigned)(a - 9 == p);
                m &= bit ? s[p] : ~s[p];
            }
            row[a] ^= m;
            fixing |= m != 0;
        }
        // the nine rows that carry data, Hamming (15,11,3): flip the one bit whose column of the check matrix equals the syndrome
        for (int r = 0; r < 9; ++r) {
            unsigned syn = 0;
            for (int p = 0; p < 4; ++p) syn |= ((popc32(row[r] & h15_mask(p)) ^ (row[r] >> (11 + p))) & 1u) << p;
            if (!syn) continue;
            for (int j = 0; j < 15; ++j) {
                unsigned col = 0;
                if (j < 11) for (int p = 0; p < 4; ++p) col |= ((h15_mask(p) >> j) & 1u) << p;
                else col = 1u << (j - 11);
                if (col == syn) { row[r] ^= 1u << j; fixing = true; break; }
            }
        }
        ++count;
    } while (fixing && count < 5);
    // payload: row 0 bits 3..10, rows 1..8 bits 0..10, MSB first
    for (int i = 0; i < 12; ++i) out[i] = 0;
    unsigned pos = 0;
    for (int j = 3; j <= 10; ++j, ++pos) if ((row[0] >> j) & 1u) out[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7u));
    for (int r = 1; r <= 8; ++r)
        for (int j = 0; j <= 10; ++j, ++pos) if ((row[r] >> j) & 1u) out[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7u));
}

QRL_HD inline void bptc_encode(const uint8_t* in, uint8_t* burst)   // the burst's other bits are kept
{
    unsigned row[13];
    unsigned pos = 0;
    {
        unsigned w = 0;
        for (int j = 3; j <= 10; ++j, ++pos) w |= rd_bit(in, pos) << j;
        row[0] = w;
    }
    for (int r = 1; r <= 8; ++r) { unsigned w = 0; for (int j = 0; j <= 10; ++j, ++pos) w |= rd_bit(in, pos) << j; row[r] = w; }
    for (int r = 0; r < 9; ++r)
        for (int p = 0; p < 4; ++p) row[r] |= (popc32(row[r] & h15_mask(p)) & 1u) << (11 + p);
    for (int p = 0; p < 4; ++p) {
        unsigned v = 0;
        for (int a = 0; a < 9; ++a) if ((h13_mask(p) >> a) & 1u) v ^= row[a];
        row[9 + p] = v;
    }
    wr_bit(burst, code_bit_pos(0), 0);   // matrix bit 0 = R(3), unused
    for (unsigned a = 1; a < 196u; ++a) wr_bit(burst, code_bit_pos((a * 181u) % 196u), (row[(a - 1) / 15] >> ((a - 1) % 15)) & 1u);
}

// ---- rate 3/4 trellis.  49 constellation points / tribits as nibbles of four 64-bit words ----
struct Nib49 { uint64_t w[4]; };
QRL_HD inline unsigned nib_get(const Nib49& n, unsigned i) { return (unsigned)(n.w[i >> 4] >> ((i & 15u) * 4u)) & 15u; }
QRL_HD inline void nib_set(Nib49& n, unsigned i, unsigned v)
{
    const unsigned sh = (i & 15u) * 4u;
    n.w[i >> 4] = (n.w[i >> 4] & ~((uint64_t)15 << sh)) | ((uint64_t)v << sh);
}
// State table by rule: from state s, tribit t sends point bitrev4((t + 2 (s & 1) + 4 (s >> 2)) mod 8) | (bit 1 of s ^ bit 2 of s)
QRL_HD constexpr unsigned bitrev3_to4(unsigned v) { return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1); }
QRL_HD constexpr unsigned trellis_point(unsigned s, unsigned t)
{
    return bitrev3_to4((t + 2u * (s & 1u) + 4u * (s >> 2)) & 7u) | (((s >> 1) ^ (s >> 2)) & 1u);
}
// the inverse: the tribit that takes state s to point p, 9 when the state cannot send p
QRL_HD constexpr unsigned trellis_tribit(unsigned s, unsigned p)
{
    if ((p & 1u) != (((s >> 1) ^ (s >> 2)) & 1u)) return 9u;
    const unsigned v = ((p >> 3) & 1u) | ((p >> 1) & 2u) | ((p << 1) & 4u);
    return (v - 2u * (s & 1u) - 4u * (s >> 2)) & 7u;
}
// bit position of transmitted dibit i (0 .. 97): 2 i, past the 68 middle bits of the burst from bit 98 on
QRL_HD inline unsigned dibit_pos(unsigned i) { const unsigned n = 2u * i; return n >= 98u ? n + 68u : n; }

QRL_HD inline void trellis_points(const uint8_t* burst, Nib49& pts)
{
    pts.w[0] = pts.w[1] = pts.w[2] = pts.w[3] = 0;
    for (unsigned k = 0; k < 49u; ++k) {
        const unsigned a = dibit_pos(2u * k), b = dibit_pos(2u * k + 1u);
        const unsigned n = (rd_bit(burst, a) << 3) | (rd_bit(burst, a + 1u) << 2) | (rd_bit(burst, b) << 1) | rd_bit(burst, b + 1u);
        nib_set(pts, c_dmr.tr_seq[k], c_dmr.con_point[n]);
    }
}
// CDMRTrellis::checkCode: the position of the first point its state cannot send, 48 for a last tribit other than 0, else TRELLIS_OK
QRL_HD inline unsigned trellis_check(const Nib49& pts, Nib49& tri)
{
    unsigned state = 0;
    for (unsigned i = 0; i < 49u; ++i) {
        const unsigned t = trellis_tribit(state, nib_get(pts, i));
        if (t == 9u) return i;
        nib_set(tri, i, t);
        state = t;
    }
    return state != 0u ? 48u : (unsigned)TRELLIS_OK;
}
QRL_HD inline void trellis_payload(const Nib49& tri, uint8_t* payload)
{
    for (unsigned i = 0; i < 48u; ++i) {
        const unsigned t = nib_get(tri, i), n = 143u - 3u * i;
        wr_bit(payload, n, t & 4u); wr_bit(payload, n - 1u, t & 2u); wr_bit(payload, n - 2u, t & 1u);
    }
}
// search statistics of the scalar decoder (what the tests assert their scenario set from)
struct TrellisStats { unsigned fail_pos; unsigned rounds; unsigned goes; bool stuck; };
// CDMRTrellis::fixCode, one candidate after the other
QRL_HD inline bool trellis_fix(Nib49& pts, unsigned fail_pos, Nib49& tri, TrellisStats* st)
{
    for (unsigned j = 0; j < 20u; ++j) {
        unsigned best_pos = 0, best_val = 0;
        if (st) ++st->rounds;
        for (unsigned i = 0; i < 16u; ++i) {
            nib_set(pts, fail_pos, i);
            const unsigned pos = trellis_check(pts, tri);
            if (pos == (unsigned)TRELLIS_OK) return true;
            if (pos > best_pos) { best_pos = pos; best_val = i; }
        }
        if (st && best_pos == 0) st->stuck = true;
        nib_set(pts, fail_pos, best_val);
        fail_pos = best_pos;
    }
    return false;
}
// CDMRTrellis::decode; payload is written only on success
QRL_HD inline bool trellis_decode(const uint8_t* burst, uint8_t* payload, TrellisStats* st = nullptr)
{
    Nib49 pts, tri{};
    trellis_points(burst, pts);
    const unsigned fail_pos = trellis_check(pts, tri);
    if (st) { st->fail_pos = fail_pos; st->rounds = 0; st->goes = 0; st->stuck = false; }
    if (fail_pos == (unsigned)TRELLIS_OK) { trellis_payload(tri, payload); return true; }
    const Nib49 save = pts;
    if (st) st->goes = 1;
    if (trellis_fix(pts, fail_pos, tri, st)) { trellis_payload(tri, payload); return true; }
    if (fail_pos == 0u) return false;
    pts = save;
    if (st) st->goes = 2;
    if (trellis_fix(pts, fail_pos - 1u, tri, st)) { trellis_payload(tri, payload); return true; }
    return false;
}
// CDMRTrellis::encode: the burst's 68 middle bits are kept
QRL_HD inline void trellis_encode(const uint8_t* payload, uint8_t* burst)
{
    Nib49 pts{};
    unsigned state = 0;
    for (unsigned i = 0; i < 49u; ++i) {
        unsigned t = 0;
        if (i < 48u) { const unsigned n = 143u - 3u * i; t = (rd_bit(payload, n) << 2) | (rd_bit(payload, n - 1u) << 1) | rd_bit(payload, n - 2u); }
        nib_set(pts, i, trellis_point(state, t));
        state = t;
    }
    for (unsigned k = 0; k < 49u; ++k) {
        const unsigned n = c_dmr.con_bits[nib_get(pts, c_dmr.tr_seq[k])];
        const unsigned a = dibit_pos(2u * k), b = dibit_pos(2u * k + 1u);
        wr_bit(burst, a, n & 8u); wr_bit(burst, a + 1u, n & 4u); wr_bit(burst, b, n & 2u); wr_bit(burst, b + 1u, n & 1u);
    }
}

// ---- voice: CAMBEFEC::regenerateDMR ----
QRL_HD inline uint32_t golay23_word(uint32_t data) { return (data << 11) | poly_rem(data << 11, 22, 11, 0xC75); }
QRL_HD inline uint32_t golay24_word(uint32_t data) { const uint32_t w = golay23_word(data); return (w << 1) | (popc32(w) & 1u); }
QRL_HD inline bool golay24_decode(uint32_t in, uint32_t& data)
{
    const uint32_t syn = poly_rem(in >> 1, 22, 11, 0xC75);
    const uint32_t out = in ^ (c_dmr.g23[syn] << 1);
    data = out >> 12;
    return popc32(syn) < 3u || !(popc32(out) & 1u);
}
QRL_HD inline uint32_t golay23_decode(uint32_t code) { return (code ^ c_dmr.g23[poly_rem(code, 22, 11, 0xC75)]) >> 11; }
// the AMBE pseudo-random word of a 12-bit seed: 23 top bits of the linear congruential sequence 173 x + 13849 mod 65536 from 16 seed
QRL_HD inline uint32_t ambe_prng23(uint32_t seed)
{
    uint32_t pr = 16u * seed, out = 0;
    for (int i = 0; i < 23; ++i) { pr = (173u * pr + 13849u) & 0xFFFFu; out = (out << 1) | (pr >> 15); }
    return out;
}
// Bit positions: the 72 bits of a codec frame are spread four apart (j -> 4 (j mod 18) + j / 18); the first 24 are the A word, the next
// 23 B, the last 25 C.  The burst holds three frames: bits 0..71, 72..107 + 156..191 (the 48 middle bits skipped), 192..263.
QRL_HD inline unsigned ambe_pos(unsigned j, unsigned frame)
{
    unsigned p = 4u * (j % 18u) + j / 18u;
    if (frame == 1u) { p += 72u; if (p >= 108u) p += 48u; }
    if (frame == 2u) p += 192u;
    return p;
}
// the codec's silence frame, what the reference substitutes for a frame it gives up on
enum : uint32_t { AMBE_SILENCE_A = 0xF00292u, AMBE_SILENCE_B = 0x0E0B20u, AMBE_SILENCE_C = 0u };
QRL_HD inline unsigned ambe_regenerate_words(uint32_t& a, uint32_t& b, uint32_t& c)
{
    const uint32_t orig_a = a, orig_b = b;
    uint32_t data = 0;
    if (!golay24_decode(a, data)) { a = AMBE_SILENCE_A; b = AMBE_SILENCE_B; c = AMBE_SILENCE_C; return 10u; }
    a = golay24_word(data);
    const uint32_t p = ambe_prng23(data);
    b ^= p;
    b = golay23_word(golay23_decode(b));
    b ^= p;
    const unsigned ea = popc32(a ^ orig_a), eb = popc32(b ^ orig_b);
    if (ea >= 4u || (ea + eb >= 6u && ea >= 2u)) { a = AMBE_SILENCE_A; b = AMBE_SILENCE_B; c = AMBE_SILENCE_C; }
    return ea + eb;
}
QRL_HD inline unsigned ambe_regenerate(uint8_t* burst)
{
    unsigned errors = 0;
    for (unsigned f = 0; f < 3u; ++f) {
        uint32_t a = 0, b = 0, c = 0;
        for (unsigned j = 0; j < 24u; ++j) a = (a << 1) | rd_bit(burst, ambe_pos(j, f));
        for (unsigned j = 24u; j < 47u; ++j) b = (b << 1) | rd_bit(burst, ambe_pos(j, f));
        for (unsigned j = 47u; j < 72u; ++j) c = (c << 1) | rd_bit(burst, ambe_pos(j, f));
        errors += ambe_regenerate_words(a, b, c);
        for (unsigned j = 0; j < 24u; ++j) wr_bit(burst, ambe_pos(j, f), (a >> (23u - j)) & 1u);
        for (unsigned j = 24u; j < 47u; ++j) wr_bit(burst, ambe_pos(j, f), (b >> (46u - j)) & 1u);
        for (unsigned j = 47u; j < 72u; ++j) wr_bit(burst, ambe_pos(j, f), (c >> (71u - j)) & 1u);
    }
    return errors;
}

// ---- the record ----
QRL_HD inline uint32_t id24(const uint8_t* p) { return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2]; }
QRL_HD inline void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// CDMRCSBK::put: which of bytes 4..6 / 7..9 is the source and which the destination, by opcode; an ID the opcode does not carry stays 0
QRL_HD inline void csbk_ids(const uint8_t* d, uint32_t& src, uint32_t& dst)
{
    const unsigned op = d[0] & 0x3Fu;
    const uint32_t lo = id24(d + 4), hi = id24(d + 7);
    src = hi; dst = lo;
    if (op == 0x38u) { dst = 0; }                                      // BS downlink activate: bytes 4..6 are the BS id
    else if (op == 0x26u) { src = lo; dst = hi; }                      // negative acknowledge response
    else if (op == 0x24u && d[3] != 0x80u) { src = lo; dst = hi; }     // radio check acknowledge
}

// Everything of a record except the rate 3/4 search.  Returns false when the burst is a rate 3/4 burst whose first check fails: the record
// is then complete as a failed burst (valid 0, the input burst, no payload), the caller runs the search and, on success, writes the payload, the
// re-encoded burst, length 18 and valid 1.
QRL_HD inline bool decode_record(const uint8_t* in, int audio_fec, uint8_t* out, bool search_here)
{
    for (int i = 0; i < REC_OUT; ++i) out[i] = 0;
    const unsigned ftype = in[0];
    out[R_FTYPE] = in[0]; out[R_FN] = in[1];
    uint8_t* burst = out + R_BURST;
    uint8_t* pay = out + R_PAYLOAD;
    for (int i = 0; i < BURST; ++i) burst[i] = in[4 + i];
    if (ftype == FT_VOICE || ftype == FT_VOICE_SYNC) {
        out[R_DTYPE] = ftype == FT_VOICE ? DT_VOICE : DT_VOICE_SYNC;
        out[R_VALID] = 1;
        if (audio_fec) out[R_ERRS] = (uint8_t)ambe_regenerate(burst);
        if (ftype == FT_VOICE) {
            const unsigned e = emb_decode(burst);
            out[R_CC] = (uint8_t)(e >> 4); out[R_PI] = (uint8_t)((e >> 3) & 1u); out[R_LCSS] = (uint8_t)((e >> 1) & 3u);
        } else out[R_CC] = in[2];
        out[R_PLEN] = 27;
        for (int i = 0; i < 14; ++i) pay[i] = burst[i];
        pay[13] = (uint8_t)((pay[13] & 0xF0u) | (burst[19] & 0x0Fu));
        for (int i = 0; i < 13; ++i) pay[14 + i] = burst[20 + i];
        return true;
    }
    if (ftype != FT_DATA) {   // a frame type the class does not know: its defaults (idle, colour code 255), validate() passes
        out[R_CC] = 255; out[R_DTYPE] = DT_IDLE; out[R_VALID] = 1;
        return true;
    }
    const unsigned st = slot_type_decode(burst);
    const unsigned dt = st & 15u;
    out[R_CC] = (uint8_t)(st >> 4); out[R_DTYPE] = (uint8_t)dt;
    if (dt == DT_RATE_34_DATA) {
        Nib49 pts, tri{};
        trellis_points(burst, pts);
        bool ok = trellis_check(pts, tri) == (unsigned)TRELLIS_OK;
        if (ok) trellis_payload(tri, pay);
        else if (search_here) ok = trellis_decode(burst, pay);
        else return false;
        if (ok) { trellis_encode(pay, burst); out[R_VALID] = 1; out[R_PLEN] = 18; }
        return true;
    }
    if (dt > DT_RATE_34_DATA) return true;   // idle, rate 1, reserved: validate() is false, nothing else is touched
    uint8_t d[12];
    bptc_decode(burst, d);
    uint32_t src = 0, dst = 0;
    unsigned flco = 0, fid = 0;
    if (dt == DT_VOICE_LC_HEADER || dt == DT_TERMINATOR_WITH_LC) {
        const uint8_t m = dt == DT_VOICE_LC_HEADER ? 0x96u : 0x99u;
        uint8_t x[12];
        for (int i = 0; i < 12; ++i) x[i] = i >= 9 ? (uint8_t)(d[i] ^ m) : d[i];
        if (!rs129_check(x)) return true;
        flco = d[0] & 0x3Fu; fid = d[1]; dst = id24(d + 3); src = id24(d + 6);
    } else if (dt == DT_CSBK || dt == DT_MBC_HEADER || dt == DT_MBC_CONTINUATION) {
        // CDMRCSBK::put checks under the CSBK mask whatever the data type and sets the type back to CSBK, so get() re-adds that CRC
        const unsigned crc = crc_ccitt10(d) ^ 0xA5A5u;
        if (d[10] != (crc >> 8) || d[11] != (crc & 0xFFu)) return true;
        flco = d[0] & 0x3Fu; fid = d[1];
        csbk_ids(d, src, dst);
    } else if (dt == DT_DATA_HEADER) {
        unsigned crc = crc_ccitt10(d) ^ 0xCCCCu;
        if (d[10] != (crc >> 8) || d[11] != (crc & 0xFFu)) return true;
        for (int i = 0; i < 12; ++i) pay[i] = d[i];   // as put() keeps it; get() below changes a UDT header
        const unsigned dpf = d[0] & 0x0Fu;
        if (dpf != 0x0Fu) {   // put() returns early for the proprietary format: no IDs
            dst = id24(d + 2); src = id24(d + 5);
            if (dpf == 0u) {  // UDT: the opcode, and get() clears bit 0 of byte 9 before the CRC is made again
                flco = d[9] & 0x3Fu;
                d[9] &= 0xFEu;
                crc = crc_ccitt10(d) ^ 0xCCCCu;
                d[10] = (uint8_t)(crc >> 8); d[11] = (uint8_t)crc;
            }
        }
    }
    if (dt != DT_DATA_HEADER) for (int i = 0; i < 12; ++i) pay[i] = d[i];
    bptc_encode(d, burst);
    out[R_VALID] = 1; out[R_PLEN] = 12; out[R_FLCO] = (uint8_t)flco; out[R_FID] = (uint8_t)fid;
    put32(out + R_SRC, src); put32(out + R_DST, dst);
    return true;
}
}  // namespace dmr
}  // namespace qrl
