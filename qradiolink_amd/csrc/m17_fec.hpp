// m17_fec.hpp — the per-frame FEC of M17 as device functions, shared by kernels_framefec.hip (k_m17_decode, k_m17_encode) and
// kernels_m17_link.hip (the decode stage of the link layer, the transmit kernels): M17FrameDecoder::decodeFrame, reference
// src/M17/M17/M17FrameDecoder.cpp:44-215 (decorrelator, quadratic de-interleaver, sync-word classification, punctured K = 5 Viterbi
// M17Viterbi.hpp:96-221, Golay(24,12) of the LICH M17Golay.cpp:24-95) and M17FrameEncoder::encodeLsf / encodeStreamFrame,
// src/M17/M17/M17FrameEncoder.cpp:52-118.  Device only; a translation unit that includes it gets its own copy of the two constant tables.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace qrl {

static __constant__ uint8_t c_m17_seq[46] = {
    0xD6, 0xB5, 0xE2, 0x30, 0x82, 0xFF, 0x84, 0x62, 0xBA, 0x4E, 0x96, 0x90, 0xD8, 0x98, 0xDD, 0x5D, 0x0C, 0xC8, 0x52, 0x43, 0x91, 0x1D, 0xF8,
    0x6E, 0x68, 0x2F, 0x35, 0xDA, 0x14, 0xEA, 0xCD, 0x76, 0x19, 0x8D, 0xD5, 0x80, 0xD1, 0x33, 0x87, 0x13, 0x57, 0x18, 0x2D, 0x29, 0x78, 0xC3};
// Golay(24,12) with generator polynomial 0xC75, tables by rule at compile time: checksum of data bit i = (x^(i + 11) mod g) << 1 | the
// overall parity of the 23-bit word; dec = the inverse map (parity error pattern -> data error pattern) by Gaussian elimination
struct GolayTables { uint16_t enc[12], dec[12]; };
constexpr GolayTables make_golay()
{
    GolayTables t{};
    for (int i = 0; i < 12; ++i) {
        uint32_t v = (uint32_t)1 << (i + 11);
        for (int b = 22; b >= 11; --b) if (v & ((uint32_t)1 << b)) v ^= (uint32_t)0xC75 << (b - 11);
        uint32_t cw = ((uint32_t)1 << (i + 11)) | v, par = 0;
        for (int b = 0; b < 23; ++b) par ^= (cw >> b) & 1u;
        t.enc[i] = (uint16_t)((v << 1) | par);
    }
    uint32_t m[12] = {};
    for (int i = 0; i < 12; ++i) m[i] = ((uint32_t)t.enc[i] << 12) | ((uint32_t)1 << i);
    for (int c = 0; c < 12; ++c) {
        int p = c;
        while (!(m[p] & ((uint32_t)1 << (12 + c)))) ++p;
        const uint32_t sw = m[p]; m[p] = m[c]; m[c] = sw;
        for (int r = 0; r < 12; ++r) if (r != c && (m[r] & ((uint32_t)1 << (12 + c)))) m[r] ^= m[c];
    }
    for (int c = 0; c < 12; ++c) t.dec[c] = (uint16_t)(m[c] & 0xFFFu);
    return t;
}
static __constant__ GolayTables c_gol = make_golay();
#define c_gol_enc c_gol.enc
#define c_gol_dec c_gol.dec

__device__ inline unsigned golay24_decode(unsigned cw)   // 0xFFFF: uncorrectable
{
    const unsigned data = (cw >> 12) & 0xFFFu, parity = cw & 0xFFFu;
    unsigned chk = 0;
    for (int i = 0; i < 12; ++i) if (data & (1u << i)) chk ^= c_gol_enc[i];
    const unsigned syn = parity ^ chk;
    if (__popc(syn) <= 3) return ((cw ^ syn) >> 12) & 0xFFFu;
    for (int i = 0; i < 12; ++i)
        if (__popc(syn ^ c_gol_enc[i]) <= 2) return (data ^ (1u << i)) & 0xFFFu;
    unsigned inv = 0;
    for (int i = 0; i < 12; ++i) if (syn & (1u << i)) inv ^= c_gol_dec[i];
    if (__popc(inv) <= 3) return (data ^ inv) & 0xFFFu;
    for (int i = 0; i < 12; ++i)
        if (__popc(inv ^ c_gol_dec[i]) <= 2) return (data ^ inv ^ c_gol_dec[i]) & 0xFFFu;
    return 0xFFFFu;
}

constexpr int M17_TPB = 64, M17_MAXSTEPS = 244;

// punctured hard-decision Viterbi (K = 5, G1 = 0x19, G2 = 0x17) of nbits received bits starting at bit `first` of di[]; the puncture
// matrix is "every fourth entry, starting with the third, is dropped" over 61 entries (LSF) or "the twelfth of twelve" (stream)
__device__ inline void m17_viterbi(const uint8_t* di, int first, int nbits, bool lsf, uint16_t* hist /* [step * M17_TPB] */, uint8_t* out, int nbytes)
{
    unsigned prev[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) prev[i] = 0;
    const int P = lsf ? 61 : 12;
    int steps = 0, pi = 0, bp = 0;
    while (bp < nbits) {
        int sym[2] = {1, 1};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool keep = lsf ? (pi & 3) != 2 : pi != 11;
            ++pi;
            if (keep) { const int b = first + bp; sym[k] = ((di[b >> 3] >> (7 - (b & 7))) & 1) ? 2 : 0; ++bp; }
            if (pi >= P) pi = 0;
        }
        unsigned cur[16], h = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c0 = i >= 4 ? 2 : 0, c1 = ((i + 1) & 2) ? 2 : 0;       // expected pair of predecessor i on input 0
            const unsigned metric = (unsigned)(abs(c0 - sym[0]) + abs(c1 - sym[1]));
            const unsigned m0 = prev[i] + metric, m1 = prev[i + 8] + (4 - metric);
            const unsigned m2 = prev[i] + (4 - metric), m3 = prev[i + 8] + metric;
            if (m0 >= m1) { h |= 1u << (2 * i); cur[2 * i] = m1; } else cur[2 * i] = m0;
            if (m2 >= m3) { h |= 1u << (2 * i + 1); cur[2 * i + 1] = m3; } else cur[2 * i + 1] = m2;
        }
        hist[steps * M17_TPB] = (uint16_t)h;
        ++steps;
#pragma unroll
        for (int i = 0; i < 16; ++i) prev[i] = cur[i] & 0xFFFFu;   // the reference's metrics are 16-bit
    }
    unsigned state = 0;
    int pos = steps;
    for (int b = nbytes * 8 - 1; b >= 0; --b) {
        --pos;
        const unsigned bit = (hist[pos * M17_TPB] >> (state >> 4)) & 1u;
        state = (state >> 1) | (bit << 7);
        if (bit) out[b >> 3] |= (uint8_t)(0x80u >> (b & 7));
    }
}

// decodeFrame of the sync word s0 s1 and the 46 bytes behind it -> rec[40] = {type (M17FrameType: 0 preamble, 1 link setup, 2 stream,
// 4 unknown), LICH ok, payload[30] (30 LSF bytes | 18 stream-frame bytes), LICH[5] at 32, segment number at 37, zeros}.  h: the lane's column
// of the block's [M17_MAXSTEPS][M17_TPB] decision words in LDS
__device__ __forceinline__ void m17_decode_frame(uint8_t s0, uint8_t s1, const uint8_t* __restrict__ body, uint16_t* h, uint8_t* rec)
{
    uint8_t data[46], di[46];
    for (int i = 0; i < 46; ++i) { data[i] = body[i] ^ c_m17_seq[i]; di[i] = 0; }
    for (int i = 0; i < 40; ++i) rec[i] = 0;
    for (unsigned i = 0; i < 368; ++i) {
        const unsigned src = (45u * i + 92u * i * i) % 368u;
        if ((data[src >> 3] >> (7 - (src & 7))) & 1u) di[i >> 3] |= (uint8_t)(0x80u >> (i & 7));
    }
    // nearest sync word: preamble 0x7777, link setup 0x55F7, stream 0xFF5D; strictly smaller distance wins; > 4 bit errors: unknown
    int type = 0, best = __popc((unsigned)(s0 ^ 0x77)) + __popc((unsigned)(s1 ^ 0x77));
    int d = __popc((unsigned)(s0 ^ 0x55)) + __popc((unsigned)(s1 ^ 0xF7));
    if (d < best) { best = d; type = 1; }
    d = __popc((unsigned)(s0 ^ 0xFF)) + __popc((unsigned)(s1 ^ 0x5D));
    if (d < best) { best = d; type = 2; }
    if (best > 4) type = 4;
    rec[0] = (uint8_t)type;
    if (type == 1) m17_viterbi(di, 0, 368, true, h, rec + 2, 30);
    if (type == 2) {
        unsigned dec[4];
        bool ok = true;
        for (int i = 0; i < 4 && ok; ++i) {
            dec[i] = golay24_decode(((unsigned)di[3 * i] << 16) | ((unsigned)di[3 * i + 1] << 8) | di[3 * i + 2]);
            ok = dec[i] != 0xFFFFu;
        }
        if (ok) {
            rec[32] = (uint8_t)(dec[0] >> 4); rec[33] = (uint8_t)(((dec[0] & 0xFu) << 4) | (dec[1] >> 8)); rec[34] = (uint8_t)(dec[1] & 0xFFu);
            rec[35] = (uint8_t)(dec[2] >> 4); rec[36] = (uint8_t)(((dec[2] & 0xFu) << 4) | (dec[3] >> 8)); rec[37] = (uint8_t)((dec[3] & 0xFFu) >> 5);
            rec[1] = 1;
        }
        m17_viterbi(di, 96, 272, false, h, rec + 2, 18);
    }
}

// encodeLsf / encodeStreamFrame of a record as m17_decode_frame writes it -> the 48-byte frame: K = 5 convolutional code (+ four flush
// bits), puncturing, Golay(24,12) of the LICH blocks, quadratic interleaver, randomiser, sync word
__device__ __forceinline__ void m17_encode_frame(const uint8_t* rec, uint8_t* __restrict__ frame)
{
    uint8_t body[46], il[46];
    for (int i = 0; i < 46; ++i) { body[i] = 0; il[i] = 0; }
    const bool lsf = rec[0] == 1;
    int ob = 0;
    if (!lsf) {
        const unsigned num = rec[37];
        const unsigned blocks[4] = {((unsigned)rec[32] << 4) | (rec[33] >> 4), (((unsigned)rec[33] & 0xFu) << 8) | rec[34],
                                    ((unsigned)rec[35] << 4) | (rec[36] >> 4), (((unsigned)rec[36] & 0xFu) << 8) | ((num << 5) & 0xFFu)};
        for (int i = 0; i < 4; ++i) {
            unsigned chk = 0;
            for (int k = 0; k < 12; ++k) if (blocks[i] & (1u << k)) chk ^= c_gol_enc[k];
            const unsigned cw = (blocks[i] << 12) | chk;
            body[3 * i] = (uint8_t)(cw >> 16); body[3 * i + 1] = (uint8_t)(cw >> 8); body[3 * i + 2] = (uint8_t)cw;
        }
        ob = 96;
    }
    const int nbits = lsf ? 240 : 144, P = lsf ? 61 : 12;
    unsigned mem = 0;
    int pi = 0;
    for (int i = 0; i < nbits + 4 && ob < 368; ++i) {
        const unsigned bit = i < nbits ? (rec[2 + (i >> 3)] >> (7 - (i & 7))) & 1u : 0u;
        mem = ((mem << 1) | bit) & 0x1Fu;
        const unsigned c[2] = {(unsigned)__popc(mem & 0x19u) & 1u, (unsigned)__popc(mem & 0x17u) & 1u};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool keep = lsf ? (pi & 3) != 2 : pi != 11;
            if (++pi >= P) pi = 0;
            if (keep && ob < 368) { if (c[k]) body[ob >> 3] |= (uint8_t)(0x80u >> (ob & 7)); ++ob; }
        }
    }
    for (unsigned i = 0; i < 368; ++i) {
        if ((body[i >> 3] >> (7 - (i & 7))) & 1u) {
            const unsigned d = (45u * i + 92u * i * i) % 368u;
            il[d >> 3] |= (uint8_t)(0x80u >> (d & 7));
        }
    }
    frame[0] = lsf ? 0x55 : 0xFF;
    frame[1] = lsf ? 0xF7 : 0x5D;
    for (int i = 0; i < 46; ++i) frame[2 + i] = il[i] ^ c_m17_seq[i];
}

}  // namespace qrl
#undef c_gol_enc
#undef c_gol_dec
