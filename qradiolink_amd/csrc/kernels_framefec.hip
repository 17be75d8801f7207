// kernels_framefec.hip — frame FEC of the DMR and M17 protocol stacks over batches of frames:
//   k_bptc_decode / k_bptc_encode   CBPTC19696::decode / encode   reference src/MMDVM/BPTC19696.cpp:47-87, Hamming (15,11,3) and
//                                   (13,9,3) src/MMDVM/Hamming.cpp:79-180
//   k_m17_decode                    M17FrameDecoder::decodeFrame   reference src/M17/M17/M17FrameDecoder.cpp:44-215 (decorrelator,
//                                   quadratic de-interleaver, sync-word classification, punctured K = 5 Viterbi M17Viterbi.hpp:96-221,
//                                   Golay(24,12) of the LICH M17Golay.cpp:24-95)
// Integer / bit work, one thread per frame.  BPTC: the 13 x 15 code matrix lives in 13 registers (one row each), the column code is
// decoded bit-sliced for all 15 columns at once (four syndrome planes, thirteen flip masks), the row code by syndrome -> column match.
// M17: 16 path metrics in registers, the decision words of the (at most 244) trellis steps in LDS, [step][thread].
// Results = oracle/orc_framefec.c, which is pinned against the reference's own sources (oracle/_ref).
#include "engine.hpp"
#include "m17_fec.hpp"

namespace qrl {

// parity equations over the data bits (ETSI TS 102 361-1 B.3): bit j of mask p set = data bit j enters parity p
__constant__ uint16_t c_h15[4] = {0x01AF, 0x035E, 0x06BC, 0x04D7};
__constant__ uint16_t c_h13[4] = {0x006B, 0x00D7, 0x01AF, 0x0135};

__device__ __forceinline__ unsigned par32(unsigned v) { return (unsigned)__popc(v) & 1u; }

// syndrome of a (k + 4)-bit word, and the word with the single error that syndrome names flipped (none if it names no column)
__device__ __forceinline__ unsigned hamming_fix(unsigned w, const uint16_t* mask, int k, bool& fixed)
{
    unsigned syn = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) syn |= (par32(w & mask[p]) ^ ((w >> (k + p)) & 1u)) << p;
    fixed = false;
    if (!syn) return w;
    for (int j = 0; j < k + 4; ++j) {
        unsigned col;
        if (j < k) col = ((mask[0] >> j) & 1u) | (((mask[1] >> j) & 1u) << 1) | (((mask[2] >> j) & 1u) << 2) | (((mask[3] >> j) & 1u) << 3);
        else col = 1u << (j - k);
        if (col == syn) { fixed = true; return w ^ (1u << j); }
    }
    return w;
}

// transmitted bit i (0 .. 195) of a 33-byte burst: bytes 0..11, the top two bits of byte 12, the low two bits of byte 20, bytes 21..32
__device__ __forceinline__ unsigned burst_bit(const uint8_t* in, int i)
{
    if (i < 98) return (in[i >> 3] >> (7 - (i & 7))) & 1u;
    if (i < 100) return (in[20] >> (99 - i)) & 1u;
    const int k = i - 100;
    return (in[21 + (k >> 3)] >> (7 - (k & 7))) & 1u;
}

__global__ __launch_bounds__(64) void k_bptc_decode(const uint8_t* __restrict__ bursts, size_t n, uint8_t* __restrict__ payloads)
{
    const size_t f = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t in[33];
    for (int i = 0; i < 33; ++i) in[i] = bursts[f * 33 + i];
    // de-interleave: matrix bit a (1 .. 195; bit 0 = R(3), unused) = transmitted bit (181 a) mod 196; row r holds bits 1 + 15 r ..
    unsigned row[13];
#pragma unroll
    for (int r = 0; r < 13; ++r) {
        unsigned w = 0;
        for (int j = 0; j < 15; ++j) w |= burst_bit(in, ((1 + 15 * r + j) * 181) % 196) << j;
        row[r] = w;
    }
    bool fixing;
    int count = 0;
    do {
        fixing = false;
        // columns, Hamming (13,9,3), all 15 at once: plane p = the p-th syndrome bit of every column
        unsigned s[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            unsigned v = row[9 + p];
#pragma unroll
            for (int a = 0; a < 9; ++a) if ((c_h13[p] >> a) & 1u) v ^= row[a];
            s[p] = v;
        }
#pragma unroll
        for (int a = 0; a < 13; ++a) {
            unsigned m = 0x7FFFu;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const unsigned bit = a < 9 ? (c_h13[p] >> a) & 1u : (unsigned)(a - 9 == p);
                m &= bit ? s[p] : ~s[p];
            }
            row[a] ^= m;
            fixing |= m != 0;
        }
        // the 9 rows that carry data, Hamming (15,11,3)
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            bool fx;
            row[r] = hamming_fix(row[r], c_h15, 11, fx);
            fixing |= fx;
        }
        ++count;
    } while (fixing && count < 5);
    // payload: row 0 bits 3..10, rows 1..8 bits 0..10, MSB first
    uint64_t lo = 0;   // 96 bits as 64 + 32
    unsigned hi = 0;
    int pos = 0;
    auto put = [&](unsigned bit) { if (pos < 64) lo |= (uint64_t)bit << (63 - pos); else hi |= bit << (95 - pos); ++pos; };
    for (int j = 3; j <= 10; ++j) put((row[0] >> j) & 1u);
    for (int r = 1; r <= 8; ++r) for (int j = 0; j <= 10; ++j) put((row[r] >> j) & 1u);
    for (int b = 0; b < 8; ++b) payloads[f * 12 + b] = (uint8_t)(lo >> (56 - 8 * b));
    for (int b = 0; b < 4; ++b) payloads[f * 12 + 8 + b] = (uint8_t)(hi >> (24 - 8 * b));
}

__global__ __launch_bounds__(64) void k_bptc_encode(const uint8_t* __restrict__ payloads, size_t n, uint8_t* __restrict__ bursts)
{
    const size_t f = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t in[12];
    for (int i = 0; i < 12; ++i) in[i] = payloads[f * 12 + i];
    auto bit = [&](int i) { return (unsigned)(in[i >> 3] >> (7 - (i & 7))) & 1u; };
    unsigned row[13];
    int pos = 0;
    {
        unsigned w = 0;
        for (int j = 3; j <= 10; ++j) w |= bit(pos++) << j;
        row[0] = w;
    }
    for (int r = 1; r <= 8; ++r) { unsigned w = 0; for (int j = 0; j <= 10; ++j) w |= bit(pos++) << j; row[r] = w; }
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int p = 0; p < 4; ++p) row[r] |= par32(row[r] & c_h15[p]) << (11 + p);
#pragma unroll
    for (int p = 0; p < 4; ++p) {      // column parities, bit-sliced: parity row 9 + p = XOR of the data rows of its equation
        unsigned v = 0;
#pragma unroll
        for (int a = 0; a < 9; ++a) if ((c_h13[p] >> a) & 1u) v ^= row[a];
        row[9 + p] = v;
    }
    // interleave into the burst: transmitted bit (181 a) mod 196 = matrix bit a, matrix bit 0 = 0; the burst's other bits are kept
    uint8_t out[33];
    for (int i = 0; i < 33; ++i) out[i] = bursts[f * 33 + i];
    for (int i = 0; i < 12; ++i) { out[i] = 0; out[21 + i] = 0; }
    out[12] &= 0x3Fu; out[20] &= 0xFCu;
    for (int a = 1; a < 196; ++a) {
        const unsigned b = (row[(a - 1) / 15] >> ((a - 1) % 15)) & 1u;
        const int t = (a * 181) % 196;
        if (t < 98) out[t >> 3] |= (uint8_t)(b << (7 - (t & 7)));
        else if (t < 100) out[20] |= (uint8_t)(b << (99 - t));
        else out[21 + ((t - 100) >> 3)] |= (uint8_t)(b << (7 - ((t - 100) & 7)));
    }
    for (int i = 0; i < 33; ++i) bursts[f * 33 + i] = out[i];
}
void launch_bptc_decode(const uint8_t* bursts, size_t n, uint8_t* payloads, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_bptc_decode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, bursts, n, payloads);
}
void launch_bptc_encode(const uint8_t* payloads, size_t n, uint8_t* bursts, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_bptc_encode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, payloads, n, bursts);
}

// ------------------------------------------------------------------------------------------------------------------ M17
// the per-frame work is m17_fec.hpp's, shared with the link layer (kernels_m17_link.hip)
__global__ __launch_bounds__(M17_TPB) void k_m17_decode(const uint8_t* __restrict__ frames, size_t n, uint8_t* __restrict__ records)
{
    __shared__ uint16_t hist[M17_MAXSTEPS * M17_TPB];
    const size_t f = (size_t)blockIdx.x * M17_TPB + threadIdx.x;
    if (f >= n) return;
    uint8_t rec[40];
    m17_decode_frame(frames[f * 48], frames[f * 48 + 1], frames + f * 48 + 2, hist + threadIdx.x, rec);
    for (int i = 0; i < 40; ++i) records[f * 40 + i] = rec[i];
}
// M17FrameEncoder::encodeLsf / encodeStreamFrame (reference src/M17/M17/M17FrameEncoder.cpp:52-118), stateless: a record as
// k_m17_decode writes it -> the frame (m17_encode_frame).  Thread per frame.
__global__ __launch_bounds__(64) void k_m17_encode(const uint8_t* __restrict__ records, size_t n, uint8_t* __restrict__ frames)
{
    const size_t f = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t rec[40];
    for (int i = 0; i < 40; ++i) rec[i] = records[f * 40 + i];
    m17_encode_frame(rec, frames + f * 48);
}
void launch_m17_encode(const uint8_t* records, size_t n, uint8_t* frames, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_m17_encode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, records, n, frames);
}
void launch_m17_decode(const uint8_t* frames, size_t n, uint8_t* records, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_m17_decode, dim3((unsigned)((n + M17_TPB - 1) / M17_TPB)), dim3(M17_TPB), 0, s, frames, n, records);
}

}  // namespace qrl
