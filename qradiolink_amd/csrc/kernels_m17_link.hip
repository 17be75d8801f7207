// kernels_m17_link.hip — the M17 link layer behind k_framesync (m17_link_core.hpp; reference src/gr_modem.cpp:1370-1439,
// src/M17/M17/M17FrameDecoder.cpp:111-159) and the transmit framing of a call (src/M17/M17/M17Transmitter.cpp:46-143, src/gr_modem.cpp:687-729,
// :868-884).
//   k_m17_link_decode   one lane per (stream, slot): the per-frame decode of m17_fec.hpp on the frame where the synchroniser wrote it, into the
//                       handle's 40-byte scratch record.  Slots behind the count, records of another size and EOT frames do no work.
//   k_m17_rx            one lane per stream, as k_dmr_rx: the lane loads its 64-byte state once (four 16-byte loads), walks its records
//                       i < min(counts[2 b + 1], cap) in order through m17_rx_step, writes one 64-byte record per slot (four 16-byte stores; zeros
//                       for the slots behind the count) and stores the state once.
//   k_m17_rx_state      the public 16 bytes of every state;  k_m17_rx_reset  every state to a fresh decoder's
//   k_m17_call          one lane per frame: the preamble and LSF frame of a call, stream frame first[b] + i, or the last frame and the EOT bytes
// The order of a stream's frames is the protocol, so the walk has no parallelism inside a stream; a wave is 64 streams.  The state and the
// record a step builds stay in registers: every index into them is a constant once the loops are unrolled (the LICH copy at 5 * segment is
// six compared cases, the base-40 division three 16-bit limbs).  Vector loads and stores only, no atomics; LDS only for the Viterbi's
// decision words.
#include "engine.hpp"
#include "m17_fec.hpp"
#include "m17_link_core.hpp"

namespace qrl {

using namespace m17;

static_assert(M17_RX_REC == M17_RX_RECORD_BYTES && M17_RX_STATE_SIZE == M17_RX_STATE_BYTES && M17_RX_STATE_PUBLIC == M17_RX_PUBLIC_BYTES &&
              M17_FS_REC == M17_FS_RECORD_BYTES && M17_DEC_REC == M17_DEC_RECORD_BYTES, "engine.hpp and m17_link_core.hpp agree");
static_assert(M17_RX_STATE_SIZE % 16 == 0 && M17_RX_REC % 16 == 0 && M17_DEC_REC % 4 == 0 && M17_FS_REC % 4 == 0, "the state and the records move as words");

__device__ __forceinline__ size_t slots_of(const uint32_t* counts, size_t b, size_t cap)
{
    const size_t c = counts[2 * b + 1];
    return c < cap ? c : cap;
}

__global__ __launch_bounds__(M17_TPB) void k_m17_link_decode(const uint8_t* __restrict__ frames, size_t frame_stride, const uint32_t* __restrict__ counts,
                                                              size_t batch, size_t cap, uint8_t* __restrict__ scratch)
{
    __shared__ uint16_t hist[M17_MAXSTEPS * M17_TPB];
    const size_t u = (size_t)blockIdx.x * M17_TPB + threadIdx.x;
    if (u >= batch * cap) return;
    const size_t b = u / cap, i = u - b * cap;
    if (i >= slots_of(counts, b, cap)) return;
    const uint8_t* f = frames + b * frame_stride + i * M17_FS_REC;
    const uint32_t ftype = reinterpret_cast<const uint32_t*>(f)[0], word1 = reinterpret_cast<const uint32_t*>(f)[1];
    if ((word1 & 0xFFFFu) != 46u || (ftype != FT_LSF && ftype != FT_STREAM)) return;
    uint8_t rec[M17_DEC_REC];
    m17_decode_frame((uint8_t)(ftype >> 8), (uint8_t)ftype, f + 8, hist + threadIdx.x, rec);       // frame[0], frame[1] of gr_modem.cpp:1375-1376
    uint32_t* dst = reinterpret_cast<uint32_t*>(scratch + u * M17_DEC_REC);
    for (int k = 0; k < M17_DEC_REC / 4; ++k)
        dst[k] = (uint32_t)rec[4 * k] | ((uint32_t)rec[4 * k + 1] << 8) | ((uint32_t)rec[4 * k + 2] << 16) | ((uint32_t)rec[4 * k + 3] << 24);
}

__global__ __launch_bounds__(64) void k_m17_rx(const uint8_t* __restrict__ frames, size_t frame_stride, const uint32_t* __restrict__ counts, size_t batch,
                                               size_t cap, int can_rx, int decode_all_can, const uint8_t* __restrict__ scratch,
                                               m17_rx_state* __restrict__ states, uint8_t* __restrict__ out)
{
    const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const m17_rx_config cfg = {can_rx, decode_all_can};
    m17_rx_state st;
    uint4* sp = reinterpret_cast<uint4*>(states + b);
    {
        const uint4 a = sp[0], c = sp[1], e = sp[2], g = sp[3];
        st.lsf[0] = a.x; st.lsf[1] = a.y; st.lsf[2] = a.z; st.lsf[3] = a.w; st.lsf[4] = c.x; st.lsf[5] = c.y; st.lsf[6] = c.z; st.lsf[7] = c.w;
        st.lich[0] = e.x; st.lich[1] = e.y; st.lich[2] = e.z; st.lich[3] = e.w; st.lich[4] = g.x; st.lich[5] = g.y; st.lich[6] = g.z; st.lich[7] = g.w;
    }
    const size_t n = slots_of(counts, b, cap);
    const uint8_t* f = frames + b * frame_stride;
    const uint32_t* dec = reinterpret_cast<const uint32_t*>(scratch + b * cap * M17_DEC_REC);
    uint4* dst = reinterpret_cast<uint4*>(out + b * cap * M17_RX_REC);
    for (size_t i = 0; i < cap; ++i, f += M17_FS_REC, dec += M17_DEC_REC / 4, dst += M17_RX_REC / 16) {
        uint32_t r[M17_RX_REC / 4];
        if (i < n) {
            const uint32_t ftype = reinterpret_cast<const uint32_t*>(f)[0], word1 = reinterpret_cast<const uint32_t*>(f)[1];
            uint32_t d[M17_DEC_REC / 4];
            const bool decoded = (word1 & 0xFFFFu) == 46u && (ftype == FT_LSF || ftype == FT_STREAM);   // what k_m17_link_decode wrote
#pragma unroll
            for (int k = 0; k < M17_DEC_REC / 4; ++k) d[k] = decoded ? dec[k] : 0u;
            m17_rx_step(cfg, st, ftype, word1, d, r);
        } else {
#pragma unroll
            for (int k = 0; k < M17_RX_REC / 4; ++k) r[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < M17_RX_REC / 16; ++k) dst[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    }
    sp[0] = make_uint4(st.lsf[0], st.lsf[1], st.lsf[2], st.lsf[3]); sp[1] = make_uint4(st.lsf[4], st.lsf[5], st.lsf[6], st.lsf[7]);
    sp[2] = make_uint4(st.lich[0], st.lich[1], st.lich[2], st.lich[3]); sp[3] = make_uint4(st.lich[4], st.lich[5], st.lich[6], st.lich[7]);
}

__global__ __launch_bounds__(64) void k_m17_rx_state(const m17_rx_state* __restrict__ states, size_t batch, uint4* __restrict__ out)
{
    const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const uint4* sp = reinterpret_cast<const uint4*>(states + b);
    const uint4 a = sp[0], c = sp[1];
    m17_rx_state st;
    st.lsf[0] = a.x; st.lsf[1] = a.y; st.lsf[2] = a.z; st.lsf[3] = a.w; st.lsf[4] = c.x; st.lsf[5] = c.y; st.lsf[6] = c.z; st.lsf[7] = c.w;
    uint32_t w[4];
    m17_rx_public(st, w);
    out[b] = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(64) void k_m17_rx_reset(m17_rx_state* __restrict__ states, size_t batch)
{
    const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const m17_rx_state st = m17_rx_fresh();
    uint4* sp = reinterpret_cast<uint4*>(states + b);
    sp[0] = make_uint4(st.lsf[0], st.lsf[1], st.lsf[2], st.lsf[3]); sp[1] = make_uint4(st.lsf[4], st.lsf[5], st.lsf[6], st.lsf[7]);
    sp[2] = make_uint4(st.lich[0], st.lich[1], st.lich[2], st.lich[3]); sp[3] = make_uint4(st.lich[4], st.lich[5], st.lich[6], st.lich[7]);
}

// kind 0: out row b = 48 preamble bytes 0x77, the LSF frame (n = 1).  kind 1: slot i of row b = stream frame first[b] + i with payload
// payloads[b][i], zeros up to slot_bytes.  kind 2: out row b = the last frame (index first[b], zero payload, EOS), sixteen EOT bytes (n = 1).
__global__ __launch_bounds__(64) void k_m17_call(int kind, const uint8_t* __restrict__ calls, const uint8_t* __restrict__ payloads,
                                                 const uint32_t* __restrict__ first, size_t batch, size_t n, uint8_t* __restrict__ out, size_t out_stride,
                                                 size_t slot_bytes)
{
    const size_t u = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= batch * n) return;
    const size_t b = u / n, i = u - b * n;
    uint8_t desc[M17_CALL_BYTES];
    for (int k = 0; k < M17_CALL_BYTES; ++k) desc[k] = calls[b * M17_CALL_BYTES + k];
    uint32_t lsf[8], rw[M17_DEC_REC / 4];
    call_lsf(desc, lsf);
    uint8_t* o = out + b * out_stride + i * slot_bytes;
    if (kind == 0) {
        for (int k = 0; k < M17_FRAME; ++k) o[k] = 0x77;
        o += M17_FRAME;
        lsf_record(lsf, rw);
    } else {
        uint32_t pay[4] = {0, 0, 0, 0};
        if (kind == 1) {
            const uint8_t* p = payloads + u * 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) pay[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        }
        stream_record(lsf, (first ? first[b] : 0u) + (uint32_t)i, pay, kind == 2, rw);
    }
    uint8_t rec[M17_DEC_REC];
#pragma unroll
    for (int k = 0; k < M17_DEC_REC; ++k) rec[k] = (uint8_t)(rw[k >> 2] >> (8 * (k & 3)));
    m17_encode_frame(rec, o);
    if (kind == 1) for (size_t k = M17_FRAME; k < slot_bytes; ++k) o[k] = 0;
    if (kind == 2) for (int k = 0; k < 16; k += 2) { o[M17_FRAME + k] = 0x55; o[M17_FRAME + k + 1] = 0x5D; }   // FrameTypeM17EOT, gr_modem.cpp:724-728
}

void launch_m17_rx(const uint8_t* frames, size_t frame_stride, const uint32_t* counts, size_t batch, size_t cap, int can_rx, int decode_all_can,
                   uint8_t* scratch, void* states, uint8_t* out, hipStream_t s)
{
    if (!batch || !cap) return;
    const size_t lanes = batch * cap;
    hipLaunchKernelGGL(k_m17_link_decode, dim3((unsigned)((lanes + M17_TPB - 1) / M17_TPB)), dim3(M17_TPB), 0, s, frames, frame_stride, counts, batch, cap,
                       scratch);
    hipLaunchKernelGGL(k_m17_rx, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, frames, frame_stride, counts, batch, cap, can_rx, decode_all_can,
                       scratch, static_cast<m17_rx_state*>(states), out);
}
void launch_m17_rx_state(const void* states, size_t batch, uint8_t* out, hipStream_t s)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_m17_rx_state, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, static_cast<const m17_rx_state*>(states), batch,
                       reinterpret_cast<uint4*>(out));
}
void launch_m17_rx_reset(void* states, size_t batch, hipStream_t s)
{
    if (!batch) return;
    hipLaunchKernelGGL(k_m17_rx_reset, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, static_cast<m17_rx_state*>(states), batch);
}
void launch_m17_call(int kind, const uint8_t* calls, const uint8_t* payloads, const uint32_t* first, size_t batch, size_t n, uint8_t* out,
                     size_t out_stride, size_t slot_bytes, hipStream_t s)
{
    if (!batch || !n) return;
    const size_t lanes = batch * n;
    hipLaunchKernelGGL(k_m17_call, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, kind, calls, payloads, first, batch, n, out, out_stride,
                       slot_bytes);
}

}  // namespace qrl
