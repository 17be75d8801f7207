// kernels_dmr_tx.hip — DMR layer 2 on the transmit side: TX records, or a call descriptor plus codec frames, to the 33-byte bursts the DMR
// modulator takes (dmr_tx_core.hpp: what DMRFrame::constructLCFrame / constructCSBKFrame / setVoice / setEmbeddedData and
// DMRControl::getTxAudio do on the CPU in the reference, src/DMR/dmrframe.cpp:399-501, src/DMR/dmrcontrol.cpp:128-223).
//   k_dmr_tx        one lane per output slot: encode_record of records[b][i]
//   k_dmr_tx_call   one lane per output slot: voice_call_record of burst first[b] + i of call b, then encode_record
// A block is one wave.  A lane keeps its record and the burst it builds from it in LDS, 21 dwords per lane (nine for the burst, its last three
// bytes zero, twelve for the record; the stride is odd, so lanes at the same byte meet no bank twice): encode_record walks both bit by bit
// with computed indices, which on arrays in registers turns into chains of selects per access (262 144 mixed records: 1.88 ms with both
// in registers, 0.23 ms with both in LDS).  The wave then stores its 64 slots together, lane l the l-th, (l + 64)-th ... unit of the wave's run of slots: whole
// dwords when the output pointer, out_stride and slot_bytes are all multiples of four, single bytes otherwise; units behind byte 32 of a
// slot are the idle zeros.  With out_stride = cap * slot_bytes a wave's stores are one contiguous run of 64 * slot_bytes bytes.  Slots at
// or past min(counts[b], cap) are staged as zeros.  Nothing between cap * slot_bytes and out_stride of a stream is written.  No atomics,
// nothing carried from call to call.
#include "engine.hpp"
#include "dmr_tx_core.hpp"

namespace qrl {

using namespace dmr;

constexpr unsigned STAGE_DW = 9, LANE_DW = STAGE_DW + TX_REC / 4;   // dwords of a staged burst; dwords a lane owns in LDS

// the lane's burst (zeroed here, its pad bytes included) and, behind it, its record
__device__ __forceinline__ uint8_t* lane_burst(uint32_t* lds, unsigned lane)
{
    uint32_t* mine = lds + lane * LANE_DW;
    for (unsigned w = 0; w < STAGE_DW; ++w) mine[w] = 0;
    return reinterpret_cast<uint8_t*>(mine);
}

// slots r0 .. r0 + nslots - 1 (nslots <= 64) of the staged wave to their places; slot r lies at out + (r / cap) * out_stride + (r % cap) * slot_bytes
__device__ __forceinline__ void store_wave(const uint32_t* lds, unsigned lane, size_t r0, unsigned nslots, size_t cap, uint8_t* out, size_t out_stride,
                                           size_t slot_bytes, bool dwords)
{
    if (dwords) {
        const size_t slot_dw = slot_bytes >> 2, total = (size_t)nslots * slot_dw;
        for (size_t u = lane; u < total; u += 64) {
            const size_t s = u / slot_dw, w = u - s * slot_dw, r = r0 + s, b = r / cap, i = r - b * cap;
            const uint32_t v = w < STAGE_DW ? lds[s * LANE_DW + w] : 0u;
            *reinterpret_cast<uint32_t*>(out + b * out_stride + i * slot_bytes + 4u * w) = v;
        }
    } else {
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(lds);
        const size_t total = (size_t)nslots * slot_bytes;
        for (size_t u = lane; u < total; u += 64) {
            const size_t s = u / slot_bytes, w = u - s * slot_bytes, r = r0 + s, b = r / cap, i = r - b * cap;
            out[b * out_stride + i * slot_bytes + w] = w < (size_t)BURST ? bytes[s * (4u * LANE_DW) + w] : (uint8_t)0;
        }
    }
}

__global__ __launch_bounds__(64) void k_dmr_tx(const uint8_t* __restrict__ records, const uint32_t* __restrict__ counts, size_t batch, size_t cap,
                                               uint8_t* __restrict__ out, size_t out_stride, size_t slot_bytes, int dwords)
{
    __shared__ uint32_t lds[64 * LANE_DW];
    const unsigned lane = threadIdx.x;
    const size_t n = batch * cap, r0 = (size_t)blockIdx.x * 64, r = r0 + lane;
    uint8_t* burst = lane_burst(lds, lane);
    uint8_t* rec = burst + 4 * STAGE_DW;
    if (r < n) {
        const size_t b = r / cap, i = r - b * cap;
        bool live = true;
        if (counts) live = i < (size_t)counts[b];   // i < cap already
        if (live) {
            for (int k = 0; k < TX_REC; ++k) rec[k] = records[r * TX_REC + k];
            encode_record(rec, burst);
        }
    }
    __syncthreads();
    const size_t left = n - r0;   // r0 < n: the grid has ceil(n / 64) blocks
    store_wave(lds, lane, r0, left < 64 ? (unsigned)left : 64u, cap, out, out_stride, slot_bytes, dwords != 0);
}

__global__ __launch_bounds__(64) void k_dmr_tx_call(const uint8_t* __restrict__ calls, const uint8_t* __restrict__ voice, const uint32_t* __restrict__ first,
                                                    size_t batch, size_t cap, uint8_t* __restrict__ out, size_t out_stride, size_t slot_bytes, int dwords)
{
    __shared__ uint32_t lds[64 * LANE_DW];
    const unsigned lane = threadIdx.x;
    const size_t n = batch * cap, r0 = (size_t)blockIdx.x * 64, r = r0 + lane;
    uint8_t* burst = lane_burst(lds, lane);
    uint8_t* rec = burst + 4 * STAGE_DW;
    if (r < n) {
        const size_t b = r / cap, i = r - b * cap;
        uint8_t call[CALL_REC], v[27];
        for (int k = 0; k < CALL_REC; ++k) call[k] = calls[b * CALL_REC + k];
        for (int k = 0; k < 27; ++k) v[k] = voice[r * 27 + k];
        voice_call_record(call, (uint64_t)(first ? first[b] : 0u) + i, v, rec);
        encode_record(rec, burst);
    }
    __syncthreads();
    const size_t left = n - r0;
    store_wave(lds, lane, r0, left < 64 ? (unsigned)left : 64u, cap, out, out_stride, slot_bytes, dwords != 0);
}

static int dword_path(const uint8_t* out, size_t out_stride, size_t slot_bytes)
{
    return ((reinterpret_cast<uintptr_t>(out) | out_stride | slot_bytes) & 3u) == 0;
}

void launch_dmr_tx(const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap, uint8_t* out, size_t out_stride, size_t slot_bytes,
                   hipStream_t s)
{
    const size_t n = batch * cap;
    if (!n) return;
    hipLaunchKernelGGL(k_dmr_tx, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, records, counts, batch, cap, out, out_stride, slot_bytes,
                       dword_path(out, out_stride, slot_bytes));
}
void launch_dmr_tx_call(const uint8_t* calls, const uint8_t* voice, const uint32_t* first, size_t batch, size_t n_bursts, uint8_t* out,
                        size_t out_stride, size_t slot_bytes, hipStream_t s)
{
    const size_t n = batch * n_bursts;
    if (!n) return;
    hipLaunchKernelGGL(k_dmr_tx_call, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, calls, voice, first, batch, n_bursts, out, out_stride,
                       slot_bytes, dword_path(out, out_stride, slot_bytes));
}

}  // namespace qrl
