// kernels_dmr_sink.hip — the repeater-mode DMR burst sink on the device: gr_dmr_sink::work / processBits / findSync on the hard bits of port 2
// of gr_demod_dmr (dmr_sink_core.hpp; reference src/gr/gr_dmr_sink.cpp:79-260, src/DMR/dmrframe.cpp:58-80, :255-288, :370-384).
//   k_dmr_sink        one lane per stream, as k_dmo_sink: the block is bit-serial per stream (two slot contexts, a 48-bit sync search on the
//                     context the bits go to, then 108 or 288 bits collected), so parallelism comes from the batch; a workgroup is one wave
//                     of 64 streams.
//   k_dmr_sink_flush  gr_dmr_sink::flush on every stream: the two bit buffers emptied, the state machines left alone.
//
// Layout.  The streams lie `stride` bytes apart with one bit per byte, so a lane that walked its own row would touch a cache line of its
// own per load.  The wave fetches a tile of TILE = 128 bits of each of its 64 rows instead: lanes 0..31 take the 32 dwords of one row and
// lanes 32..63 those of the next, 32 coalesced loads a tile, held in registers and issued a tile ahead of the walk; they go to LDS as rows of
// ROW = 136 bytes, and the owning lane reads its row back as four 8-byte words per 32 bits (34 dwords a row: the 32 lanes of an LDS
// group fall on distinct bank pairs) and packs them, eight bits to a byte, into one 32-bit word for dmr_sink_core.hpp's sink_bits.  Where
// the bit pointer or the stride is no multiple of four the tile is fetched a byte per lane.
//
// Per-bit cost.  A searching context costs, per bit: the 64-bit shift, four 48-bit compares, the saturating count, and one move of five
// words in 32 bits.  A collecting context takes what is left of the 32-bit word, or of the burst, in one append; the 108 payload bits
// after a sync word and the 288 bits of a voice burst cost a handful of appends.  A burst is emitted as five 8-byte stores (frame record)
// and one 16-byte store (slot record).
//
// The work-entry trim of the reference (erase 288 bits once a buffer holds 864) is not run: dmr_sink_core.hpp's header says why it can
// never change a result; tests/test_gpu_dmr_sink.py feeds the same long sync-free run as one call and as many.
//
// Bounds: a lane reads bits[b * stride + i] for b < batch and i < min(n, counts[b * count_stride]) only; records are written for slots
// < cap only, the count goes on (out_counts[b] > cap: bursts were dropped).  Vector loads and stores only, no atomics.
#include "engine.hpp"
#include "dmr_sink_core.hpp"

namespace qrl {

using namespace dmr_sink;

static_assert(STATE_BYTES == DMR_SINK_STATE_BYTES && STATE_BYTES % 16 == 0, "engine.hpp and dmr_sink_core.hpp agree; the state moves as 16-byte words");

namespace {
constexpr int TILE = 128, ROW = 136, WAVE = 64;

__device__ inline uint32_t pack4(uint32_t w) { return ((w & 0x01010101u) * 0x08040201u) >> 24; }   // four bit-bytes, the first lowest -> a nibble, the first bit highest
__device__ inline uint32_t pack8(uint64_t x) { return ((pack4((uint32_t)x) & 0xFu) << 4) | (pack4((uint32_t)(x >> 32)) & 0xFu); }
}  // namespace

__global__ __launch_bounds__(64) void k_dmr_sink(const DmrSinkParams P, int batch)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[WAVE * ROW];
    const int lane = threadIdx.x, b0 = blockIdx.x * WAVE, b = b0 + lane;
    const bool live = b < batch;
    uint32_t cnt = 0;
    if (live) { cnt = P.counts ? P.counts[(size_t)b * P.count_stride] : P.n; if (cnt > P.n) cnt = P.n; }
    uint32_t longest = cnt;
    for (int m = 32; m; m >>= 1) { const uint32_t o = __shfl_xor(longest, m, WAVE); longest = o > longest ? o : longest; }

    dmr_sink_state* sp = static_cast<dmr_sink_state*>(P.st) + (live ? b : 0);
    dmr_sink_run run;
    {
        dmr_sink_state st;
        uint32_t w[STATE_BYTES / 4];
        const uint4* src = reinterpret_cast<const uint4*>(sp);
        for (int k = 0; k < (int)STATE_BYTES / 16; ++k) { const uint4 v = src[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
        __builtin_memcpy(&st, w, STATE_BYTES);
        run_load(run, st);
    }
    uint32_t nout = 0;
    uint8_t* frames = P.frames + (size_t)(live ? b : 0) * P.cap * FRAME_REC;
    uint8_t* info = P.info + (size_t)(live ? b : 0) * P.cap * INFO_REC;
    auto emit = [&](const uint32_t* f, const uint32_t* s) {
        if (nout < P.cap) {
            uint2* fd = reinterpret_cast<uint2*>(frames + (size_t)nout * FRAME_REC);
#pragma unroll
            for (int k = 0; k < FRAME_REC / 8; ++k) fd[k] = make_uint2(f[2 * k], f[2 * k + 1]);
            *reinterpret_cast<uint4*>(info + (size_t)nout * INFO_REC) = make_uint4(s[0], s[1], s[2], s[3]);
        }
        ++nout;
    };

    const bool wide = ((reinterpret_cast<uintptr_t>(P.bits) | P.stride) & 3u) == 0;
    const int half = lane >> 5, word = lane & 31;
    // the dwords of tile t that this lane fetches: row 2 j + half of the wave, bytes t TILE + 4 word ..; a dword that reaches past the row's
    // bits is read by bytes, so nothing behind bits[b * stride + min(n, count)] is touched
    auto fetch = [&](uint32_t t, uint32_t* pre) {
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const int row = 2 * j + half;
            const uint32_t lim = __shfl(cnt, row, WAVE), off = t * TILE + 4u * word;
            uint32_t v = 0;
            if (off < lim) {
                const uint8_t* p = P.bits + (size_t)(b0 + row) * P.stride + off;
                if (off + 4u <= lim) v = *reinterpret_cast<const uint32_t*>(p);
                else for (uint32_t m = 0; off + m < lim; ++m) v |= (uint32_t)p[m] << (8u * m);
            }
            pre[j] = v;
        }
    };
    uint32_t pre[32];
    const uint32_t tiles = (longest + TILE - 1) / TILE;
    if (wide && tiles) fetch(0, pre);
    for (uint32_t t = 0; t < tiles; ++t) {
        if (wide) {
#pragma unroll
            for (int j = 0; j < 32; ++j) *reinterpret_cast<uint32_t*>(tile + (2 * j + half) * ROW + 4 * word) = pre[j];
        } else {
            for (int j = 0; j < 2 * WAVE; ++j) {
                const int row = j >> 1;
                const uint32_t lim = __shfl(cnt, row, WAVE), off = t * TILE + (uint32_t)(j & 1) * WAVE + lane;
                tile[row * ROW + (j & 1) * WAVE + lane] = off < lim ? P.bits[(size_t)(b0 + row) * P.stride + off] : (uint8_t)0;
            }
        }
        __syncthreads();
        if (wide && t + 1 < tiles) fetch(t + 1, pre);
        const uint32_t base = t * TILE;
        const uint64_t* mine = reinterpret_cast<const uint64_t*>(tile + lane * ROW);
#pragma unroll 1
        for (int g = 0; g < TILE / 32; ++g) {
            const uint32_t at = base + 32u * g;
            if (at < cnt) {
                const uint32_t left = cnt - at, nbits = left < 32u ? left : 32u;
                const uint32_t w = (pack8(mine[4 * g]) << 24) | (pack8(mine[4 * g + 1]) << 16) | (pack8(mine[4 * g + 2]) << 8) | pack8(mine[4 * g + 3]);
                sink_bits(run, w, nbits, emit);
            }
        }
        __syncthreads();
    }
    if (!live) return;
    {
        dmr_sink_state st;
        run_store(run, st);
        uint32_t w[STATE_BYTES / 4];
        __builtin_memcpy(w, &st, STATE_BYTES);
        uint4* dst = reinterpret_cast<uint4*>(sp);
        for (int k = 0; k < (int)STATE_BYTES / 16; ++k) dst[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    P.out_counts[b] = nout;   // bursts FOUND by the call; records beyond cap are not written
}

__global__ __launch_bounds__(64) void k_dmr_sink_flush(dmr_sink_state* __restrict__ states, int batch)
{
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if (b >= batch) return;
    for (int c = 0; c < 2; ++c) {
        for (int w = 0; w < 9; ++w) states[b].c[c].buf[w] = 0;
        states[b].c[c].size = 0;
    }
}

void launch_dmr_sink(const DmrSinkParams& p, int batch, hipStream_t s)
{
    if (batch < 1) return;
    hipLaunchKernelGGL(k_dmr_sink, dim3((unsigned)((batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, p, batch);
}
void launch_dmr_sink_flush(void* states, int batch, hipStream_t s)
{
    if (batch < 1) return;
    hipLaunchKernelGGL(k_dmr_sink_flush, dim3((unsigned)((batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, static_cast<dmr_sink_state*>(states), batch);
}

}  // namespace qrl
