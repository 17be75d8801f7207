// kernels_dmr_rx.hip — the DMR receive call layer behind k_dmr_l2: per stream, what DMRControl::addFrames does with the validated bursts of a
// call (dmr_rx_core.hpp; reference src/DMR/dmrcontrol.cpp:225-665, src/MMDVM/DMREmbeddedData.cpp:47-109, :213-322).
//   k_dmr_rx   one lane per stream, as k_dmo_sink: the lane loads its 128-byte state once (eight 16-byte loads), walks its mailbox slots
//              i < min(counts[b], cap) in order through dmr_rx_step, writes one 128-byte record per slot (eight 16-byte stores; zeros for the
//              slots behind the count) and stores the state once.  With slot records (qrl_dmr_rx_process_slots: the bursts of the repeater-mode
//              sink) a step also reads the two bytes of its 16-byte slot record that the CACH and timeslot rules ask for.
// The order of a stream's bursts is the protocol, so there is no parallelism inside a stream; a wave is 64 streams.  The state and the
// record a step builds stay in registers: every index into them is a constant once the loops are unrolled (the embedded matrix is four
// words and its transpose eight, the alias buffer 17 words appended to by comparison).  Of the 80 input bytes a step reads the ten it needs.
// Vector loads and stores only, no atomics, no LDS.
#include "engine.hpp"
#include "dmr_rx_core.hpp"

namespace qrl {

using namespace dmr;

static_assert(DMR_RX_REC == DMR_RX_RECORD_BYTES && DMR_RX_STATE_SIZE == DMR_RX_STATE_BYTES && DMR_RX_STATE_PUBLIC == DMR_RX_PUBLIC_BYTES,
              "engine.hpp and dmr_rx_core.hpp agree");
static_assert(DMR_RX_STATE_SIZE % 16 == 0 && DMR_RX_REC % 16 == 0, "the state and the record move as 16-byte words");

__global__ __launch_bounds__(64) void k_dmr_rx(const uint8_t* __restrict__ l2, const uint32_t* __restrict__ counts, size_t batch, size_t cap,
                                               int color_code, int promiscuous, dmr_rx_state* __restrict__ states, uint8_t* __restrict__ out,
                                               const uint8_t* __restrict__ slot_info, int repeater, int timeslot)
{
    const size_t b = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const dmr_rx_config cfg = {color_code, promiscuous, repeater, timeslot};
    dmr_rx_state st;
    uint32_t w[DMR_RX_STATE_SIZE / 4];
    uint4* sp = reinterpret_cast<uint4*>(states + b);
    for (int k = 0; k < DMR_RX_STATE_SIZE / 16; ++k) { const uint4 v = sp[k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
    __builtin_memcpy(&st, w, DMR_RX_STATE_SIZE);
    size_t n = cap;
    if (counts) { const size_t c = counts[b]; n = c < cap ? c : cap; }
    const uint8_t* rec = l2 + b * cap * REC_OUT;
    uint4* dst = reinterpret_cast<uint4*>(out + b * cap * DMR_RX_REC);
    const uint8_t* slot = slot_info ? slot_info + b * cap * SLOT_REC : nullptr;
    for (size_t i = 0; i < cap; ++i, rec += REC_OUT, dst += DMR_RX_REC / 16) {
        uint32_t r[DMR_RX_REC / 4];
        if (i < n) dmr_rx_step_slots(cfg, st, rec, slot ? slot + i * SLOT_REC : nullptr, r);
        else for (int k = 0; k < DMR_RX_REC / 4; ++k) r[k] = 0;
        for (int k = 0; k < DMR_RX_REC / 16; ++k) dst[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    }
    __builtin_memcpy(w, &st, DMR_RX_STATE_SIZE);
    for (int k = 0; k < DMR_RX_STATE_SIZE / 16; ++k) sp[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// the public first DMR_RX_STATE_PUBLIC bytes of every state, three dwords per stream
__global__ __launch_bounds__(64) void k_dmr_rx_state(const dmr_rx_state* __restrict__ states, size_t batch, uint32_t* __restrict__ out)
{
    const size_t u = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (u >= batch * (DMR_RX_STATE_PUBLIC / 4)) return;
    const size_t b = u / (DMR_RX_STATE_PUBLIC / 4), w = u - b * (DMR_RX_STATE_PUBLIC / 4);
    out[u] = reinterpret_cast<const uint32_t*>(states + b)[w];
}

void launch_dmr_rx(const uint8_t* l2, const uint32_t* counts, size_t batch, size_t cap, int color_code, int promiscuous, void* states, uint8_t* out,
                   hipStream_t s, const uint8_t* slot_info, int repeater, int timeslot)
{
    if (!batch || !cap) return;
    hipLaunchKernelGGL(k_dmr_rx, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, l2, counts, batch, cap, color_code, promiscuous,
                       static_cast<dmr_rx_state*>(states), out, slot_info, repeater, timeslot);
}
void launch_dmr_rx_state(const void* states, size_t batch, uint8_t* out, hipStream_t s)
{
    if (!batch) return;
    const size_t n = batch * (DMR_RX_STATE_PUBLIC / 4);
    hipLaunchKernelGGL(k_dmr_rx_state, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, static_cast<const dmr_rx_state*>(states), batch,
                       reinterpret_cast<uint32_t*>(out));
}

}  // namespace qrl
