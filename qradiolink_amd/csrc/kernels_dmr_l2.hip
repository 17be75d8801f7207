// kernels_dmr_l2.hip — DMR layer 2 over the DMO slicer's mailbox (kernels_dmo.hip): what the reference does to every burst next,
// DMRFrame::DMRFrame / validate / runAudioFEC (src/DMR/dmrframe.cpp:36-253) and CDMREMB::putData (src/DMR/dmrcontrol.cpp:247).
//   k_dmr_l2           one lane per mailbox slot: everything of dmr_l2_core.hpp's decode_record except the rate 3/4 search; a rate 3/4
//                      burst whose first checkCode fails is left as a failed record with the mark SEARCH in its `valid` byte
//   k_dmr_l2_search    CDMRTrellis::fixCode (src/MMDVM/DMRTrellis.cpp:321-348) for the marked records: 16 lanes per burst, four bursts
//                      per wave; lane i tries candidate point i of a round, the 16 results are reduced inside the DPP row
//   k_trellis34_check / _search / _encode   the same pair, and CDMRTrellis::encode, on bare bursts (qrl_dmr_trellis34_*)
// The search has a launch of its own, so a burst that passes its first check never pays for it: its group of 16 lanes reads one byte and
// leaves.  Reduction rule of a round (the scalar loop's choices): key = pos << 4 | (15 - i), maximum over the row.  pos = 999 beats every
// position, so the lowest i that reaches 999 wins; otherwise the lowest i with the strictly greatest pos; and when no candidate gets past
// position 0 the winner is i = 0 with pos 0, which is the loop's bestVal = 0 / failPos = 0.
#include "engine.hpp"
#include "dmr_l2_core.hpp"

namespace qrl {

using namespace dmr;

constexpr uint8_t SEARCH = 0xFF;   // `valid` / `ok` byte of a burst that waits for k_*_search

__global__ __launch_bounds__(64) void k_dmr_l2(const uint8_t* __restrict__ records, const uint32_t* __restrict__ counts, size_t batch,
                                               size_t cap, int audio_fec, uint8_t* __restrict__ out)
{
    const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= batch * cap) return;
    const size_t b = r / cap, i = r - b * cap;
    uint8_t rec[REC_OUT];
    bool live = true;
    if (counts) live = i < (size_t)counts[b];   // i < cap already
    if (live) {
        uint8_t in[REC_IN];
        for (int k = 0; k < REC_IN; ++k) in[k] = records[r * REC_IN + k];
        if (!decode_record(in, audio_fec, rec, false)) rec[R_VALID] = SEARCH;
    } else {
        for (int k = 0; k < REC_OUT; ++k) rec[k] = 0;
    }
    uint8_t* dst = out + r * REC_OUT;
    for (int k = 0; k < REC_OUT; ++k) dst[k] = rec[k];
}

// maximum over the 16 lanes of a DPP row, in every lane of the row
__device__ __forceinline__ uint32_t row_max16(uint32_t v)
{
    uint32_t o;
    o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xf, 0xf, false); v = o > v ? o : v;    // quad_perm [1,0,3,2]
    o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xf, 0xf, false); v = o > v ? o : v;    // quad_perm [2,3,0,1]
    o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false); v = o > v ? o : v;   // row_half_mirror
    o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false); v = o > v ? o : v;   // row_mirror
    return v;
}

// CDMRTrellis::decode behind a failed first check, the 16 lanes of a row together (all of them call this, with the same burst).  Returns
// true in every lane on success; `payload` is written in the winning lane only, whose number (0..15) comes back in `winner`.
__device__ bool trellis_search16(const uint8_t* burst, unsigned lane, uint8_t* payload, unsigned& winner)
{
    Nib49 save, tri{};
    trellis_points(burst, save);
    const unsigned first = trellis_check(save, tri);   // not 999: the caller marked this burst
    for (unsigned go = 0; go < 2u; ++go) {
        if (go == 1u && first == 0u) break;
        Nib49 pts = save;                               // the second go starts from the saved points, one place back
        unsigned fail_pos = go == 0u ? first : first - 1u;
        for (unsigned j = 0; j < 20u; ++j) {
            Nib49 mine = pts;
            nib_set(mine, fail_pos, lane);
            const unsigned pos = trellis_check(mine, tri);
            const uint32_t key = row_max16((pos << 4) | (15u - lane));
            const unsigned best_pos = key >> 4, best_val = 15u - (key & 15u);
            if (best_pos == (unsigned)TRELLIS_OK) {
                winner = best_val;
                if (lane == best_val) trellis_payload(tri, payload);
                return true;
            }
            nib_set(pts, fail_pos, best_val);
            fail_pos = best_pos;
        }
    }
    return false;
}

__global__ __launch_bounds__(64) void k_dmr_l2_search(size_t n, uint8_t* __restrict__ out)
{
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 4);
    const unsigned lane = threadIdx.x & 15u;
    if (r >= n) return;
    uint8_t* rec = out + r * REC_OUT;
    if (rec[R_VALID] != SEARCH) return;     // the whole row leaves together
    uint8_t burst[BURST], payload[18];
    for (int k = 0; k < BURST; ++k) burst[k] = rec[R_BURST + k];
    for (int k = 0; k < 18; ++k) payload[k] = 0;
    unsigned winner = 0;
    const bool ok = trellis_search16(burst, lane, payload, winner);
    if (ok) {
        if (lane == winner) {
            trellis_encode(payload, burst);
            for (int k = 0; k < BURST; ++k) rec[R_BURST + k] = burst[k];
            for (int k = 0; k < 18; ++k) rec[R_PAYLOAD + k] = payload[k];
            rec[R_PLEN] = 18;
            rec[R_VALID] = 1;
        }
    } else if (lane == 0u) rec[R_VALID] = 0;
}

__global__ __launch_bounds__(64) void k_trellis34_check(const uint8_t* __restrict__ bursts, size_t n, uint8_t* __restrict__ payloads, uint8_t* __restrict__ ok)
{
    const size_t f = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t in[BURST], pay[18];
    for (int k = 0; k < BURST; ++k) in[k] = bursts[f * BURST + k];
    for (int k = 0; k < 18; ++k) pay[k] = 0;
    Nib49 pts, tri{};
    trellis_points(in, pts);
    const bool pass = trellis_check(pts, tri) == (unsigned)TRELLIS_OK;
    if (pass) trellis_payload(tri, pay);
    for (int k = 0; k < 18; ++k) payloads[f * 18 + k] = pay[k];
    ok[f] = pass ? 1 : SEARCH;
}

__global__ __launch_bounds__(64) void k_trellis34_search(const uint8_t* __restrict__ bursts, size_t n, uint8_t* __restrict__ payloads, uint8_t* __restrict__ ok)
{
    const size_t f = (size_t)blockIdx.x * 4 + (threadIdx.x >> 4);
    const unsigned lane = threadIdx.x & 15u;
    if (f >= n) return;
    if (ok[f] != SEARCH) return;
    uint8_t in[BURST], pay[18];
    for (int k = 0; k < BURST; ++k) in[k] = bursts[f * BURST + k];
    for (int k = 0; k < 18; ++k) pay[k] = 0;
    unsigned winner = 0;
    const bool found = trellis_search16(in, lane, pay, winner);
    if (found) {
        if (lane == winner) { for (int k = 0; k < 18; ++k) payloads[f * 18 + k] = pay[k]; ok[f] = 1; }
    } else if (lane == 0u) ok[f] = 0;
}

__global__ __launch_bounds__(64) void k_trellis34_encode(const uint8_t* __restrict__ payloads, size_t n, uint8_t* __restrict__ bursts)
{
    const size_t f = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    uint8_t pay[18], b[BURST];
    for (int k = 0; k < 18; ++k) pay[k] = payloads[f * 18 + k];
    for (int k = 0; k < BURST; ++k) b[k] = bursts[f * BURST + k];
    trellis_encode(pay, b);
    for (int k = 0; k < BURST; ++k) bursts[f * BURST + k] = b[k];
}

void launch_dmr_l2(const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap, int audio_fec, uint8_t* out, hipStream_t s)
{
    const size_t n = batch * cap;
    if (!n) return;
    hipLaunchKernelGGL(k_dmr_l2, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, records, counts, batch, cap, audio_fec, out);
    hipLaunchKernelGGL(k_dmr_l2_search, dim3((unsigned)((n + 3) / 4)), dim3(64), 0, s, n, out);
}
void launch_trellis34_decode(const uint8_t* bursts, size_t n, uint8_t* payloads, uint8_t* ok, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_trellis34_check, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, bursts, n, payloads, ok);
    hipLaunchKernelGGL(k_trellis34_search, dim3((unsigned)((n + 3) / 4)), dim3(64), 0, s, bursts, n, payloads, ok);
}
void launch_trellis34_encode(const uint8_t* payloads, size_t n, uint8_t* bursts, hipStream_t s)
{
    if (!n) return;
    hipLaunchKernelGGL(k_trellis34_encode, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, payloads, n, bursts);
}

}  // namespace qrl
