// What k_decim_pm relies on when the caller's buffer holds 8-bit pairs (2 bytes per sample), evaluated on the CPU: a stand-alone program over
// qradiolink_amd/csrc/decim_plan.hpp (no HIP), built by tests/test_iq8_plan_host.py with the address and undefined-behaviour sanitizers.
// For every front-end geometry D in {9, 18, 25, 27, 50, 98, 100} (41.8 D taps, three lag tiles) and a set of calls -- n over multiples of 8 and
// n % 8 in {2, 4, 6}, row pitches that are and are not multiples of 8 samples, bases on and off a 16-byte boundary, at several stream positions --
// it checks that
//   * decim_pm_streamable says what the rule says: base 16-byte aligned, pitch a multiple of 8 samples, n % 8 == 0 (and the rotator and an aligned
//     edge scratch); a call that is not streamable gets no main and no edge range (decim_pm_plan_call, what launch_decim_pm calls);
//   * for streamable calls, per segment of pm_segments, with the kernel's own arithmetic: the segment starts on the absolute 16-block grid, its
//     oldest block lies in the buffer and its newest block ends inside it; the first 16-byte piece of every 1 KiB DMA piece is 16-byte aligned
//     inside the row; and the last byte ANY lane may fetch -- pieces inside the row whole, later ones clamped to the row's last 16 bytes -- lies
//     inside row + row_bytes, as does the last byte a lane reads from the ring for an output it stores.
// Prints "ok <calls> <streamable> <segments>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../qradiolink_amd/csrc/decim_plan.hpp"

using namespace qrl;

static int fails = 0;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s (D %d n %u pitch %u base %u n0 %" PRIu64 ")\n", __LINE__, #c, D, n, pitch, base16, n0); if (++fails > 20) std::exit(1); } } while (0)

int main()
{
    const int Ds[] = {9, 18, 25, 27, 50, 98, 100};
    const uint32_t cap = 256 * 4 * 4;                      // wave slots of the chip as the launcher would count them (any value gives a valid split)
    const uint32_t batch = 3;
    const int RPs[] = {8, 8, 8, 8, 8, 16, 16};             // ring pieces per wave of the instantiations (launch_decim_pm)
    long calls = 0, streamable = 0, segments = 0;
    for (int di = 0; di < 7; ++di) {
        const int D = Ds[di];
        const int nt = (int)(41.8 * D) | 1;                // the front-end filters have 41.8 D taps
        if (!decim_uses_pm(nt, D) || pm_tiles(pm_kernel_lags(nt, D)) != 3) { std::fprintf(stderr, "D %d is no three-tile pm geometry\n", D); return 1; }
        const int J = pm_kernel_lags(nt, D);
        const uint32_t edge_cap = (uint32_t)decim_pm_edge_len(nt, D);
        const uint32_t lens[] = {8, 16, 8u * (uint32_t)D, 64u * (uint32_t)D + 8, 200u * (uint32_t)D, 1000u * (uint32_t)D + 16, 5000u * (uint32_t)D + 24,
                                 2, 4, 6, ((58u * (uint32_t)D) & ~7u) + 2, ((700u * (uint32_t)D) & ~7u) + 4, ((5000u * (uint32_t)D) & ~7u) + 6, ((10u * (uint32_t)D) & ~7u) + 2};
        const uint64_t starts[] = {0, 8, 5000ull * D + 24, 123456ull * 8, (1ull << 33) + 40};
        for (uint64_t n0 : starts)
            for (uint32_t n : lens)
                for (uint32_t extra : {0u, 8u, 4u, 2u, 1u})          // pitch = n rounded up to 8 + extra
                    for (uint32_t base16 : {0u, 8u, 2u}) {
                        const uint32_t pitch = (n + 7) / 8 * 8 + extra;
                        const uint64_t m0 = decim_count(n0, 1, D), m1 = decim_count(n0 + n, 1, D);
                        const uint32_t m_count = (uint32_t)(m1 - m0);
                        const uint64_t row = 0x7f0000000000ull + base16;
                        CallInput ci{row, pitch, n, false, true, 0x7e0000000000ull, edge_cap};
                        ci.iq8 = true;
                        ++calls;
                        const bool want = base16 == 0 && pitch % 8 == 0 && n % 8 == 0;
                        const bool ok = decim_pm_streamable(ci);
                        REQUIRE(ok == want);
                        REQUIRE(pm_piece_mask(false, true) == 7u && in_sample_shift(false, true) == 1u);
                        const DecimSplit sp = decim_pm_plan_call(n0, m0, m_count, nt, D, edge_cap, ci);
                        REQUIRE(sp.gen_head.lo == m0 && sp.gen_tail.hi == m1);
                        REQUIRE(sp.gen_head.hi == sp.edge.lo && (sp.edge.empty() || sp.edge.hi == sp.main.lo) && sp.main.hi == sp.gen_tail.lo);
                        REQUIRE(sp.gen_head.count() + sp.edge.count() + sp.main.count() + sp.gen_tail.count() == m_count);
                        if (!ok) { REQUIRE(sp.main.empty() && sp.edge.empty()); continue; }
                        ++streamable;
                        if (!sp.edge.empty()) REQUIRE(sp.edge_len <= edge_cap && (sp.edge_len & 1u) == 0);
                        if (sp.main.empty()) continue;
                        const uint64_t row_bytes = (uint64_t)n << 1;
                        REQUIRE((row_bytes & 15u) == 0 && (((uint64_t)pitch << 1) & 15u) == 0 && (row & 15u) == 0);
                        const DecimSegments sg = pm_segments(sp.main.count(), batch, cap, J, 1, !sp.edge.empty());
                        REQUIRE(sg.S % 16 == 0 && (uint64_t)sg.S * sg.nseg >= sp.main.count());
                        const uint32_t RP = (uint32_t)RPs[di];
                        for (uint32_t seg = 0; seg < sg.nseg; ++seg) {      // the kernel's own arithmetic for unit (stream, seg), ssh = 1
                            const uint64_t ms = sp.main.lo + (uint64_t)seg * sg.S;
                            if (ms >= sp.main.hi) break;
                            ++segments;
                            const uint64_t me = std::min<uint64_t>(ms + sg.S, sp.main.hi);
                            const int64_t cfs = (int64_t)ms - (J - 1);
                            REQUIRE(cfs >= 0 && cfs % 16 == 0);
                            const int64_t G0 = cfs / 16;
                            const int ngrp = (int)((int64_t)((me - 1) / 16) - G0) + 1;
                            const int64_t i_first = (G0 * 16 - 1) * (int64_t)D + 1;
                            REQUIRE(i_first >= (int64_t)n0);
                            REQUIRE((me - 1) * (uint64_t)D <= n0 + n - 1);
                            const uint64_t off0 = (uint64_t)(i_first - (int64_t)n0) << 1;
                            const uint32_t o0 = (uint32_t)(off0 & 127u);
                            const uint64_t a_off = off0 - o0;
                            REQUIRE(a_off <= row_bytes && ((row + a_off) & 15u) == 0);        // every segment's first piece is 16-byte aligned inside the row
                            const uint32_t GB = (16u * (uint32_t)D) << 1;
                            REQUIRE(GB + 1024u <= RP * 1024u);                                 // a group and a piece of slack fit the wave's ring
                            const uint32_t npieces = (o0 + (uint32_t)ngrp * GB + 1023u) >> 10;
                            const uint32_t q_safe = (uint32_t)((row_bytes - a_off) >> 10);
                            // the last byte any lane may fetch: lane 63 of the last unclamped piece, or the clamp address + 15
                            uint64_t last = 0;
                            for (uint32_t piece = 0; piece < npieces; ++piece) {
                                const uint64_t gp63 = a_off + (uint64_t)piece * 1024 + 63 * 16;
                                const uint64_t at = piece < q_safe ? gp63 : std::min<uint64_t>(gp63, row_bytes - 16);
                                last = std::max(last, at + 15);
                            }
                            REQUIRE(last < row_bytes);
                            // the bytes of the ring a stored output depends on were fetched from inside the row: the last sample of the newest block of
                            // output me - 1 ends at stream byte 2 (me - 1) D + 1 relative to sample 1
                            const uint64_t last_needed = ((me - 1) * (uint64_t)D - n0) * 2 + 1;     // sample index (me - 1) D, 0-based row offset of its second byte
                            REQUIRE(last_needed < row_bytes);
                        }
                    }
    }
    if (fails) return 1;
    std::printf("ok %ld %ld %ld\n", calls, streamable, segments);
    return 0;
}
