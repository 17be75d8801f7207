// Which route the outputs of a 1 Msps handle's phase-major first stage take when the stream is cut as tests/iq8_baseband.py cuts it and fed
// 8-bit pairs: a stand-alone program over qradiolink_amd/csrc/decim_plan.hpp (no HIP), built by tests/test_iq8_baseband_plan.py with the
// address and undefined-behaviour sanitizers.
//   stdin:  "stage <D> <nt> <batch> <cap>"                      the stage, the batch and the wave slots of the chip (pm_segments)
//           "call <n> <fmt> <pitch> <base_mod_16>"              one call each, in stream order: samples, format (0 cf32, 1 int16, 2 8-bit pairs),
//                                                               row pitch in samples, the byte address of the call's first sample modulo 16
//   stdout: per call  "call <k> <n> <fmt> <streamable> <gen> <edge> <main> <S> <nseg> <turns x 100> <pieces per group>"
//           then      "total <8-bit outputs> <gen> <edge> <main>" (8-bit calls only) and "ok <calls>"
// For every call it evaluates the launcher's own rule (decim_pm_plan_call with CallInput::iq8 set for the 8-bit calls, then pm_segments) and
// checks what the streaming kernel relies on for a buffer of 2-byte samples: the four ranges tile the call's outputs in order; every segment's
// oldest block lies in the buffer and its newest block ends inside it; a row is whole 16-byte pieces; the edge unit fits the scratch; and the
// ring arithmetic of the one-tile case -- a group of 16 D samples (1600 bytes at D = 50) with the piece its first byte lies in, the pieces the
// next group's prefetch may have landed and the reach of the last matrix step past the group all fit the wave's ring of 8 KiB.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../qradiolink_amd/csrc/decim_plan.hpp"

using namespace qrl;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s (call %d)\n", __LINE__, #c, ncalls); return 1; } } while (0)

int main()
{
    constexpr uint32_t RING = 8u * 1024u;   // RP = 8 pieces of 1 KiB per wave (QRL_PM_RP)
    int D = 0, nt = 0, ncalls = 0;
    uint32_t batch = 0, cap = 0;
    uint64_t n0 = 0, m0 = 0;
    uint64_t tot = 0, tot_gen = 0, tot_edge = 0, tot_main = 0;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string what;
        if (!(ss >> what)) continue;
        if (what == "stage") {
            REQUIRE(static_cast<bool>(ss >> D >> nt >> batch >> cap));
            REQUIRE(decim_uses_pm(nt, D) && pm_tiles(pm_kernel_lags(nt, D)) == 1);   // a ONE-tile geometry: what this file is about
            continue;
        }
        REQUIRE(what == "call" && D > 0);
        uint32_t n = 0, pitch = 0, base16 = 0; int fmt = 0;
        REQUIRE(static_cast<bool>(ss >> n >> fmt >> pitch >> base16));
        REQUIRE(fmt >= 0 && fmt <= 2);
        const bool sc16 = fmt == 1, iq8 = fmt == 2;
        const int J = pm_kernel_lags(nt, D);
        const uint32_t edge_cap = (uint32_t)decim_pm_edge_len(nt, D);
        const uint64_t m1 = decim_count(n0 + n, 1, D);
        const uint32_t m_count = (uint32_t)(m1 - m0);
        // the addresses only matter modulo 16: a 16-byte aligned allocation plus what Python reports for the call's first sample
        const CallInput ci{0x7f0000000000ull + base16, pitch, n, sc16, true, 0x7e0000000000ull, edge_cap, iq8};
        const bool ok = decim_pm_streamable(ci);
        const unsigned ssh = in_sample_shift(sc16, iq8);
        REQUIRE(ssh == (iq8 ? 1u : sc16 ? 2u : 3u) && pm_piece_mask(sc16, iq8) == (16u >> ssh) - 1u);
        if (iq8) REQUIRE(ok == (base16 == 0 && pitch % 8 == 0 && n % 8 == 0));         // whole 16-byte pieces of 2-byte samples
        const DecimSplit sp = decim_pm_plan_call(n0, m0, m_count, nt, D, edge_cap, ci);   // what launch_decim_pm calls
        // the ranges tile [m0, m1) in order
        REQUIRE(sp.gen_head.lo == m0 && sp.gen_tail.hi == m1);
        REQUIRE(sp.gen_head.hi == sp.edge.lo && (sp.edge.empty() || sp.edge.hi == sp.main.lo) && sp.main.hi == sp.gen_tail.lo);
        REQUIRE(sp.gen_head.count() + sp.edge.count() + sp.main.count() + sp.gen_tail.count() == m_count);
        if (!ok) REQUIRE(sp.main.empty() && sp.edge.empty());
        if (!sp.edge.empty()) REQUIRE(sp.edge_len <= edge_cap && (sp.edge_len & 1u) == 0);
        DecimSegments sg{0, 0, 0};
        unsigned turns100 = 0, pieces = 0;
        if (!sp.main.empty()) {
            REQUIRE((((uint64_t)n << ssh) & 15u) == 0 && (((uint64_t)pitch << ssh) & 15u) == 0);   // rows are whole 16-byte pieces
            sg = pm_segments(sp.main.count(), batch, cap, J, 1, !sp.edge.empty());
            REQUIRE(sg.S % 16 == 0 && (uint64_t)sg.S * sg.nseg >= sp.main.count());
            const uint32_t GB = (16u * (uint32_t)D) << ssh;                                  // bytes per group, the kernel's GB
            const uint32_t NS = ((uint32_t)D + 3u) / 4u;
            for (uint32_t seg = 0; seg < sg.nseg; ++seg) {   // the kernel's own arithmetic for unit (stream, seg)
                const uint64_t ms = sp.main.lo + (uint64_t)seg * sg.S;
                if (ms >= sp.main.hi) break;
                const uint64_t me = std::min<uint64_t>(ms + sg.S, sp.main.hi);
                const int64_t cfs = (int64_t)ms - (J - 1);
                REQUIRE(cfs >= 0 && cfs % 16 == 0);                                       // segments start on the absolute 16-block grid
                const int64_t i_first = (cfs - 1) * (int64_t)D + 1;                      // first sample of the oldest block
                REQUIRE(i_first >= (int64_t)n0);                                          // ... lies in this call's buffer
                REQUIRE((me - 1) * (uint64_t)D <= n0 + n - 1);                            // the newest block of the last output ends inside it
                const uint64_t off0 = (uint64_t)(i_first - (int64_t)n0) << ssh;           // byte offset of the segment in the row
                const uint32_t o0 = (uint32_t)(off0 & 127u);
                REQUIRE(((off0 - o0) & 15u) == 0 && (o0 & ((1u << ssh) - 1u)) == 0);      // piece 0 starts on a whole piece, samples on their own size
                // the ring: while group g is read, the pieces from the one its first byte lies in up to the last one the prefetch of the groups
                // behind it may have issued (first piece of group g + RP) are distinct slots, and the lane that reaches furthest -- block 15,
                // step NS - 1, lane row 3 -- reads inside them
                const int ngrp = (int)((int64_t)((me - 1) / 16) - cfs / 16) + 1;
                for (int g = 0; g < ngrp; g += std::max(1, ngrp - 1)) {                   // first and last group: gbytes only grows by GB
                    const uint64_t gbytes = o0 + (uint64_t)g * GB;
                    const uint64_t first_piece = gbytes >> 10, need = (gbytes + GB + 1023u) >> 10;
                    REQUIRE(need - first_piece <= RING / 1024u);                          // the group fits the ring beside nothing else
                    const uint64_t reach = gbytes + ((uint64_t)(15u * (uint32_t)D + 3u + 4u * (NS - 1u)) << ssh) + (1u << ssh);
                    REQUIRE(reach <= (first_piece << 10) + RING);                         // reads past the group stay in the ring's window
                    pieces = std::max<unsigned>(pieces, (unsigned)(need - first_piece));
                }
            }
            turns100 = (unsigned)(100ull * ((uint64_t)(sg.S + J - 1 + 15) * D << ssh) / RING);
        }
        std::printf("call %d %u %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u\n", ncalls, n, fmt, ok ? 1 : 0,
                    sp.gen_head.count() + sp.gen_tail.count(), sp.edge.count(), sp.main.count(), sg.S, sg.nseg, turns100, pieces);
        if (iq8) { tot += m_count; tot_gen += sp.gen_head.count() + sp.gen_tail.count(); tot_edge += sp.edge.count(); tot_main += sp.main.count(); }
        n0 += n; m0 = m1;
        ++ncalls;
    }
    std::printf("total %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot, tot_gen, tot_edge, tot_main);
    std::printf("ok %d\n", ncalls);
    return 0;
}
