// Which route the outputs of a 1 Msps handle's phase-major first stage take when the stream is cut as tests/sc16_baseband.py cuts it:
// a stand-alone program over qradiolink_amd/csrc/decim_plan.hpp (no HIP), built by tests/test_sc16_baseband_plan.py with the address and
// undefined-behaviour sanitizers.
//   stdin:  "stage <D> <nt> <batch> <cap>"                      the stage, the batch and the wave slots of the chip (pm_segments)
//           "call <n> <sc16 0|1> <pitch> <base_mod_16>"         one call each, in stream order: samples, format, row pitch in samples,
//                                                               the byte address of the call's first sample modulo 16
//   stdout: per call  "call <k> <n> <sc16> <streamable> <gen> <edge> <main> <S> <nseg> <turns x 100>"
//           then      "total <sc16 outputs> <gen> <edge> <main>" (int16 calls only) and "ok <calls>"
// For every call it evaluates the launcher's own rule (decim_pm_plan_call = decim_pm_streamable -> decim_pm_split, then pm_segments) and checks what the streaming
// kernel relies on for a buffer of 4-byte (or 8-byte) samples: the four ranges tile the call's outputs in order; every segment's oldest
// block lies in the buffer and its newest block ends inside it, so the bytes a stored output depends on are bytes of the row; a row is whole
// 16-byte pieces; the edge unit fits the scratch.
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
        uint32_t n = 0, pitch = 0, base16 = 0; int sc16 = 0;
        REQUIRE(static_cast<bool>(ss >> n >> sc16 >> pitch >> base16));
        const int J = pm_kernel_lags(nt, D);
        const uint32_t edge_cap = (uint32_t)decim_pm_edge_len(nt, D);
        const uint64_t m1 = decim_count(n0 + n, 1, D);
        const uint32_t m_count = (uint32_t)(m1 - m0);
        // the addresses only matter modulo 16: a 16-byte aligned allocation plus what Python reports for the call's first sample
        const CallInput ci{0x7f0000000000ull + base16, pitch, n, sc16 != 0, true, 0x7e0000000000ull, edge_cap};
        const bool ok = decim_pm_streamable(ci);
        const DecimSplit sp = decim_pm_plan_call(n0, m0, m_count, nt, D, edge_cap, ci);   // what launch_decim_pm calls
        // the ranges tile [m0, m1) in order
        REQUIRE(sp.gen_head.lo == m0 && sp.gen_tail.hi == m1);
        REQUIRE(sp.gen_head.hi == sp.edge.lo && (sp.edge.empty() || sp.edge.hi == sp.main.lo) && sp.main.hi == sp.gen_tail.lo);
        REQUIRE(sp.gen_head.count() + sp.edge.count() + sp.main.count() + sp.gen_tail.count() == m_count);
        if (!ok) REQUIRE(sp.main.empty() && sp.edge.empty());
        if (!sp.edge.empty()) REQUIRE(sp.edge_len <= edge_cap && (sp.edge_len & 1u) == 0);
        DecimSegments sg{0, 0, 0};
        unsigned turns100 = 0;
        if (!sp.main.empty()) {
            const unsigned ssh = sc16 ? 2 : 3;
            REQUIRE((((uint64_t)n << ssh) & 15u) == 0 && (((uint64_t)pitch << ssh) & 15u) == 0);   // rows are whole 16-byte pieces
            sg = pm_segments(sp.main.count(), batch, cap, J, 1, !sp.edge.empty());
            REQUIRE(sg.S % 16 == 0 && (uint64_t)sg.S * sg.nseg >= sp.main.count());
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
                REQUIRE(((off0 - (off0 & 127u)) & 15u) == 0);                             // piece 0 starts on a whole piece
            }
            turns100 = (unsigned)(100ull * ((uint64_t)(sg.S + J - 1 + 15) * D << ssh) / 8192u);
        }
        std::printf("call %d %u %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u\n", ncalls, n, sc16, ok ? 1 : 0,
                    sp.gen_head.count() + sp.gen_tail.count(), sp.edge.count(), sp.main.count(), sg.S, sg.nseg, turns100);
        if (sc16) { tot += m_count; tot_gen += sp.gen_head.count() + sp.gen_tail.count(); tot_edge += sp.edge.count(); tot_main += sp.main.count(); }
        n0 += n; m0 = m1;
        ++ncalls;
    }
    std::printf("total %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot, tot_gen, tot_edge, tot_main);
    std::printf("ok %d\n", ncalls);
    return 0;
}
