// test_decim_plan — the call-cut arithmetic of the decimating front end (qradiolink_amd/csrc/decim_plan.hpp) on the CPU.
// Reads lines from standard input:
//   class D nt   prints "class D nt NAME": the kernel class decim_choose gives the geometry (pm | pl | m16 | generic | none)
//   plan D nt    a pm or pl geometry: random streams from sample 0, cut into about 40 calls of even sizes (2 samples; up to 2 D; up to
//                80 D; up to 400 D; about (J + 16) D, the size of the edge region; up to 6000 D; and a mix of these), outputs of a call as
//                decim_count gives them, scratch of decim_*_edge_len.  Checked for every call with outputs:
//     ranges    gen_head, edge, main, gen_tail are in order, contiguous and cover [m0, m_end); gen_head and gen_tail are EMPTY
//     main      its oldest warm-up block (m_main - (J - 1) for pm, m_main - WU for pl) starts at or behind n0, block m_tail - 1 ends inside
//               the buffer, and for pm block m_main - (J - 1) opens a 16-block group
//     edge      edge_len even and <= the scratch; edge_i0 <= the first sample of the oldest block output m0 needs; the scratch reaches past
//               the last sample of block m_main - 1; and the stage never reads behind the carried history: n0 - edge_i0 <= the stage's
//               look-back when edge_i0 >= 0, n0 <= look-back otherwise
//     segments  (random batch, wave slots and, for pm, per-stream offsets or not) S a multiple of 16 and >= 16, nseg S >= the main count,
//               (nseg - 1) S < it without per-stream offsets, nseg a multiple of the waves per workgroup with them, S <= s_cap for pl
//   prints "plan D nt CONTRACT calls staged streamed": calls checked, calls with a staged edge, calls with a non-empty main range.
// Built with -fsanitize=address,undefined by tests/test_decim_plan_host.py.  Ends with "ok <calls>"; exit status 1 with the first violation.
#include "../../qradiolink_amd/csrc/decim_plan.hpp"
#include <cstdio>
#include <cstring>
#include <random>

using namespace qrl;

static std::mt19937 rng(20240919u);
static uint32_t upto(uint32_t n) { return (uint32_t)(rng() % (n + 1)); }   // 0 .. n

struct Call { int D, nt; uint64_t n0; uint32_t n; uint64_t m0, m_end; };
#define CHECK(cond) do { if (!(cond)) { std::printf("D %d nt %d call n0 %llu n %u outputs [%llu, %llu): %s is false\n", c.D, c.nt, \
    (unsigned long long)c.n0, c.n, (unsigned long long)c.m0, (unsigned long long)c.m_end, #cond); return false; } } while (0)

// warm: warm-up blocks in front of a segment (the streaming kernel reads blocks m - warm .. m for output m); look: the stage's look-back
static bool check_split(const Call& c, const DecimSplit& sp, int warm, uint32_t edge_cap, uint32_t look, bool pm)
{
    const int64_t D = c.D, n0 = (int64_t)c.n0, n_end = n0 + c.n;
    CHECK(sp.gen_head.lo == c.m0 && sp.gen_head.hi == sp.edge.lo && sp.edge.hi == sp.main.lo && sp.main.hi == sp.gen_tail.lo && sp.gen_tail.hi == c.m_end);
    CHECK(sp.gen_head.lo <= sp.gen_head.hi && sp.edge.lo <= sp.edge.hi && sp.main.lo <= sp.main.hi && sp.gen_tail.lo <= sp.gen_tail.hi);
    CHECK(sp.gen_head.empty() && sp.gen_tail.empty());
    if (!sp.main.empty()) {
        const int64_t c_old = (int64_t)sp.main.lo - warm;
        CHECK((c_old - 1) * D + 1 >= n0);                            // block c = samples (c - 1) D + 1 .. c D
        CHECK(((int64_t)sp.main.hi - 1) * D <= n_end - 1);
        if (pm) CHECK(c_old % 16 == 0);
    }
    if (!sp.edge.empty()) {
        CHECK(sp.edge_len % 2 == 0 && sp.edge_len <= edge_cap);
        CHECK(sp.edge_i0 <= ((int64_t)c.m0 - warm - 1) * D + 1);
        CHECK(sp.edge_i0 + (int64_t)sp.edge_len > ((int64_t)sp.edge.hi - 1) * D);
        if (sp.edge_i0 >= 0) CHECK(n0 - sp.edge_i0 <= (int64_t)look);
        else CHECK(n0 <= (int64_t)look);
    } else CHECK(sp.edge_len == 0);
    return true;
}
static bool check_segments(const Call& c, const DecimSegments& sg, uint64_t M, uint32_t batch, uint32_t mult, bool edge_unit, uint64_t s_cap)
{
    CHECK(sg.S % 16 == 0 && sg.S >= 16);
    CHECK((uint64_t)sg.nseg * sg.S >= M);
    if (mult == 1) CHECK(M == 0 ? sg.nseg == 0 : (uint64_t)(sg.nseg - 1) * sg.S < M);
    CHECK(sg.nseg % mult == 0);
    CHECK(sg.S <= s_cap);
    CHECK(sg.units == sg.nseg * batch + (edge_unit ? batch : 0u));
    return true;
}

static uint32_t call_size(int kind, int D, int J)
{
    switch (kind) {
    case 0: return 2;
    case 1: return 2 * (1 + upto((uint32_t)D - 1));
    case 2: return 2 * (1 + upto(40u * D - 1));
    case 3: return 2 * (1 + upto(200u * D - 1));
    case 4: return ((uint32_t)(J + 14) * D + upto(4u * D)) & ~1u;   // (J + 16) D -+ 2 D
    default: return 2 * (1 + upto(3000u * D - 1));
    }
}

static bool plan_geometry(int D, int nt, unsigned long long& total)
{
    const bool pm = decim_uses_pm(nt, D);
    if (!pm && !decim_uses_pl(nt, D)) { std::printf("plan %d %d: neither a pm nor a pl geometry\n", D, nt); return false; }
    const PlGeom g = pl_geom(nt, D);
    const int J = pm ? pm_kernel_lags(nt, D) : g.Upad, warm = pm ? J - 1 : g.WU;
    const uint32_t edge_cap = (uint32_t)(pm ? decim_pm_edge_len(nt, D) : decim_pl_edge_len(nt, D));
    const uint32_t look = pm ? decim_pm_lookback(nt, D) : decim_pl_lookback(nt, D);
    unsigned long long calls = 0, staged = 0, streamed = 0;
    for (int stream = 0; stream < 280; ++stream) {
        const int kind = stream % 7;   // 6: every call of its own kind
        const int ncalls = 30 + (int)upto(20);
        uint64_t n0 = 0;
        for (int k = 0; k < ncalls; ++k) {
            const uint32_t n = call_size(kind == 6 ? (int)upto(5) : kind, D, J);
            const Call c{D, nt, n0, n, decim_count(n0, 1, D), decim_count(n0 + n, 1, D)};
            n0 += n;
            if (c.m_end == c.m0) continue;   // (the launchers return at once)
            const DecimSplit sp = pm ? decim_pm_split(c.n0, c.n, c.m0, (uint32_t)(c.m_end - c.m0), nt, D, edge_cap, true)
                                     : decim_pl_split(c.n0, c.n, c.m0, (uint32_t)(c.m_end - c.m0), nt, D, edge_cap, true);
            if (!check_split(c, sp, warm, edge_cap, look, pm)) return false;
            const uint32_t batch = upto(3) ? 1 + upto(63) : 1 + upto(4999);
            const uint64_t M = sp.main.count();
            if (pm) {
                const uint32_t mult = upto(1) ? 4u : 1u, cap = 1024u * (1 + upto(3));   // 256 CUs x 1 .. 4 workgroups of four waves
                if (!check_segments(c, pm_segments(M, batch, cap, J, mult, !sp.edge.empty()), M, batch, mult, !sp.edge.empty(), ~0ull)) return false;
            } else if (!check_segments(c, pl_segments(M, batch, g, !sp.edge.empty()), M, batch, 1, !sp.edge.empty(), pl_segment_cap(g))) return false;
            ++calls; staged += !sp.edge.empty(); streamed += !sp.main.empty();
        }
    }
    std::printf("plan %d %d %s %llu %llu %llu\n", D, nt, pm ? "pm" : "pl", calls, staged, streamed);
    total += calls;
    return true;
}

int main()
{
    char what[16];
    int D, nt;
    unsigned long long total = 0;
    while (std::scanf("%15s %d %d", what, &D, &nt) == 3) {
        if (D < 1 || nt < 1) { std::printf("bad line: %s %d %d\n", what, D, nt); return 1; }
        if (!std::strcmp(what, "class")) {
            static const char* const names[] = {"pm", "pl", "m16", "generic", "none"};
            std::printf("class %d %d %s\n", D, nt, names[decim_choose(nt, D).cls]);
        } else if (!std::strcmp(what, "plan")) {
            if (!plan_geometry(D, nt, total)) return 1;
        } else { std::printf("bad line: %s %d %d\n", what, D, nt); return 1; }
    }
    std::printf("ok %llu\n", total);
    return 0;
}
