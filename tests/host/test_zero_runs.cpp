// test_zero_runs — the bookkeeping of the gr_zero_idle_bursts run list (qradiolink_amd/csrc/zero_runs.hpp) against the block's rule, on the CPU.
// Random cases: 1-3 rows, up to 12 tags per row with distinct starts, added in random order, then [0, N) cut into random calls.
//   rule      item t of a row is zeroed iff some tag i of the row has s_i <= t < s_i + c_i and no tag j of it has s_i < s_j <= t
//             (one counter per stream, loaded by every tag: gr_zero_idle_bursts.cpp:62-69)
//   checked   the union of split()'s live runs, each clipped to its call, equals the rule for every item of [0, N); after the last call the
//             list holds only runs that reach past N.
// Built with -fsanitize=address,undefined by tests/test_zero_runs_host.py.  Prints "ok <cases>"; exit status 1 with the first mismatch otherwise.
#include "../../qradiolink_amd/csrc/zero_runs.hpp"
#include <algorithm>
#include <cstdio>
#include <random>

struct Tag { uint32_t row; uint64_t start, count; };

int main()
{
    std::mt19937 rng(20240607u);
    auto upto = [&](uint32_t n) { return (uint32_t)(rng() % (n + 1)); };   // 0 .. n
    const int cases = 400;
    for (int c = 0; c < cases; ++c) {
        const uint32_t rows = 1 + upto(2);
        const uint64_t N = 40 + upto(360);
        std::vector<Tag> tags;
        for (uint32_t r = 0; r < rows; ++r) {
            std::vector<uint64_t> starts(N + 20);
            for (size_t i = 0; i < starts.size(); ++i) starts[i] = i;
            std::shuffle(starts.begin(), starts.end(), rng);
            const uint32_t nt = upto(12);
            for (uint32_t i = 0; i < nt; ++i) tags.push_back(Tag{r, starts[i], upto(3) ? upto(80) : upto(2)});   // some runs of 0-2 items, some past N
        }
        std::shuffle(tags.begin(), tags.end(), rng);
        qrl::ZeroRunList list;
        for (const Tag& t : tags) list.add(t.row, t.start, t.count);

        std::vector<std::vector<char>> got(rows, std::vector<char>(N, 0));
        std::vector<qrl::ZeroRun> live;
        for (uint64_t lo = 0; lo < N;) {
            const uint64_t hi = std::min<uint64_t>(N, lo + 1 + upto((uint32_t)N / 3));
            list.split(lo, hi, live);
            for (const qrl::ZeroRun& z : live) {
                if (z.row >= rows) { std::printf("case %d: live run of row %u\n", c, z.row); return 1; }
                for (uint64_t t = std::max(lo, z.start); t < std::min(hi, z.start + z.count); ++t) got[z.row][t] = 1;
            }
            lo = hi;
        }
        for (uint32_t r = 0; r < rows; ++r)
            for (uint64_t t = 0; t < N; ++t) {
                bool want = false;
                for (const Tag& i : tags) {
                    if (i.row != r || !(i.start <= t && t < i.start + i.count)) continue;
                    bool cut = false;
                    for (const Tag& j : tags) cut |= j.row == r && i.start < j.start && j.start <= t;
                    want |= !cut;
                }
                if (want != (bool)got[r][t]) {
                    std::printf("case %d: row %u item %llu: zeroed %d, the rule says %d (N = %llu, %zu tags)\n", c, r, (unsigned long long)t, (int)got[r][t],
                                (int)want, (unsigned long long)N, tags.size());
                    return 1;
                }
            }
        for (const qrl::ZeroRun& z : list.runs)
            if (z.start + z.count <= N) {
                std::printf("case %d: run [%llu, +%llu) of row %u is still listed after item %llu\n", c, (unsigned long long)z.start,
                            (unsigned long long)z.count, z.row, (unsigned long long)N);
                return 1;
            }
    }
    std::printf("ok %d\n", cases);
    return 0;
}
