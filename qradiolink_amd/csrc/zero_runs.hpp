// zero_runs.hpp — the run list of a gr_zero_idle_bursts (reference src/gr/gr_zero_idle_bursts.cpp:62-76) behind qrl_mod_add_zero_runs and
// qrl_synth_add_zero_runs.  Bookkeeping only, nothing from HIP: tests/host/test_zero_runs.cpp compiles it alone.  The device step is
// ZeroRuns::apply (tx_common.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace qrl {

struct ZeroRun { uint32_t row; uint32_t pad; uint64_t start, count; };   // ring row, absolute item range [start, start + count)

struct ZeroRunList {
    std::vector<ZeroRun> runs;
    void clear() { runs.clear(); }
    // The block keeps ONE counter per stream and a tag overwrites it: a run that starts inside another one of its row ends it there -- the
    // zeroed set is [s_i, min(s_i + c_i, s_next)) over the tags in offset order, in whatever order they are added.
    void add(uint32_t row, uint64_t start, uint64_t count)
    {
        ZeroRun z{row, 0u, start, count};
        for (ZeroRun& o : runs) {
            if (o.row != z.row) continue;
            if (o.start < z.start && o.start + o.count > z.start) o.count = z.start - o.start;
            else if (z.start < o.start && z.start + z.count > o.start) z.count = o.start - z.start;
        }
        runs.push_back(z);
    }
    // live = the runs that touch the call's items [lo, hi); the runs that end at or before hi are dropped from the list
    void split(uint64_t lo, uint64_t hi, std::vector<ZeroRun>& live)
    {
        live.clear();
        size_t kept = 0;
        for (const ZeroRun& z : runs) {
            if (z.start < hi && z.start + z.count > lo) live.push_back(z);
            if (z.start + z.count > hi) runs[kept++] = z;
        }
        runs.resize(kept);
    }
};

}  // namespace qrl
