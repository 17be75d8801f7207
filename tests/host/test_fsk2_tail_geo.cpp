// test_fsk2_tail_geo — the host arithmetic of k_2fsk_tail (qradiolink_amd/csrc/fsk2_tail_geo.hpp) on the CPU, for 16 / 32 / 64 streams per workgroup:
//   lds       the arrays are 8-byte aligned, in order, do not overlap, every index the kernel forms stays inside its stream's pitch, and a
//             workgroup fits the 160 KB of a compute unit
//   banks     a half wave of the FIR role (8 streams x 4 threads, consecutive words of one row) reads 64 different banks with its 8-byte reads
//             of the y and f rings and 32 different banks with its 4-byte reads of the d ring, at every row and word
//   windows   for every count 0 .. 6000: the trips j = FIRST + 1 .. nwin, in which the FLL role writes window j (0 <= j < nwin) and the FIR role
//             works on window j - 1, never touch one y slot from both sides; the prologue's fetch of window j (trip j - 1, behind the stages)
//             lands in a slot that stage 1 of that trip does not read; the windows written back cover the last KEEP samples of the call
//   eligible  only the 16-tap FLL with the (11, 11, 7) tap quads, not FM, QRL_OPT_FLL_SLIM off
// Built with -fsanitize=address,undefined by tests/test_fsk2_tail_geo_host.py.  Ends with "ok <checks>"; exit status 1 with the first violation.
#include "../../qradiolink_amd/csrc/fsk2_tail_geo.hpp"
#include <cstdio>
#include <set>
#include <vector>

using namespace qrl;
using G = Fsk2TailGeo;

static long checks = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { std::printf("line %d: %s is false\n", __LINE__, #cond); return false; } } while (0)

static bool check_lds(int ns)
{
    const size_t off[] = {G::off_y(ns), G::off_f(ns), G::off_x(ns), G::off_dump(ns), G::off_d(ns), G::off_taps(ns), G::lds_bytes(ns)};
    const size_t need[] = {(size_t)ns * G::YP * 8, (size_t)ns * G::FP * 8, (size_t)ns * G::XP * 8, (size_t)ns * 4 * 8, (size_t)ns * G::DP * 4,
                           (size_t)(4 * G::QF + 8 * G::QB + 4 * G::QS) * 4};
    for (int i = 0; i < 6; ++i) { CHECK(off[i] % 8 == 0); CHECK(off[i] + need[i] <= off[i + 1]); }
    CHECK(G::off_taps(ns) % 16 == 0 && (4 * G::QF * 4) % 16 == 0 && ((4 * G::QF + 8 * G::QB) * 4) % 16 == 0);   // 16-byte tap reads
    CHECK(G::lds_bytes(ns) <= 160 * 1024);
    CHECK(G::threads(ns) == 8 * ns && G::threads(ns) <= 1024 && G::threads(ns) % 64 == 0);
    // the largest index of a stream's block: row 3, last word
    CHECK(3 * G::YW + G::YW - 1 < G::YP && 3 * G::FW + G::FW - 1 < G::FP && 3 * G::DW + G::DW - 1 < G::DP && G::W - 1 < G::XP);
    return true;
}

static bool check_banks(int ns)
{
    for (int half = 0; half < 2; ++half)
        for (int r = 0; r < 4; ++r) {
            for (int w = 0; w + 3 < G::YW; ++w) {
                std::set<int> banks;
                for (int l = 0; l < 32; ++l) {
                    const size_t a = G::off_y(ns) + ((size_t)((l >> 2) + 8 * half) * G::YP + r * G::YW + w + (l & 3)) * 8;
                    banks.insert((int)(a / 4 % 64)); banks.insert((int)((a / 4 + 1) % 64));
                }
                CHECK(banks.size() == 64);
            }
            for (int w = 0; w + 3 < G::FW; ++w) {
                std::set<int> banks;
                for (int l = 0; l < 32; ++l) {
                    const size_t a = G::off_f(ns) + ((size_t)((l >> 2) + 8 * half) * G::FP + r * G::FW + w + (l & 3)) * 8;
                    banks.insert((int)(a / 4 % 64)); banks.insert((int)((a / 4 + 1) % 64));
                }
                CHECK(banks.size() == 64);
            }
            for (int w = 0; w + 3 < G::DW; ++w) {
                std::set<int> banks;
                for (int l = 0; l < 32; ++l) {
                    const size_t a = G::off_d(ns) + ((size_t)((l >> 2) + 8 * half) * G::DP + r * G::DW + w + (l & 3)) * 4;
                    banks.insert((int)(a / 4 % 32));
                }
                CHECK(banks.size() == 32);
            }
        }
    return true;
}

// y slots stage 1 of window jw reads: the window's own words and QF words in front of its first one
static std::set<int> stage1_slots(int jw)
{
    std::set<int> s;
    for (int w = G::WW * jw - G::QF; w < G::WW * (jw + 1); ++w) s.insert(G::slot_y(w >= 0 ? w / G::WW : -((-w + G::WW - 1) / G::WW)));
    return s;
}

static bool check_windows(uint32_t count)
{
    const int nwin = G::nwin(count);
    CHECK((uint32_t)nwin * G::W >= count && (nwin == 0 || (uint32_t)(nwin - 1) * G::W < count));
    int trips = 0;
    for (int j = G::FIRST + 1; j <= nwin; ++j, ++trips) {
        const int jw = j - 1;
        const std::set<int> rd = stage1_slots(jw);
        CHECK((int)rd.size() <= G::YWIN - 1);
        if (j >= 0 && j < nwin) CHECK(!rd.count(G::slot_y(j)));          // the FLL role's window of this trip
        if (jw < -1) CHECK(!rd.count(G::slot_y(jw + 1)));                // the prologue's next window
    }
    CHECK(G::barriers(count) == 1 + trips);
    // what the first FIR window reads was fetched in front of the loop
    for (int w = G::WW * G::FIRST - G::QF; w < G::WW * (G::FIRST + 1); ++w) CHECK(w >= G::WW * G::LOAD0);
    // the windows written back hold the last KEEP samples of the call (all of it when it is shorter)
    const int64_t first_kept = (int64_t)G::first_keep_window(count) * G::W;
    CHECK(first_kept <= (count > (uint32_t)G::KEEP ? (int64_t)count - G::KEEP : 0));
    CHECK(G::first_keep_window(count) >= 0 && G::first_keep_window(count) <= (nwin ? nwin - 1 : 0));
    return true;
}

int main()
{
    for (int ns : {16, 32, 64}) if (!check_lds(ns) || !check_banks(ns)) return 1;
    for (uint32_t count = 0; count <= 6000; ++count) if (!check_windows(count)) return 1;
    for (uint32_t count : {262144u / 50u, 1u << 20}) if (!check_windows(count)) return 1;
    {
        auto ok = [] {
            CHECK(fsk2_tail_eligible(true, 16, 41, 41, 25, false));
            CHECK(!fsk2_tail_eligible(true, 16, 41, 41, 25, true));       // QRL_OPT_FLL_SLIM = 1: the unfused pair
            CHECK(!fsk2_tail_eligible(false, 16, 41, 41, 25, false));     // FM variants, other families
            CHECK(!fsk2_tail_eligible(true, 32, 41, 41, 25, false));
            CHECK(!fsk2_tail_eligible(true, 16, 37, 41, 25, false) && !fsk2_tail_eligible(true, 16, 41, 45, 25, false) && !fsk2_tail_eligible(true, 16, 41, 41, 21, false));
            return true;
        };
        if (!ok()) return 1;
    }
    std::printf("ok %ld\n", checks);
    return 0;
}
