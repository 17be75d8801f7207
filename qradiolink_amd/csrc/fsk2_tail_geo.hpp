// fsk2_tail_geo.hpp — geometry of k_2fsk_tail (kernels_2fsk_tail.hip), the FLL and the three FIR stages of the non-FM 2FSK chain in one
// wave-specialised kernel: window and ring sizes, LDS pitches and offsets, which calls get the kernel.  Host arithmetic free of HIP, so
// that tests/host/test_fsk2_tail_geo.cpp can run it under the sanitizers on the CPU.
//
// A workgroup owns NS streams and walks them in windows of W samples.  Per stream the LDS holds three rings of 4-item WORDS, stored
// transposed by 4 as the tiles of k_2fsk_ff are (item i of a ring at row i & 3, word (i >> 2) mod ring words): y (FLL output), f (_filter
// output) and d (discriminator output).  An FIR thread owns four consecutive outputs = one word of a window, and reads QUADS words back.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qrl {

struct Fsk2TailGeo {
    static constexpr int W = 16, WW = W / 4;                     // samples / words per window
    static constexpr int FLL_NT = 16;                            // band-edge taps of the 2FSK FLL
    static constexpr int QF = 11, QB = 11, QS = 7;               // tap quads of _filter, the band-pass pair, _symbol_filter (41 + 41 + 25 taps)
    static constexpr int HF = 4 * (QF - 1), HB = 4 * (QB - 1), HS = 4 * (QS - 1);   // their histories: 40, 40, 24
    static constexpr int KEEP = HF + HB + HS;                    // y samples in front of a call that its first output depends on: 104
    // ring words.  y: the FLL waves write window j while the FIR waves read window j - 1 and QF words in front of its first word (the
    // oldest holds zero-tap items only, but they are the true items, as in k_2fsk_ff); f and d have one writer and reader, the FIR wave
    static constexpr int YW = 20, FW = 16, DW = 16;
    static constexpr int YWIN = YW / WW, FWIN = FW / WW;         // windows per ring
    // per-stream pitches in items: four rows + 4.  A half wave is 8 streams x 4 threads reading 4 consecutive words of one row: the 8-byte
    // reads (y, f) cover 64 different banks when the pitch is 4 x odd, the 4-byte reads (d) 32 different banks (the host test walks the lanes)
    static constexpr int YP = 4 * YW + 4, FP = 4 * FW + 4, DP = 4 * DW + 4;
    static constexpr int XP = W + 1;                             // FLL input staging, as k_fll's window: [stream][W + 1]
    static constexpr int FIRST = -4;                             // first window the FIR waves run (stage 1 from q0 - 64, stage 2 from window -2)
    static constexpr int LOAD0 = -7;                             // first window of y fetched from the history ring (q0 - 112; items in front of q0 - KEEP read as zero)
    static constexpr int KEEP_WIN = 8;                           // windows of y at the end of a call that go back to the history ring (>= KEEP + W - 1 samples)

    static_assert(KEEP == 104, "history of the three filters");
    static_assert(YW >= 2 * WW + QF + 1 && YW % WW == 0, "y ring: a window being written, one being read, QF words of history and the zero-tap word");
    static_assert(FW >= WW + QB + 1 && FW % WW == 0 && DW >= WW + QS + 1 && DW % WW == 0, "f / d rings");
    static_assert(-LOAD0 * W >= KEEP && (-FIRST + 0) * WW + QF <= -LOAD0 * WW, "the fetch covers what the first FIR window reads");
    static_assert(-FIRST * W >= HB + HS && 2 * W >= HS, "stage 1 from q0 - 64, stage 2 from q0 - 32 <= q0 - 24");
    static_assert(KEEP_WIN * W >= KEEP + W - 1, "the windows written back hold the last KEEP samples for any count");
    static_assert(YWIN >= -FIRST + 1, "windows FIRST .. -1 and window 0 do not share a slot: the FLL starts beside the FIR window -1");

    static constexpr int threads(int ns) { return 4 * ns + 64 * (ns / 16); }          // 4 lanes per stream (FLL) + one FIR wave per 16 streams
    static constexpr size_t off_y(int) { return 0; }
    static constexpr size_t off_f(int ns) { return off_y(ns) + (size_t)ns * YP * 8; }
    static constexpr size_t off_x(int ns) { return off_f(ns) + (size_t)ns * FP * 8; }
    static constexpr size_t off_dump(int ns) { return off_x(ns) + (size_t)ns * XP * 8; }
    static constexpr size_t off_d(int ns) { return off_dump(ns) + (size_t)ns * 4 * 8; }
    static constexpr size_t off_taps(int ns) { return off_d(ns) + (size_t)ns * DP * 4; }                  // tf[4 QF] | up[4 QB] (re, im) | ts[4 QS], floats
    static constexpr size_t lds_bytes(int ns) { return off_taps(ns) + (size_t)(4 * QF + 8 * QB + 4 * QS) * 4; }

    static constexpr int nwin(uint32_t count) { return (int)((count + (uint32_t)W - 1) / (uint32_t)W); }
    static constexpr int slot_y(int j) { return ((j % YWIN) + YWIN) % YWIN; }
    static constexpr int slot_f(int j) { return ((j % FWIN) + FWIN) % FWIN; }
    static constexpr int first_keep_window(uint32_t count) { return nwin(count) > KEEP_WIN ? nwin(count) - KEEP_WIN : 0; }
    static constexpr int barriers(uint32_t count) { return 1 + (nwin(count) - (FIRST + 1) + 1); }   // per wave: one behind the LDS clear, one per trip j = FIRST + 1 .. nwin
};

// which calls get the kernel: the 16-tap FLL in front of gr_demod_2fsk's 41 + 41 + 25 designs (2FSK-1k, -2k), not FM, QRL_OPT_FLL_SLIM off
// (nf / nb / ns: the padded tap counts of fsk2_ff_padded)
inline bool fsk2_tail_eligible(bool fsk2_non_fm, int fll_nt, int nf, int nb, int ns, bool fll_slim)
{
    return fsk2_non_fm && !fll_slim && fll_nt == Fsk2TailGeo::FLL_NT && (nf - 1) / 4 + 1 == Fsk2TailGeo::QF && (nb - 1) / 4 + 1 == Fsk2TailGeo::QB &&
           (ns - 1) / 4 + 1 == Fsk2TailGeo::QS;
}

}  // namespace qrl
