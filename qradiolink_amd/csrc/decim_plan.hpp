// decim_plan.hpp — the host-side integer arithmetic of the decimating front end (DecimStage, launch_decim*), free of HIP: which kernel class
// a geometry gets, the sizes a handle allocates from, how one call's outputs are split between the streaming kernel, the staged edge scratch
// and the per-output kernel, and the segment geometry of a launch.  Results must not depend on how a stream is cut into calls, and THIS is
// where that is decided; tests/host/test_decim_plan.cpp checks it on the CPU under the sanitizers.  The launchers only launch.
#pragma once
#include <cstdint>
#include <cstddef>
#include <algorithm>

namespace qrl {

// outputs of an I / D resampler that exist once n input samples do: a call covers the outputs [decim_count(n0), decim_count(n0 + n))
inline uint64_t decim_count(uint64_t n, int I, int D) { return n ? ((n - 1) * (uint64_t)I + (uint64_t)I - 1) / (uint64_t)D + 1 : 0; }

// ---- generic tile kernel k_decim<R, JC> (kernels_frontend.hip) ----
enum { DECIM_R4_J44 = 0, DECIM_R4_J12 = 1, DECIM_R2_J10 = 2, DECIM_R1_J14 = 3 };
inline void decim_variant(int variant, int& R, int& JC)
{
    switch (variant) {
    case DECIM_R4_J44: R = 4; JC = 44; break;
    case DECIM_R4_J12: R = 4; JC = 12; break;
    case DECIM_R2_J10: R = 2; JC = 10; break;
    default: R = 1; JC = 14; break;
    }
}
inline int decim_jc(int variant) { int R, JC; decim_variant(variant, R, JC); return JC; }
inline size_t decim_lds_bytes(int D, int Jpad, int variant)
{
    int R, JC;
    decim_variant(variant, R, JC);
    const int TILE = 64 * R;
    const int W = TILE + Jpad;
    const int Wq = (W + R - 1) / R;
    const int PT = (R * Wq) | 1;
    return (size_t)(512 + 64 + 4 * TILE + D * PT) * 8;   // complex samples
}

// ---- f32-MFMA decimator k_decim_mfma (D >= 8): contract "m16" of oracle/orc_blocks.c ----
inline int decim_mfma_steps(int nt, int D)
{
    const int S = (nt + 15 * D + 3) / 4;
    return (S + 3) / 4 * 4;
}
inline int decim_mfma_hpn(int nt, int D) { return (15 * D + 4 * decim_mfma_steps(nt, D) + 4 + 3) & ~3; }
inline long long mfma_jtot(int nt, int D, int NA) { return (long long)(NA - 1) * 16 * D + 4LL * decim_mfma_steps(nt, D); }
inline int mfma_nhi(int nt, int D, int NA) { return (int)(mfma_jtot(nt, D, NA) / 512 + 3); }
inline size_t mfma_lds(int nt, int D, int NA)
{
    const long long Jtot = mfma_jtot(nt, D, NA);
    const long long npos = Jtot + 2 * (Jtot / (16LL * D)) + 4 + 512 + 16;   // + dump slots (+ pad slack of the unpredicated commit)
    return (size_t)(512 + ((mfma_nhi(nt, D, NA) + 1) & ~1) + npos) * 8 + (size_t)decim_mfma_hpn(nt, D) * 4;   // complex samples + float taps
}
// rule shared with oracle/orc_blocks.c orc_decim_uses_m16
inline bool decim_uses_mfma(int nt, int D)
{
    if (D < 8) return false;
    const long long samples = 7LL * 16 * D + 4LL * decim_mfma_steps(nt, D);
    return (samples + 2 * (samples / (16LL * D)) + 64) * 8 <= 150 * 1024;
}
// 16 output blocks per tile when two workgroups of that size fit the 160 KB of a CU, else 8
inline int decim_mfma_na(int nt, int D)
{
    if (mfma_lds(nt, D, 16) <= 80 * 1024) return 16;    // two (or more) workgroups per CU with the efficient tile
    if (mfma_lds(nt, D, 8) <= 160 * 1024) return 8;   // (4-block tiles with three workgroups per CU were measured slower)
    return 4;   // very long filters (100:1 front end, 4181 taps): only the 4-block tile fits the 160 KB of a CU
}
// one call of launch_decim_mfma.  fast: the tile comes from the caller's cf32 buffer through register-prefetched 16-byte loads
struct MfmaPlan {
    int NA; uint32_t tiles, tpw, nchunks; int nhi; size_t lds;
    int nld;      // 16-byte loads per thread a tile needs, with the thread count the kernel runs with
    bool big;     // 512-thread workgroups
    bool slow;    // a fast tile that needs more than 16 loads per thread even with 512 threads: per-sample staging
};
inline MfmaPlan decim_mfma_plan(int nt, int D, uint64_t m0, uint32_t m_count, int batch, bool fast)
{
    constexpr int kTpwMax = 16;
    MfmaPlan pl{};
    pl.NA = decim_mfma_na(nt, D);
    const uint32_t T = 16 * pl.NA;
    pl.tiles = (uint32_t)((m0 + m_count + T - 1) / T - m0 / T);
    // consecutive tiles per workgroup: enough to amortise the un-overlapped first load, few enough to keep >= ~4k workgroups
    const uint64_t total = (uint64_t)pl.tiles * (uint64_t)batch;
    pl.tpw = (uint32_t)std::min<uint64_t>(kTpwMax, std::max<uint64_t>(1, total / 4096));
    pl.nchunks = (pl.tiles + pl.tpw - 1) / pl.tpw;
    pl.nhi = mfma_nhi(nt, D, pl.NA);
    pl.lds = mfma_lds(nt, D, pl.NA);
    const long long pairs = (mfma_jtot(nt, D, pl.NA) + 2) / 2;
    const int nld = (int)((pairs + 255) / 256);
    // More than 16 loads per thread (front ends beyond ~40:1): a 36-load variant would need 144 prefetch registers, more than
    // the accumulator half of the register file holds, and hipcc then spills registers whose asm-issued loads are still in
    // flight.  Those tiles run with 512 threads (<= 16 loads per thread); anything larger takes the slow per-sample staging.
    const int nld512 = (int)((pairs + 511) / 512);
    pl.big = fast && nld > 16 && nld512 <= 16;
    pl.nld = pl.big ? nld512 : nld;
    pl.slow = fast && nld > 16 && !pl.big;
    return pl;
}

// ---- register-resident phase-lane decimator k_decim_plx: contract "pl" (oracle/orc_blocks.c orc_pl_geometry) ----
constexpr int PLX_NHI = 256;       // coarse rotator entries per wave: a segment spans <= 255 x 512 samples
struct PlGeom { int R, Dp, E, U, Upad, WU; bool ok; };
inline PlGeom pl_geom(int nt, int D)
{
    PlGeom g{};
    g.R = D <= 32 ? 64 / D : 1;
    g.Dp = g.R * D;
    g.E = (g.Dp + 63) / 64;
    g.U = (nt + g.Dp - 1) / D;
    g.Upad = g.U;
    if (g.E == 1 && g.R == 1) g.ok = false;   // 32 < D <= 64: the phase-major matrix-pipe kernel (decim_uses_pm) or the generic paths
    else if (g.E == 2 && g.R == 1) { g.ok = (D % 2) == 0 && g.U <= 42; g.Upad = 42; }   // (the front-end filters have 41.8 D taps: U = 42 for every D)
    else g.ok = false;
    g.WU = (g.Upad - 1) / g.R;
    return g;
}
// rule shared with oracle/orc_blocks.c orc_decim_uses_pl
inline bool decim_uses_pl(int nt, int D) { return pl_geom(nt, D).ok; }
// samples of edge scratch per stream (0: geometry without the register kernel)
inline size_t decim_pl_edge_len(int nt, int D)
{
    const PlGeom g = pl_geom(nt, D);
    return g.ok ? (size_t)(2 * g.WU + 4) * g.Dp : 0;   // warm-up blocks + the blocks of <= (WU + 1) R + 1 edge outputs
}
inline uint32_t decim_pl_lookback(int nt, int D) { return (uint32_t)(((nt + D - 1) / D + 1) * D); }

// ---- phase-major matrix-pipe decimator k_decim_pm: contract "pm" (rule shared with oracle/orc_blocks.c orc_decim_uses_pm) ----
inline bool decim_uses_pm(int nt, int D)
{
    const int J = (nt + D - 1) / D, NS = (D + 3) / 4;
    if (D > 32 && D <= 52 && J <= 16) return true;                // one lag tile: the 1:50 first stages of a 1 Msps device
    // up to three lag tiles: the device-rate front ends (41.8 D taps) at 10:1, 20:1, 25:1, 50:1, 100:1
    return J > 16 && J <= 48 && (NS == 3 || NS == 5 || NS == 7 || NS == 13 || NS == 25);
}
// block lags the instantiated kernel walks (its table is zero beyond the filter's own J): segment alignment, edge unit and look-back
// are all counted in THESE lags
inline int pm_kernel_lags(int nt, int D)
{
    const int J = (nt + D - 1) / D, NS = (D + 3) / 4;
    if (J <= 16) return J == 9 && NS == 13 ? 9 : 16;
    return J <= 42 ? 42 : 48;
}
inline int pm_tiles(int J) { return J <= 16 ? 1 : 3; }
inline size_t decim_pm_edge_len(int nt, int D)
{
    // the edge unit of a call starts at the 16-block group of block m0 - (J - 1) and ends with the last output in front of the first
    // aligned segment: at most 15 + (J - 1) + (J + 16) blocks
    const int J = pm_kernel_lags(nt, D);
    return decim_uses_pm(nt, D) ? (size_t)(((2 * J + 32) * D + 1) & ~1) : 0;
}
inline uint32_t decim_pm_lookback(int nt, int D) { return (uint32_t)((pm_kernel_lags(nt, D) + 18) * D); }

// ---- the class of a stage (DecimStage::plan): pm -> pl -> m16 -> generic, the order of oracle/orc_blocks.c orc_decim_auto ----
enum { DECIM_CLASS_PM, DECIM_CLASS_PL, DECIM_CLASS_M16, DECIM_CLASS_GENERIC, DECIM_CLASS_NONE /* the generic tile does not fit a CU's LDS */ };
struct DecimChoice { int cls; int variant, Jpad; /* generic class only */ };
inline DecimChoice decim_choose(int nt, int D)
{
    if (decim_uses_pm(nt, D)) return DecimChoice{DECIM_CLASS_PM, DECIM_R4_J12, 0};   // phase-major matrix-pipe kernel (the 1:50 first stages)
    if (decim_uses_pl(nt, D)) return DecimChoice{DECIM_CLASS_PL, DECIM_R4_J12, 0};   // register-resident phase-lane kernel (the 100:1 front end)
    if (decim_uses_mfma(nt, D)) return DecimChoice{DECIM_CLASS_M16, DECIM_R4_J12, 0};
    const int J = (nt + D - 1) / D;
    const size_t kLds2 = 80 * 1024;  // two workgroups per CU
    auto pad = [&](int v) { const int jc = decim_jc(v); return (J + jc - 1) / jc * jc; };
    int variant;
    if (J <= 10 && decim_lds_bytes(D, pad(DECIM_R2_J10), DECIM_R2_J10) <= kLds2) variant = DECIM_R2_J10;
    else if (J > 36 && J <= 44 && decim_lds_bytes(D, 44, DECIM_R4_J44) <= kLds2) variant = DECIM_R4_J44;
    else if (decim_lds_bytes(D, pad(DECIM_R4_J12), DECIM_R4_J12) <= kLds2) variant = DECIM_R4_J12;
    else variant = DECIM_R1_J14;
    const int Jpad = pad(variant);
    return DecimChoice{decim_lds_bytes(D, Jpad, variant) > 160 * 1024 ? DECIM_CLASS_NONE : DECIM_CLASS_GENERIC, variant, Jpad};
}
// input samples in front of a call's first one that the stage reads (what the carried history has to hold)
inline uint32_t decim_lookback(const DecimChoice& c, int nt, int D)
{
    return c.cls == DECIM_CLASS_PM ? decim_pm_lookback(nt, D) : c.cls == DECIM_CLASS_PL ? decim_pl_lookback(nt, D)
         : c.cls == DECIM_CLASS_M16 ? (uint32_t)(nt + D) : (uint32_t)(c.Jpad * D);
}

// ---- can the streaming kernel read this call's buffer? (the `stream_ok` of decim_split) ----
// What a launcher knows about the call's input: the caller's buffer (in_base = 0: the stage reads an engine ring), whether the rotator runs
// in this stage, the row pitch and the call's length in samples, the sample format, and the stage's edge scratch (cf32 whatever the format).
// iq8 (appended, so that the seven-field initialisers of older callers stay valid): the buffer holds 8-bit pairs, 2 bytes per sample (sc8 / cu8).
struct CallInput { uint64_t in_base; uint64_t in_stride; uint32_t n; bool sc16; bool rot; uint64_t edge_base; uint32_t edge_stride; bool iq8 = false; };
// log2 of the bytes per sample of the caller's buffer: cf32 3, int16 pairs 2, 8-bit pairs 1
inline uint32_t in_sample_shift(bool sc16, bool iq8 = false) { return iq8 ? 1u : sc16 ? 2u : 3u; }
// samples per 16-byte piece, minus one: cf32 rows are whole pieces at even sample counts, int16 rows at multiples of FOUR samples, 8-bit rows at
// multiples of EIGHT
inline uint32_t pm_piece_mask(bool sc16, bool iq8 = false) { return (16u >> in_sample_shift(sc16, iq8)) - 1u; }
// pm: the matrix kernel streams the rows of the buffer as 16-byte LDS-DMA pieces, so the base, the row pitch and the row length are whole
// pieces, in EVERY format and at every lag-tile count (one tile: the 1:50 first stages; three: the device-rate front ends); the edge unit of
// the same launch reads the scratch the same way.  Anything else: one thread per output (k_decim_pm_gen).
inline bool decim_pm_streamable(const CallInput& c)
{
    const uint32_t amask = pm_piece_mask(c.sc16, c.iq8);
    return c.in_base && c.rot && (c.in_base & 15u) == 0 && (c.in_stride & amask) == 0 && (c.n & amask) == 0 &&
           c.edge_base && (c.edge_base & 15u) == 0 && (c.edge_stride & 1u) == 0;
}
// pl: the register kernel loads per lane (8 or 4 bytes): any caller's buffer that is rotated here
inline bool decim_pl_streamable(const CallInput& c) { return c.in_base && c.rot; }

// ---- one call of the pm / pl launchers: outputs [m0, m0 + m_count) from the samples [n0, n0 + n) ----
// Half-open output ranges, in order: per-output kernel, edge unit of the streaming kernel (reads the staged scratch: ROTATED samples
// edge_i0 .. edge_i0 + edge_len - 1, absolute indices, edge_i0 may be negative), the streaming kernel's segments on the caller's buffer,
// per-output kernel.  With a streamable buffer and the scratch at its designed size (decim_*_edge_len) both per-output ranges are empty.
struct OutRange { uint64_t lo, hi; bool empty() const { return hi <= lo; } uint64_t count() const { return empty() ? 0 : hi - lo; } };
struct DecimSplit { OutRange gen_head, edge, main, gen_tail; int64_t edge_i0; uint32_t edge_len; };
// Block c = samples (c - 1) D + 1 .. c D; output m reads the blocks m - warm .. m.  The oldest block of a segment, and the first block of
// the scratch, open a group of `align` blocks (pm: 16, the columns of a matrix result; pl: 1).  stream_ok: the kernel can stream the
// caller's buffer; edge_cap: samples of scratch per stream.
inline DecimSplit decim_split(uint64_t n0, uint32_t n, uint64_t m0, uint32_t m_count, int D, int warm, int align, uint32_t edge_cap, bool stream_ok)
{
    const uint64_t m_end = m0 + m_count, A = (uint64_t)align;
    uint64_t m_main = m_end, m_tail = m_end;                           // [m_main, m_tail): the segments
    if (stream_ok) {
        // interior segments start at outputs m == warm (mod align), and their oldest block lies in the buffer
        const uint64_t qb = n0 > 1 ? (n0 - 1 + D - 1) / D : 0;         // block qb + 1 is the first one whose samples are all >= n0
        m_main = (qb + 1 + A - 1) / A * A + (uint64_t)warm;
        if (m_main < m0) m_main = m0 + ((uint64_t)warm % A + A - m0 % A) % A;
        const uint64_t c_max = (n0 + n - 1) / D;                       // last block that ends inside the buffer
        m_tail = std::max(std::min(c_max + 1, m_end), m0);
        if (m_main > m_tail) m_main = m_tail;
    }
    // the head [m0, m_main) through the scratch, which starts with the group of block m0 - warm, when it fits: else one by one
    const int64_t cfs = (int64_t)m0 - warm;
    const int64_t c0 = (cfs >= 0 ? cfs / align : -((-cfs + align - 1) / align)) * align;
    const int64_t i0 = (c0 - 1) * (int64_t)D + 1;
    const int64_t i_last = (int64_t)(m_main - 1) * D;                  // last sample of the last edge output's newest block
    const int64_t len = ((i_last - i0 + 1) + 1) & ~(int64_t)1;
    const bool head = m_main > m0, staged = head && stream_ok && len <= (int64_t)edge_cap;
    const uint64_t head_end = head ? m_main : m0, edge_lo = staged ? m0 : head_end;
    return DecimSplit{{m0, edge_lo}, {edge_lo, head_end}, {m_main, m_tail}, {m_tail, m_end}, staged ? i0 : 0, staged ? (uint32_t)len : 0u};
}
inline DecimSplit decim_pm_split(uint64_t n0, uint32_t n, uint64_t m0, uint32_t m_count, int nt, int D, uint32_t edge_cap, bool stream_ok)
{
    return decim_split(n0, n, m0, m_count, D, pm_kernel_lags(nt, D) - 1, 16, edge_cap, stream_ok);
}
inline DecimSplit decim_pl_split(uint64_t n0, uint32_t n, uint64_t m0, uint32_t m_count, int nt, int D, uint32_t edge_cap, bool stream_ok)
{
    return decim_split(n0, n, m0, m_count, D, pl_geom(nt, D).WU, 1, edge_cap, stream_ok);   // (the register kernel exists for R = 1, D' = D)
}

// What launch_decim_pm / launch_decim_pl do with one call, whole: the streamability of the call's buffer decides the split, for every geometry of
// the class (tests/host/test_sc16_baseband_plan.cpp evaluates exactly these two lines for the one-tile stage fed int16)
inline DecimSplit decim_pm_plan_call(uint64_t n0, uint64_t m0, uint32_t m_count, int nt, int D, uint32_t edge_cap, const CallInput& c)
{
    return decim_pm_split(n0, c.n, m0, m_count, nt, D, edge_cap, decim_pm_streamable(c));
}
inline DecimSplit decim_pl_plan_call(uint64_t n0, uint64_t m0, uint32_t m_count, int nt, int D, uint32_t edge_cap, const CallInput& c)
{
    return decim_pl_split(n0, c.n, m0, m_count, nt, D, edge_cap, decim_pl_streamable(c));
}

// ---- segments of the streaming kernels: S outputs each, nseg per stream, one wave per unit = (stream, segment) + one edge unit per stream ----
struct DecimSegments { uint32_t S, nseg, units; };
// pm, M main outputs per stream.  Segments: a multiple of 16 outputs each (every segment then starts on a group boundary).  Every segment
// re-reads J - 1 blocks of warm-up, and the call ends when the last wave does: with `cap` waves resident on the chip (occupancy x CUs x waves
// per workgroup: the launcher asks the runtime) the cost of a split into nseg segments per stream is  ceil(nseg x batch / cap)  rounds of
// S + J - 1 + 16  blocks.  Take the cheapest split; ties go to the finer one.
// mult > 1 (per-stream offsets: the waves per workgroup): only segment counts that are multiples of mult, each stream's units then fill whole
// workgroups (one fine rotator table each; segments past the end idle, idle units counted)
inline DecimSegments pm_segments(uint64_t M, uint32_t batch, uint32_t cap, int J, uint32_t mult, bool edge_unit)
{
    uint64_t best_cost = ~0ull; uint32_t best_S = 16;
    uint32_t n_lo = (uint32_t)((M + 4095) / 4096);
    const uint32_t n_hi = (uint32_t)((M + 127) / 128);
    n_lo = (n_lo + mult - 1) / mult * mult;
    for (uint32_t nseg = n_lo; M > 16 && nseg <= (n_hi > n_lo ? n_hi : n_lo); nseg += mult) {
        const uint32_t S = (uint32_t)(((M + nseg - 1) / nseg + 15) / 16 * 16);
        const uint64_t units = (mult > 1 ? nseg : (M + S - 1) / S) * (uint64_t)batch;
        const uint64_t cost = ((units + cap - 1) / cap) * (uint64_t)(S + (uint32_t)(J - 1) + 16);
        if (cost <= best_cost) { best_cost = cost; best_S = S; }
    }
    const uint32_t nseg = (uint32_t)(((M + best_S - 1) / best_S + mult - 1) / mult * mult);
    return DecimSegments{best_S, nseg, nseg * batch + (edge_unit ? batch : 0u)};
}
// pl: two waves per SIMD (<= 256 VGPRs), ~3 segments per wave slot of the chip; a segment stays inside the wave's coarse rotator table
// (pl_segment_cap) and is a multiple of 16 outputs
inline uint64_t pl_segment_cap(const PlGeom& g) { return (uint64_t)(((PLX_NHI - 2) * 512) / g.Dp - g.WU) * g.R / 16 * 16; }
inline DecimSegments pl_segments(uint64_t M, uint32_t batch, const PlGeom& g, bool edge_unit)
{
    uint64_t S = std::min<uint64_t>(M * (uint64_t)batch / (2048u * 3u), std::min<uint64_t>(2048, pl_segment_cap(g))) / 16 * 16;
    if (S < 16) S = 16;
    const uint32_t nseg = (uint32_t)((M + S - 1) / S);
    return DecimSegments{(uint32_t)S, nseg, nseg * batch + (edge_unit ? batch : 0u)};
}

}  // namespace qrl
