// kernels_2fsk_tail.hip — k_2fsk_tail: fll_band_edge_cc and the three FIR stages behind it (gr_demod_2fsk.cpp:90-104,140-152) in ONE
// wave-specialised kernel.  The arithmetic is that of k_fll (kernels_loops.hip) and of k_2fsk_ff<11, 11, 7> (kernels_ff.hip), chain for
// chain -- both take it from fsk2_steps.hpp, as this kernel does; what changes is who runs when and where the hand-off lives:
//   FLL waves   QRL_FLL_STEP, four lanes per stream, 16 streams per wave.  y goes into the stream's LDS ring instead of an LDS
//               window that is flushed to the r2l ring in HBM.
//   FIR waves   one per 16 streams, four threads per stream, each thread four consecutive outputs of a stage (the register window of
//               window4).  While the FLL waves work on window j they run _filter -> band-pass pair / divide / rail -> _symbol_filter on
//               window j - 1; a stream's three stages hand over through LDS inside one wave.
// One __syncthreads() per window (the FLL -> FIR hand-off and the reuse of the y ring); trip counts come from P.count alone.
// Between calls the chain lives in the r2l ring as before: a call stores its last windows of y there (>= the 104 samples the first
// output of the next call depends on) and starts by fetching them and recomputing the f and d items in front of q0 -- the halo
// recomputation k_2fsk_ff does per tile, so the unfused kernels (QRL_OPT_FLL_SLIM = 1) can take over between any two calls and back.
// Geometry, ring sizes and pitches: fsk2_tail_geo.hpp.
#include "devmath.hpp"
#include "engine.hpp"
#include "fsk2_tail_geo.hpp"
#include "fsk2_steps.hpp"

namespace qrl {

// LDS hand-over inside one wave: the writes of all lanes in front of the reads behind (LDS operations of a wave complete in order)
__device__ __forceinline__ void tl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NS>
__global__ __launch_bounds__(Fsk2TailGeo::threads(NS)) void k_2fsk_tail(const Fsk2TailParams P, int batch)
{
    using G = Fsk2TailGeo;
    constexpr int TH = G::threads(NS), NFLL = NS / 16;
    constexpr int NT = G::FLL_NT, GL = NT / 4, W = G::W;
    constexpr int YW = G::YW, FW = G::FW, DW = G::DW, YP = G::YP, FP = G::FP, DP = G::DP, XP = G::XP;
    static_assert(NS % 16 == 0 && TH <= 1024, "whole waves of 16 streams");
    extern __shared__ __align__(16) unsigned char tl_smem[];
    float2* const Y = reinterpret_cast<float2*>(tl_smem + G::off_y(NS));        // [NS][YP]  FLL output ring
    float2* const F = reinterpret_cast<float2*>(tl_smem + G::off_f(NS));        // [NS][FP]  _filter output ring
    float2* const X = reinterpret_cast<float2*>(tl_smem + G::off_x(NS));        // [NS][XP]  FLL input window
    float2* const dump = reinterpret_cast<float2*>(tl_smem + G::off_dump(NS));  // [4 NS]    lanes 1-3 of a quad store their copy of y here
    float* const D = reinterpret_cast<float*>(tl_smem + G::off_d(NS));          // [NS][DP]  discriminator output ring

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const bool is_fll = wv < NFLL;                    // wave-uniform role
    const int b0 = blockIdx.x * NS;
    const int nstreams = min(NS, batch - b0);
    const uint32_t count = P.fll.count;
    const int nwin = G::nwin(count);
    const uint64_t q0 = P.fll.q0;

    for (int i = tid; i < (int)(G::off_taps(NS) / 4); i += TH) reinterpret_cast<uint32_t*>(tl_smem)[i] = 0u;
    float* const T = reinterpret_cast<float*>(tl_smem + G::off_taps(NS));       // tf[44] | up[44] (re, im) | ts[28]
    for (int i = tid; i < 4 * G::QF; i += TH) T[i] = P.ff.tf[i];
    for (int i = tid; i < 4 * G::QB; i += TH) reinterpret_cast<float2*>(T + 4 * G::QF)[i] = P.ff.up[i];
    for (int i = tid; i < 4 * G::QS; i += TH) T[4 * G::QF + 8 * G::QB + i] = P.ff.ts[i];
    const float* const tap_f = T; const float2* const tap_b = reinterpret_cast<const float2*>(T + 4 * G::QF); const float* const tap_s = T + 4 * G::QF + 8 * G::QB;
    __syncthreads();

    // ---- FLL lanes: stream sl of the workgroup, group g of its delay line (k_fll)
    const int sl = is_fll ? tid >> 2 : 0, g = tid & 3;
    const bool fll_active = is_fll && b0 + sl < batch;
    float phase = 0.f, freq = 0.f;
    float2 dl[GL], hu[GL], hl[GL];
    constexpr int NPT = W * 16 / 64;                  // input items a lane stages per window: its wave's 16 streams x W samples
    float2 pre[NPT];
#pragma unroll
    for (int t = 0; t < GL; ++t) { dl[t] = make_float2(0.f, 0.f); hu[t] = hl[t] = make_float2(0.f, 0.f); }
#pragma unroll
    for (int i = 0; i < NPT; ++i) pre[i] = make_float2(0.f, 0.f);
    auto preload = [&](uint32_t c0) {   // NPT unconditional 8-byte loads, their latency hidden behind the window's recursion
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int s = min(16 * wv + (lane >> 4) + 4 * i, nstreams - 1), k = lane & 15;
            const int64_t a = (int64_t)(q0 + c0 + k) - NT;   // x[n - NT]; ring reads are in bounds for any index
            const float2 v = P.fll.in.p[(size_t)(b0 + s) * (P.fll.in.mask + 1u) + ((uint32_t)a & P.fll.in.mask)];
            pre[i] = a >= 0 ? v : make_float2(0.f, 0.f);
        }
    };
    // ---- FIR lanes: stream fs of the workgroup, word ft of a window
    const int fs = is_fll ? 0 : 16 * (wv - NFLL) + (lane >> 2), ft = lane & 3;
    const int fb = b0 + fs;
    const bool fir_active = !is_fll && fb < batch;
    float2* const Ys = Y + fs * YP;
    float2* const Fs = F + fs * FP;
    float* const Ds = D + fs * DP;
    const bool al4 = (q0 & 3u) == 0;                  // a thread's four r3 items are one aligned 16-byte group
    float hold[4] = {0.f, 0.f, 0.f, 0.f};             // r3 goes out two windows at a time: 128 contiguous bytes per stream
    // window pj < 0 of y from the history ring; items in front of q0 - KEEP, or of the stream's start, are zero
    auto fetch_y = [&](int pj, float2 (&v)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int off = W * pj + 4 * ft + r;
            const int64_t a = (int64_t)q0 + off;
            const float2 x = P.ff.in.p[(size_t)(b0 + min(fs, nstreams - 1)) * (P.ff.in.mask + 1u) + ((uint32_t)a & P.ff.in.mask)];
            v[r] = (a >= 0 && off >= -G::KEEP && fir_active) ? x : make_float2(0.f, 0.f);
        }
    };
    auto put_y = [&](int pj, const float2 (&v)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Ys[r * YW + 4 * G::slot_y(pj) + ft] = v[r];
    };
    auto store_r3 = [&](int jw, const float (&v)[4]) {
        const uint32_t t0 = (uint32_t)(W * jw + 4 * ft);
        if (!fir_active || t0 >= count) return;
        float* const row = P.ff.out.p + (size_t)fb * (P.ff.out.mask + 1u);
        const uint64_t n = q0 + t0;
        if (al4 && t0 + 3u < count) *reinterpret_cast<float4*>(row + ((uint32_t)n & P.ff.out.mask)) = make_float4(v[0], v[1], v[2], v[3]);
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) if (t0 + r < count) row[(uint32_t)(n + r) & P.ff.out.mask] = v[r];
        }
    };

    // The two roles run loops of their own (the registers of one are not live in the other) with the same trips: j = FIRST + 1 .. nwin, one
    // __syncthreads() each, whatever the data.
    if (is_fll) {
        if (fll_active) {
            const FllState& s = P.fll.st[b0 + sl];
            phase = s.phase; freq = s.freq;
#pragma unroll
            for (int t = 0; t < GL; ++t) dl[t] = s.dl[g * GL + t];
        }
#pragma unroll
        for (int t = 0; t < GL; ++t) { hu[t] = P.fll.upper[g * GL + t]; hl[t] = P.fll.lower[g * GL + t]; }   // entry j of the tables belongs to y[n - j]
        preload(0);
        int ys_w = 0;                                 // slot of the y window being written: slot_y(j)
        for (int j = G::FIRST + 1; j <= nwin; ++j) {
            if (j >= 0 && j < nwin) {
                const uint32_t c0 = (uint32_t)(W * j);
                const int len = min((uint32_t)W, count - c0);
#pragma unroll
                for (int i = 0; i < NPT; ++i) X[(16 * wv + (lane >> 4) + 4 * i) * XP + (lane & 15)] = pre[i];
                tl_wave_sync();
                if (j + 1 < nwin) preload(c0 + W);
                if (fll_active) {
                    const float2* const xw = X + sl * XP;
                    float2* const yr = Y + sl * YP + 4 * ys_w;
                    for (int k = 0; k < len; ++k) {
                        const float2 x = xw[k];
                        // item k of the window: row k & 3, word k >> 2
                        QRL_FLL_STEP(GL, P.fll, x, g, g == 0 ? &yr[(k & 3) * YW + (k >> 2)] : &dump[tid], phase, freq, dl, hu, hl)
                    }
                }
                ys_w = ys_w == G::YWIN - 1 ? 0 : ys_w + 1;
            }
            __syncthreads();
        }
        if (fll_active) {
            FllState& s = P.fll.st[b0 + sl];
            if (g == 0) { s.phase = phase; s.freq = freq; }
#pragma unroll
            for (int t = 0; t < GL; ++t) s.dl[g * GL + t] = dl[t];
        }
    } else {
        float2 v[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fetch_y(G::LOAD0 + i, v[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) put_y(G::LOAD0 + i, v[i]);
        static_assert(G::LOAD0 + 3 == G::FIRST, "windows LOAD0 .. FIRST in front of the loop, one more per prologue trip");
        int ys_r = G::slot_y(G::FIRST), fs_r = G::slot_f(G::FIRST);   // slots of the window being worked on: slot_y(j - 1), slot_f(j - 1)
        for (int j = G::FIRST + 1; j <= nwin; ++j) {
            const int jw = j - 1;                                  // FIRST .. nwin - 1
            const int64_t n0 = (int64_t)q0 + W * jw + 4 * ft;      // absolute index of this thread's first item, all three stages
            const uint32_t t0 = (uint32_t)(W * jw + 4 * ft);       // ... inside the call (jw >= 0)
            float2 nv[4];
            if (jw < -1) fetch_y(jw + 1, nv);                      // the next prologue window, in flight behind this one's stages
            if (jw >= 0) {
                if (jw == 0 && ft == 0 && fir_active && P.ff.counts) P.ff.counts[fb * 4 + 0] = count;
                if (jw >= nwin - G::KEEP_WIN && fir_active) {      // the call's last windows of y: the next call's history
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (t0 + r < count) P.ff.in.p[(size_t)fb * (P.ff.in.mask + 1u) + ((uint32_t)(n0 + r) & P.ff.in.mask)] = Ys[r * YW + 4 * ys_r + ft];
                }
            }
            {   // stage 1: f[n] = sum tf[k] y[n - k]
                AccRealCplx acc;
                window4<YW, true, G::QF, true>(Ys, 4 * ys_r + ft, 0, tap_f, acc);
                float2 (&a)[4] = acc.a;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n0 + r < 0) a[r] = make_float2(0.f, 0.f);
                    Fs[r * FW + 4 * fs_r + ft] = a[r];
                }
                if (jw >= 0 && fir_active && P.ff.port) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (t0 + r < count && t0 + r < P.ff.port_cap) P.ff.port[(size_t)fb * P.ff.port_cap + t0 + r] = a[r];
                }
            }
            tl_wave_sync();
            if (jw >= -2) {   // stage 2: conjugate tap pair (AccConjPair): A = sum a f, B = sum b f; d = rail(|u| / |l|) - 1
                AccConjPair<4> acc;
                window4<FW, true, G::QB, true>(Fs, 4 * fs_r + ft, 0, tap_b, acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = acc.disc(r);   // unconditional: a select, not a branch
                    Ds[r * DW + 4 * fs_r + ft] = (n0 + r < 0) ? 0.f : d;
                }
                tl_wave_sync();
            }
            if (jw >= 0) {    // stage 3: o[n] = sum ts[k] d[n - k]
                AccRealReal acc;
                window4<DW, true, G::QS, true>(Ds, 4 * fs_r + ft, 0, tap_s, acc);
                const float (&a)[4] = acc.a;
                if ((jw & 1) == 0 && jw != nwin - 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) hold[r] = a[r];
                } else {
                    if (jw & 1) store_r3(jw - 1, hold);
                    store_r3(jw, a);
                }
            }
            if (jw < -1) put_y(jw + 1, nv);
            ys_r = ys_r == G::YWIN - 1 ? 0 : ys_r + 1;
            fs_r = (fs_r + 1) & (G::FWIN - 1);
            __syncthreads();
        }
    }
}

#ifndef QRL_TAIL_NS
#define QRL_TAIL_NS 64   // streams per workgroup: 64 = four FLL and four FIR waves, one of each per SIMD
#endif
size_t fsk2_tail_lds_bytes() { return Fsk2TailGeo::lds_bytes(QRL_TAIL_NS); }

void launch_2fsk_tail(const Fsk2TailParams& p, int batch, hipStream_t s)
{
    if (!p.fll.count) return;
    constexpr int NS = QRL_TAIL_NS;
    const auto k = k_2fsk_tail<NS>;
    const size_t lds = Fsk2TailGeo::lds_bytes(NS);
    if (dyn_lds_limit(reinterpret_cast<const void*>(k), (int)lds) != hipSuccess) return;
    hipLaunchKernelGGL(k, dim3((batch + NS - 1) / NS), dim3(Fsk2TailGeo::threads(NS)), lds, s, p, batch);
}

}  // namespace qrl
