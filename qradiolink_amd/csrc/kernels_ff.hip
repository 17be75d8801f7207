// kernels_ff.hip — feed-forward blocks at the decimated rate (<= 2 % of the input bytes).
// One thread per output item, inputs read from the producer's ring (L2-resident), one fmaf chain
// per output with k ascending: exactly the order of oracle/orc_blocks.c.
//   k_fir_ccf    fft_filter_ccf  (gr_demod_2fsk.cpp:91-92, gr_demod_gmsk.cpp:84-85, gr_demod_qpsk.cpp:100-103)
//   k_fir_fff    fft_filter_fff  (gr_demod_2fsk.cpp:104, gr_demod_gmsk.cpp:96-98)
//   k_quad_demod quadrature_demod_cf (gr_demod_gmsk.cpp:95, gr_demod_2fsk.cpp:112)
//   k_disc_2fsk  2x fft_filter_ccc + complex_to_mag + divide + rail(0,2) + add(-1) (gr_demod_2fsk.cpp:94-102,140-149)
#include "devmath.hpp"
#include "engine.hpp"
#include "fsk2_steps.hpp"
#include <cstdlib>

namespace qrl {

__global__ __launch_bounds__(256) void k_fir_ccf(const FirCcfParams P)
{
    const int b = blockIdx.y;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P.count) return;
    if (t == 0 && P.counts) P.counts[b * 4 + 0] = P.count;
    const int64_t n = (int64_t)(P.q0 + t);
    float ar = 0.f, ai = 0.f;
    for (int k = 0; k < P.nt; ++k) {
        const float h = P.taps[k];
        const float2 x = ringc_at(P.in, b, n - k);
        ar = fmaf(h, x.x, ar);
        ai = fmaf(h, x.y, ai);
    }
    const float2 y = make_float2(ar, ai);
    P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = y;
    if (P.port && t < P.port_cap) P.port[(size_t)b * P.port_cap + t] = y;
}
// LDS-tiled variants for the longer filters (RRC shaping filters of the FM / 4FSK / BPSK chains, 75 ... 501 taps): a workgroup
// stages FT_OUT + nt - 1 input items of one stream and the taps in LDS, every thread then produces FT_R outputs 256 apart
// (consecutive lanes -> consecutive LDS words, taps are wave-uniform broadcasts).  Same fmaf chain, k ascending.
constexpr int FT_R = 4, FT_OUT = 256 * FT_R, FT_MAXT = 1024;

template <int MAXT>   // 1024 for the digital chains; 2048 for the 1904-tap channel filter of gr_demod_wbfm (its own instance: the larger LDS
                      // footprint would cost the short filters occupancy)
__global__ __launch_bounds__(256) void k_fir_ccf_tiled(const FirCcfParams P)
{
    __shared__ float taps[MAXT];
    __shared__ float2 xs[FT_OUT + MAXT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * (uint32_t)FT_OUT;
    const int nt = P.nt;
    for (int k = tid; k < nt; k += 256) taps[k] = P.taps[k];
    const int64_t first = (int64_t)(P.q0 + t0) - (nt - 1);         // xs[i] = x[first + i]
    const int span = min((uint32_t)FT_OUT, P.count - t0) + nt - 1;
    for (int i = tid; i < span; i += 256) xs[i] = ringc_at(P.in, b, first + i);
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0 && P.counts) P.counts[b * 4 + 0] = P.count;
    float ar[FT_R], ai[FT_R];
#pragma unroll
    for (int r = 0; r < FT_R; ++r) { ar[r] = 0.f; ai[r] = 0.f; }
    const float2* xp = xs + (nt - 1) + tid;                        // output j = tid + 256 r reads xp[256 r - k]
    for (int k = 0; k < nt; ++k) {
        const float h = taps[k];
#pragma unroll
        for (int r = 0; r < FT_R; ++r) {
            const float2 x = xp[256 * r - k];
            ar[r] = fmaf(h, x.x, ar[r]);
            ai[r] = fmaf(h, x.y, ai[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < FT_R; ++r) {
        const uint32_t t = t0 + tid + 256u * r;
        if (t < P.count) {
            const int64_t n = (int64_t)(P.q0 + t);
            const float2 y = make_float2(ar[r], ai[r]);
            P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = y;
            if (P.port && t < P.port_cap) P.port[(size_t)b * P.port_cap + t] = y;
        }
    }
}
__global__ __launch_bounds__(256) void k_fir_fff_tiled(const FirFffParams P)
{
    __shared__ float taps[FT_MAXT];
    __shared__ float xs[FT_OUT + FT_MAXT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * (uint32_t)FT_OUT;
    const int nt = P.nt;
    for (int k = tid; k < nt; k += 256) taps[k] = P.taps[k];
    const int64_t first = (int64_t)(P.q0 + t0) - (nt - 1);
    const int span = min((uint32_t)FT_OUT, P.count - t0) + nt - 1;
    for (int i = tid; i < span; i += 256) xs[i] = ringf_at(P.in, b, first + i);
    __syncthreads();
    float a[FT_R];
#pragma unroll
    for (int r = 0; r < FT_R; ++r) a[r] = 0.f;
    const float* xp = xs + (nt - 1) + tid;
    for (int k = 0; k < nt; ++k) {
        const float h = taps[k];
#pragma unroll
        for (int r = 0; r < FT_R; ++r) a[r] = fmaf(h, xp[256 * r - k], a[r]);
    }
#pragma unroll
    for (int r = 0; r < FT_R; ++r) {
        const uint32_t t = t0 + tid + 256u * r;
        if (t < P.count) P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)(P.q0 + t) & P.out.mask)] = a[r];
    }
}
// (the per-thread global-load form only for the shortest filters / calls: at 23 taps it is texture-address bound -- C5: 2.57 ms
// for 134 M outputs, the tiled form reads every input once)
static bool fir_use_tiled(int nt, uint32_t count) { return nt >= 8 && nt <= FT_MAXT && count >= 512; }

void launch_fir_ccf(const FirCcfParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    if (fir_use_tiled(p.nt, p.count)) hipLaunchKernelGGL(k_fir_ccf_tiled<FT_MAXT>, dim3((p.count + FT_OUT - 1) / FT_OUT, batch), dim3(256), 0, s, p);
    else if (p.nt > FT_MAXT && p.nt <= 2 * FT_MAXT && p.count >= 512)
        hipLaunchKernelGGL(k_fir_ccf_tiled<2 * FT_MAXT>, dim3((p.count + FT_OUT - 1) / FT_OUT, batch), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_fir_ccf, dim3((p.count + 255) / 256, batch), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_fir_fff(const FirFffParams P)
{
    const int b = blockIdx.y;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P.count) return;
    const int64_t n = (int64_t)(P.q0 + t);
    float a = 0.f;
    for (int k = 0; k < P.nt; ++k) a = fmaf(P.taps[k], ringf_at(P.in, b, n - k), a);
    P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = a;
}
void launch_fir_fff(const FirFffParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    if (fir_use_tiled(p.nt, p.count)) hipLaunchKernelGGL(k_fir_fff_tiled, dim3((p.count + FT_OUT - 1) / FT_OUT, batch), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_fir_fff, dim3((p.count + 255) / 256, batch), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_quad_demod(const QuadDemodParams P)
{
    __shared__ float T[257];
    for (int k = threadIdx.x; k < 257; k += 256) T[k] = P.atan_tab[k];
    __syncthreads();
    const int b = blockIdx.y;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P.count) return;
    const int64_t n = (int64_t)(P.q0 + t);
    const float2 a = ringc_at(P.in, b, n), p = ringc_at(P.in, b, n - 1);
    const float re = a.x * p.x + a.y * p.y;
    const float im = a.y * p.x - a.x * p.y;
    const float ang = fast_atan2f_lut(im, re, T);
    P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = P.gain * ang;
    if (P.out2.p) P.out2.p[(size_t)b * (P.out2.mask + 1u) + ((uint32_t)n & P.out2.mask)] = P.gain2 * ang;
    if (P.s16) {   // multiply_const_ff(level) + float_to_short(1, scale) (gr_demod_mmdvm_multi2.cpp:84,92), as k_f2s
        float r = rintf(((P.gain * ang) * P.s16_level) * P.s16_scale);
        if (r > 32767.0f) r = 32767.0f;
        if (r < -32768.0f) r = -32768.0f;
        if (t < P.s16_cap) P.s16[(size_t)b * P.s16_cap + t] = (int16_t)r;
        if (t == 0 && P.s16_counts) P.s16_counts[b] = P.count < P.s16_cap ? P.count : (uint32_t)P.s16_cap;
    }
}
void launch_quad_demod(const QuadDemodParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    hipLaunchKernelGGL(k_quad_demod, dim3((p.count + 255) / 256, batch), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_disc_2fsk(const Disc2fskParams P)
{
    const int b = blockIdx.y;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P.count) return;
    const int64_t n = (int64_t)(P.q0 + t);
    // the conjugate tap pair of AccConjPair (fsk2_steps.hpp), one output per thread
    AccConjPair<1> acc;
    for (int k = 0; k < P.nt; ++k) {
        const float2 x = ringc_at(P.in, b, n - k);
        acc.tap(P.up[k], x, 0);
    }
    P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = acc.disc(0);
}
// gr_demod_4fsk non-FM branch (gr_demod_4fsk.cpp:110-127,165-176 + gr_4fsk_discriminator::work, gr_4fsk_discriminator.cpp:17-44):
// four complex band-pass filters -> complex_to_mag -> strict arg-max -> one of (+-0.707107, +-0.707107), else 0
__global__ __launch_bounds__(256) void k_disc_4fsk(const Disc4fskParams P)
{
    const int b = blockIdx.y;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= P.count) return;
    const int64_t n = (int64_t)(P.q0 + t);
    float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < P.nt; ++k) {
        const float2 x = ringc_at(P.in, b, n - k);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float2 h = P.taps[q * P.nt + k];
            re[q] = fmaf(h.x, x.x, re[q]); re[q] = fmaf(-h.y, x.y, re[q]);
            im[q] = fmaf(h.x, x.y, im[q]); im[q] = fmaf(h.y, x.x, im[q]);
        }
    }
    const float m1 = sqrtf(re[0] * re[0] + im[0] * im[0]), m2 = sqrtf(re[1] * re[1] + im[1] * im[1]);
    const float m3 = sqrtf(re[2] * re[2] + im[2] * im[2]), m4 = sqrtf(re[3] * re[3] + im[3] * im[3]);
    const float A = 0.707107f;
    float2 v = make_float2(0.f, 0.f);
    if (m1 > m2 && m1 > m3 && m1 > m4) v = make_float2(-A, -A);
    else if (m2 > m1 && m2 > m3 && m2 > m4) v = make_float2(-A, A);
    else if (m3 > m2 && m3 > m1 && m3 > m4) v = make_float2(A, A);
    else if (m4 > m2 && m4 > m1 && m4 > m3) v = make_float2(A, -A);
    P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = v;
}
void launch_disc_4fsk(const Disc4fskParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    hipLaunchKernelGGL(k_disc_4fsk, dim3((p.count + 255) / 256, batch), dim3(256), 0, s, p);
}

void launch_disc_2fsk(const Disc2fskParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    hipLaunchKernelGGL(k_disc_2fsk, dim3((p.count + 255) / 256, batch), dim3(256), 0, s, p);
}

// ---- fused feed-forward part of the non-FM 2FSK chain (gr_demod_2fsk.cpp:91-104,140-152):
//   _filter (fft_filter_ccf) -> {_upper_filter, _lower_filter} (fft_filter_ccc) -> complex_to_mag x2 -> divide ->
//   rail(0,2) -> add_const(-1) -> _symbol_filter (fft_filter_fff)
// One workgroup = FF_T consecutive outputs of one stream; the three FIR stages run out of LDS with the intermediate
// halos recomputed (6 % extra MACs).  Every thread owns FOUR consecutive outputs of a stage (window4, fsk2_steps.hpp); tiles are
// stored TRANSPOSED by 4 (item i at row i & 3, word (i >> 2) + 1).  Taps are wave-uniform (scalar loads) and zero padded to 4A + 1
// entries.  Items at negative absolute index are zero, exactly as a ring read in front of the stream start returns zero.
constexpr int FF_PL = 280, FF_PF = 264, FF_PD = 264;   // row pitches (words); 8-byte rows: pitch = 8 or 24 (mod 32)

template <int NQF, int NQB, int NQS>   // tap quads of the three filters ((padded taps - 1) / 4 + 1), or 0, 0, 0 = run-time counts
__global__ __launch_bounds__(256) void k_2fsk_ff(const Fsk2FfParams P)
{
    __shared__ float2 lt[4 * FF_PL];   // FLL output, item i <-> abs n0t - (hf + hb + hs) + i
    __shared__ float2 ft[4 * FF_PF];   // _filter output, item j <-> abs n0t - (hb + hs) + j
    __shared__ float dt[4 * FF_PD];    // discriminator output, item j <-> abs n0t - hs + j
    const int b = blockIdx.y, tid = threadIdx.x;
    const int hf = P.nf - 1, hb = P.nb - 1, hs = P.ns - 1;      // multiples of 4 (padded tap counts 4A + 1)
    const int T = 1024 - hb - hs;                                // outputs per workgroup: stage 1 computes exactly 1024 items
    const int64_t n0t = (int64_t)P.q0 + (int64_t)blockIdx.x * T;
    const int nl = 1024 + hf, nd = T + hs;
    if (tid < 4) { lt[tid * FF_PL] = make_float2(0.f, 0.f); ft[tid * FF_PF] = make_float2(0.f, 0.f); dt[tid * FF_PD] = 0.f; }
    {   // nl <= 1064 items: five unconditional ring reads per thread in flight together (ring reads are in bounds for any index)
        float2 v[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int64_t a = n0t - (hf + hb + hs) + tid + 256 * it;
            v[it] = P.in.p[(size_t)b * (P.in.mask + 1u) + ((uint32_t)a & P.in.mask)];
            if (a < 0) v[it] = make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            const int i = tid + 256 * it;
            if (i < nl) lt[(i & 3) * FF_PL + (i >> 2) + 1] = v[it];
        }
    }
    __syncthreads();
    {   // stage 1: f[j] = sum tf[k] l[j + hf - k], j = 4 tid + r
        AccRealCplx acc;
        window4<FF_PL, false, NQF, false>(lt, tid + (hf >> 2) + 1, (hf >> 2) + 1, P.tf, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool neg = n0t - (hb + hs) + 4 * tid + r < 0;
            ft[r * FF_PF + tid + 1] = neg ? make_float2(0.f, 0.f) : acc.a[r];
        }
    }
    __syncthreads();
    if (4 * tid < nd) {   // stage 2: u/l[j] = sum up/lo[k] f[j + hb - k]; d = rail(|u| / |l|) - 1
        AccConjPair<4> acc;
        window4<FF_PF, false, NQB, false>(ft, tid + (hb >> 2) + 1, (hb >> 2) + 1, P.up, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = acc.disc(r);   // unconditional: a select, not a branch
            dt[r * FF_PD + tid + 1] = (n0t - hs + 4 * tid + r < 0) ? 0.f : d;
        }
    }
    __syncthreads();
    if (4 * tid < T) {   // stage 3: y[o] = sum ts[k] d[o + hs - k]
        AccRealReal acc;
        window4<FF_PD, false, NQS, false>(dt, tid + (hs >> 2) + 1, (hs >> 2) + 1, P.ts, acc);
        const uint32_t t0 = blockIdx.x * (uint32_t)T + 4u * tid;   // output index inside this call
        if (t0 == 0 && P.counts) P.counts[b * 4 + 0] = P.count;
        const int wf = tid + ((hb + hs) >> 2) + 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t t = t0 + r;
            if (t < P.count) {
                const int64_t n = n0t + 4 * tid + r;
                P.out.p[(size_t)b * (P.out.mask + 1u) + ((uint32_t)n & P.out.mask)] = acc.a[r];
                if (P.port && t < P.port_cap) P.port[(size_t)b * P.port_cap + t] = ft[r * FF_PF + wf];
            }
        }
    }
}
// padded tap count of the fused kernel: 4 A + 1 >= n (tables hold 4 (A + 1) entries, zero filled)
int fsk2_ff_padded(int n) { return (n - 1 + 3) / 4 * 4 + 1; }
void launch_2fsk_ff(const Fsk2FfParams& p, int batch, hipStream_t s)
{
    if (!p.count) return;
    const int T = 1024 - (p.nb - 1) - (p.ns - 1);
    const dim3 grid((p.count + T - 1) / T, batch);
    // gr_demod_2fsk's designs at sps = 10 / 5 (2FSK-1k, -2k: 41 + 41 + 25 taps at 20 / 40 ksps) and at sps = 1 (10k: 80 ksps) are the instantiations
    static const bool rt = [] { const char* e = getenv("QRL_FF_RUNTIME_TAPS"); return e && atoi(e) != 0; }();
    const int qf = (p.nf - 1) / 4 + 1, qb = (p.nb - 1) / 4 + 1, qs = (p.ns - 1) / 4 + 1;
    if (!rt && qf == 11 && qb == 11 && qs == 7) hipLaunchKernelGGL((k_2fsk_ff<11, 11, 7>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_2fsk_ff<0, 0, 0>), grid, dim3(256), 0, s, p);
}

}  // namespace qrl
