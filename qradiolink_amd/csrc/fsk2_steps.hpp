// fsk2_steps.hpp — the arithmetic chains that the unfused 2FSK kernels (k_fll: kernels_loops.hip; k_2fsk_ff, k_disc_2fsk: kernels_ff.hip)
// and the fused k_2fsk_tail (kernels_2fsk_tail.hip) have in common, each ONCE: the contract on all of them is bit-exactness against the
// oracle chain for chain, and a handle may switch between the fused kernel and the pair from call to call.  Device only.
#pragma once
#include "devmath.hpp"
#include "engine.hpp"

namespace qrl {

template <int CTRL> __device__ __forceinline__ float dpp_quad(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// ------------------------------------------------------------------ FLL band edge: one sample
// FOUR LANES PER STREAM.  The two NT-tap band-edge filters are the bulk of the arithmetic but only their newest link sits on
// the recursion's critical path, so the delay line is cut into 4 groups of GL = NT/4 samples, one per lane of a quad: every lane
// runs the short oldest-first fmaf chains of its group, the delay line shifts through the quad with one DPP move, and the
// partial sums meet by two DPP butterflies as (p0 + p1) + (p2 + p3) -- the summation contract of oracle orc_fll_band_edge.
// The NCO / loop update is computed redundantly by the four lanes (bit-identical inputs, bit-identical results).  Compared with
// a lane-per-stream kernel there are 4x more waves (one per SIMD instead of one per CU at 16k streams) with ~3x shorter
// instruction streams.
// x = x[n - NT]; g = this lane's group; dl[t] = y[n - (g GL + t)]; hu / hl = this lane's taps (entry j of the device tables belongs
// to y[n - j]); y_dst = where this lane stores y: the output slot for lane 0 of a quad, a dump slot of its own for lanes 1-3.
// Critical path: NCO -> derotated sample -> newest link of lane 0 -> butterflies -> loop update.  The body is ONE basic block (no
// lane-dependent branch, hence the dump slot), so the scheduler can fill the dependency gaps of this chain with the independent work.
// P = the FllParams; phase, freq, dl (float2[GL]) = the lane's state, updated in place.
// A MACRO, not a function: both callers are latency-bound loops, one wave per SIMD.  As a function template with the lane state behind
// references the delay line goes through the loop as i64 instead of <2 x float> and the schedule changes: with that alone
// k_2fsk_tail's C1 step measured 0.054 ms slower in each of four alternating passes (ranges 0.011), and the step over
// k_fll<16, 64, 16> 0.01 - 0.20 ms slower in each of eight.  Expanded in place both kernels have the instructions they had with the
// step written out in each (docs/KERNELS.md section 28, profiles/fsk2_steps_ab.txt).
#define QRL_FLL_STEP(GL, P, x, g, y_dst, phase, freq, dl, hu, hl)                                                                    \
    {                                                                                                                                \
        const float2 nco = sincos_rad(phase); /* (cos, sin) */                                                                       \
        /* independent of this sample's NCO: shift the delay line through the quad -- lane g takes the oldest entry of lane */       \
        /* g - 1 -- and run the oldest-first chains over everything but the newest slot */                                           \
        float2 carry;                                                                                                                \
        carry.x = dpp_quad<0x90>(dl[GL - 1].x);                                                                                      \
        carry.y = dpp_quad<0x90>(dl[GL - 1].y);                                                                                      \
        _Pragma("unroll") for (int t = GL - 1; t > 0; --t) dl[t] = dl[t - 1];                                                        \
        float ur = 0.f, ui = 0.f, lr = 0.f, li = 0.f;                                                                                \
        _Pragma("unroll") for (int t = GL - 1; t >= 1; --t) {                                                                        \
            const float2 v = dl[t];                                                                                                  \
            ur = fmaf(hu[t].x, v.x, ur); ur = fmaf(-hu[t].y, v.y, ur);                                                               \
            ui = fmaf(hu[t].x, v.y, ui); ui = fmaf(hu[t].y, v.x, ui);                                                                \
            lr = fmaf(hl[t].x, v.x, lr); lr = fmaf(-hl[t].y, v.y, lr);                                                               \
            li = fmaf(hl[t].x, v.y, li); li = fmaf(hl[t].y, v.x, li);                                                                \
        }                                                                                                                            \
        const float2 y = cmul(x, nco);                                                                                               \
        *(y_dst) = y;                                                                                                                \
        dl[0] = g == 0 ? y : carry;                                                                                                  \
        {                                                                                                                            \
            const float2 v = dl[0];                                                                                                  \
            ur = fmaf(hu[0].x, v.x, ur); ur = fmaf(-hu[0].y, v.y, ur);                                                               \
            ui = fmaf(hu[0].x, v.y, ui); ui = fmaf(hu[0].y, v.x, ui);                                                                \
            lr = fmaf(hl[0].x, v.x, lr); lr = fmaf(-hl[0].y, v.y, lr);                                                               \
            li = fmaf(hl[0].x, v.y, li); li = fmaf(hl[0].y, v.x, li);                                                                \
        }                                                                                                                            \
        /* (p0 + p1) + (p2 + p3): quad butterflies (lane ^ 1, then lane ^ 2); float addition commutes, so all four */                \
        /* lanes end up with the same bits */                                                                                        \
        ur = ur + dpp_quad<0xB1>(ur); ui = ui + dpp_quad<0xB1>(ui); lr = lr + dpp_quad<0xB1>(lr); li = li + dpp_quad<0xB1>(li);      \
        ur = ur + dpp_quad<0x4E>(ur); ui = ui + dpp_quad<0x4E>(ui); lr = lr + dpp_quad<0x4E>(lr); li = li + dpp_quad<0x4E>(li);      \
        const float error = (lr * lr + li * li) - (ur * ur + ui * ui);                                                               \
        freq = freq + (P).beta * error;                                                                                              \
        phase = phase + freq + (P).alpha * error;                                                                                    \
        phase = phase_wrap(phase);                                                                                                   \
        freq = __builtin_fminf(__builtin_fmaxf(freq, -(P).max_freq), (P).max_freq); /* == the two-sided clamp for finite freq */     \
    }

// ------------------------------------------------------------------ four outputs per thread: the register window
// Rows are TRANSPOSED by 4: item i sits at row i & 3 (STRIDE words apart), word i >> 2, so that a thread owns the four consecutive
// outputs of word w and slides a register window over the taps -- one read per tap for four outputs instead of four -- while the lanes
// of a wave read consecutive words.  acc[r] += sum_k taps[k] * item[4 w + r - k], k = 0 .. 4 nq - 1, every acc[r] ONE fmaf chain, k
// ascending: the chain of the one-output-per-thread kernels, followed by the zero taps of the padding, which leave the value untouched.
// What callers choose:
//   RING    false: the word index steps back linearly (k_2fsk_ff's tiles, which have their halo in front); true: modulo a ring of STRIDE
//           words (k_2fsk_tail's per-stream rings);
//   NQ, FULL  NQ > 0: nq is a compile-time constant and the loop is unrolled by four (FULL = false) or completely (FULL = true);
//           NQ = 0: the run-time count nq_rt, not unrolled;
//   taps    wave-uniform global memory (scalar loads) or LDS.
// The scalar loads share their counter with the LDS reads, so they cannot be prefetched across a quad's LDS wait.  Unrolled by four
// the tap loads of four quads are issued together, one wait per sixteen taps: at C1's geometry (41 + 41 + 25 taps) k_2fsk_ff takes
// 855 us alone, against 1 011 in the per-quad form (29 waits per thread) and 914 unrolled completely (105 VGPRs);
// profiles/r06_c1_helper_stream.log.  A FIR wave of k_2fsk_tail is alone on its SIMD beside one FLL wave and nothing hides a wait:
// there the taps are in LDS (a 16-byte broadcast read per quad, in order with the window reads) and the loop is unrolled completely,
// 2.08 ms for the kernel alone against 2.52 with scalar taps unrolled by four (docs/KERNELS.md section 28).
template <int STRIDE, bool RING, int NQ, bool FULL, typename TapT, typename ItemT, typename Fma>
__device__ __forceinline__ void window4(const ItemT* __restrict__ rows, int w, int nq_rt, const TapT* __restrict__ taps, Fma&& fma4)
{
    ItemT cur[4], nxt[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) cur[s] = rows[s * STRIDE + w];
    auto quad = [&](int q) {
        w = (RING && w == 0 ? STRIDE : w) - 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) nxt[s] = rows[s * STRIDE + w];   // word w - 1: rows 1..3 are this step's u < 0 samples
        const TapT h0 = taps[4 * q], h1 = taps[4 * q + 1], h2 = taps[4 * q + 2], h3 = taps[4 * q + 3];
        fma4(h0, cur[0], cur[1], cur[2], cur[3]);     // e = 0: output r takes sample u = r
        fma4(h1, nxt[3], cur[0], cur[1], cur[2]);     // e = 1: u = r - 1
        fma4(h2, nxt[2], nxt[3], cur[0], cur[1]);     // e = 2: u = r - 2
        fma4(h3, nxt[1], nxt[2], nxt[3], cur[0]);     // e = 3: u = r - 3
#pragma unroll
        for (int s = 0; s < 4; ++s) cur[s] = nxt[s];
    };
    if constexpr (NQ > 0 && FULL) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) quad(q);
    } else if constexpr (NQ > 0) {
#pragma unroll 4
        for (int q = 0; q < NQ; ++q) quad(q);
    } else {
        for (int q = 0; q < nq_rt; ++q) quad(q);
    }
}

// The accumulate steps of window4: the four accumulators and what one tap adds to them.
struct AccRealCplx {   // real tap x complex items (fft_filter_ccf)
    float2 a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
    __device__ __forceinline__ void operator()(float h, const float2& x0, const float2& x1, const float2& x2, const float2& x3)
    {
        a[0].x = fmaf(h, x0.x, a[0].x); a[0].y = fmaf(h, x0.y, a[0].y);
        a[1].x = fmaf(h, x1.x, a[1].x); a[1].y = fmaf(h, x1.y, a[1].y);
        a[2].x = fmaf(h, x2.x, a[2].x); a[2].y = fmaf(h, x2.y, a[2].y);
        a[3].x = fmaf(h, x3.x, a[3].x); a[3].y = fmaf(h, x3.y, a[3].y);
    }
};
// the two band-pass filters are a conjugate pair (the engine checks it bit for bit): h = a + j b, A = sum a x, B = sum b x (real taps, k
// ascending, the real and imaginary parts of the UPPER filter's taps), upper = (A.re - B.im, A.im + B.re), lower = (A.re + B.im,
// A.im - B.re) -- oracle orc_fir_ccc_conj_pair.  N outputs: 4 under window4, 1 in the one-output-per-thread k_disc_2fsk.
template <int N>
struct AccConjPair {
    float ar[N] = {}, ai[N] = {}, br[N] = {}, bi[N] = {};
    __device__ __forceinline__ void tap(const float2 h, const float2 x, int r)
    {
        ar[r] = fmaf(h.x, x.x, ar[r]); ai[r] = fmaf(h.x, x.y, ai[r]);
        br[r] = fmaf(h.y, x.x, br[r]); bi[r] = fmaf(h.y, x.y, bi[r]);
    }
    __device__ __forceinline__ void operator()(const float2 h, const float2& x0, const float2& x1, const float2& x2, const float2& x3)
    {
        const float2 xs[4] = {x0, x1, x2, x3};
#pragma unroll
        for (int r = 0; r < 4; ++r) tap(h, xs[r], r);
    }
    // the discriminator behind the pair: complex_to_mag x2 -> divide -> rail(0, 2) -> add_const(-1) (gr_demod_2fsk.cpp:94-102,140-149).
    // Callers compute it unconditionally and SELECT zero for an item in front of the stream start: as one arm of a ?: it becomes a
    // branch per output, and k_2fsk_tail then takes 256 VGPRs and 272 bytes of scratch instead of 156 and none.  A member reading the
    // accumulators, not a free function of four floats: that form pairs k_2fsk_ff<11, 11, 7>'s packed FMAs differently (60 VGPRs
    // for 56) and costs it 7 % (docs/KERNELS.md section 28).
    __device__ __forceinline__ float disc(int r) const
    {
        const float ur = ar[r] - bi[r], ui = ai[r] + br[r], lr = ar[r] + bi[r], li = ai[r] - br[r];
        const float mu = sqrtf(ur * ur + ui * ui);
        const float ml = sqrtf(lr * lr + li * li);
        float v = mu / ml;
        if (!(v >= 0.0f)) v = 0.0f;   // rail_ff lower bound; NaN (0/0) -> 0
        if (v > 2.0f) v = 2.0f;
        return v + (-1.0f);
    }
};
struct AccRealReal {   // real tap x real items (fft_filter_fff)
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    __device__ __forceinline__ void operator()(float h, float x0, float x1, float x2, float x3)
    {
        a[0] = fmaf(h, x0, a[0]); a[1] = fmaf(h, x1, a[1]); a[2] = fmaf(h, x2, a[2]); a[3] = fmaf(h, x3, a[3]);
    }
};

}  // namespace qrl
