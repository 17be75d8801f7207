// devmath.hpp — device-side deterministic math shared by the HIP kernels.
// Compiled with -ffp-contract=off: every fused multiply-add is an explicit fmaf().
// The polynomial NCO replaces libm sincosf in rotator_cc / fll_band_edge_cc / costas_loop_cc
// (GNU Radio gr_expj) so that results do not depend on a math library; see DESIGN.md "Arithmetic".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/qrl_contracts.h"

namespace qrl {

__device__ __forceinline__ float poly_sin(float x)
{
    const float z = x * x;
    float p = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    p = fmaf(z, p, -1.6666654611e-1f);
    return fmaf(x * z, p, x);
}
__device__ __forceinline__ float poly_cos(float x)
{
    const float z = x * x;
    float p = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    p = fmaf(z, p, 4.166664568298827e-2f);
    const float q = fmaf(z, -0.5f, 1.0f);
    return fmaf(z * z, p, q);
}
// returns (cos, sin)
// quadrant q: 0 -> (pc, ps), 1 -> (-ps, pc), 2 -> (-pc, -ps), 3 -> (ps, -pc).  Branch-free (two selects, two sign flips):
// the recursive loops call this once per sample and a switch costs four exec-mask regions on a wave that cannot hide them.
__device__ __forceinline__ float2 quad_fix(int q, float ps, float pc)
{
    const bool swap = q & 1;
    const uint32_t c0 = __float_as_uint(swap ? ps : pc), s0 = __float_as_uint(swap ? pc : ps);
    const uint32_t negc = ((uint32_t)(q + 1) & 2u) << 30, negs = ((uint32_t)q & 2u) << 30;
    return make_float2(__uint_as_float(c0 ^ negc), __uint_as_float(s0 ^ negs));
}
// (cos x, sin x) of a float angle in radians.  Held to orc_sincosf bit for bit for |x| <= 1e5 (tests/test_gpu_devmath.py), where the oracle stays
// within 1.8e-7 of sin / cos (tests/test_devmath_definition.py); (int)k needs |x| < 2^31 quarter turns
__device__ __forceinline__ float2 sincos_rad(float x)
{
    const float k = rintf(x * 0.636619772367581343f);
    float r = fmaf(-k, 1.57079637050628662109375f, x);
    r = fmaf(-k, -4.37113900018624283e-8f, r);
    return quad_fix((int)k, poly_sin(r), poly_cos(r));
}
// (cos, sin) of a 2^-64-turn fixed-point angle (top 32 bits used)
__device__ __forceinline__ float2 sincos_turn(uint64_t angle)
{
    const uint32_t a = (uint32_t)(angle >> 32);
    const uint32_t q = (a + 0x20000000u) >> 30;
    const int32_t r = (int32_t)(a - (q << 30));
    const float x = (float)r * 1.4629180792671596e-9f;
    return quad_fix((int)q, poly_sin(x), poly_cos(x));
}
// complex product with the fixed fmaf pattern of the rotator contract
__device__ __forceinline__ float2 cmul_fma(float2 a, float2 b)
{
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
// plain complex product (std::complex operator*: two products and one add/sub per part)
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// gnuradio fast_atan2f with its 257-entry table T
__device__ __forceinline__ float fast_atan2f_lut(float y, float x, const float* __restrict__ T)
{
    const float y_abs = fabsf(y), x_abs = fabsf(x);
    if (!((y_abs > 0.0f) || (x_abs > 0.0f))) return 0.0f;
    const float z = (y_abs < x_abs) ? (y_abs / x_abs) : (x_abs / y_abs);
    float base;
    // gnuradio compares in double: (double)z < 0.003921569.  For a float z that is z < nextfloat-at-or-above(0.003921569) = 0x3B808082 exactly
    // (0.003921569 is not a float; the floats below it are < it, 0x3B808082 is the first one >= it): one f32 compare instead of a conversion and an f64 compare
    if (z < __uint_as_float(0x3B808082u)) {
        base = z;
    } else {
        float alpha = z * 255.0f;
        const int index = ((int)alpha) & 0xff;
        alpha -= (float)index;
        const float d = T[index + 1] - T[index];
        base = T[index] + d * alpha;
    }
    const float PI_F = 3.14159265358979323846f, PIO2_F = 1.57079632679489661923f;
    float angle;
    if (x_abs > y_abs) {
        if (x >= 0.0f) angle = (y >= 0.0f) ? base : -base;
        else           angle = (y >= 0.0f) ? (PI_F - base) : (base - PI_F);
    } else {
        if (y >= 0.0f) angle = (x >= 0.0f) ? (PIO2_F - base) : (PIO2_F + base);
        else           angle = (x >= 0.0f) ? (-PIO2_F + base) : (-PIO2_F - base);
    }
    return angle;
}

__device__ __forceinline__ float tanhf_lut(float x, const float* __restrict__ T)
{
    if (x > 2.0f) return 1.0f;
    if (x <= -2.0f) return -1.0f;
    int index = (int)(128.0f + 64.0f * x);
    index = index > 255 ? 255 : (index < 0 ? 0 : index);
    return T[index];
}

__device__ __forceinline__ float branchless_clip(float x, float clip)
{
    float x1 = fabsf(x + clip);
    const float x2 = fabsf(x - clip);
    x1 -= x2;
    return 0.5f * x1;
}

// ---- float -> int16 in front of the transmitters' sc16 stores (qrl_*_process_sc16): the float_to_short rule of the oracle's f2s ----
// per component r = rintf(x * scale) (one rounded f32 multiply, round to nearest even), saturated to [-32768, 32767]; NaN gives 0.
// nclip = components with r outside the int16 range (+-inf included, NaN not).  The pair is packed I low, Q high: one 4-byte store.
__device__ __forceinline__ int sc16_sat(float r) { return r != r ? 0 : (int)fminf(fmaxf(r, -32768.0f), 32767.0f); }
__device__ __forceinline__ uint32_t f2_to_sc16(float2 v, float scale, uint32_t& nclip)
{
    const float ri = rintf(v.x * scale), rq = rintf(v.y * scale);
    nclip = (uint32_t)(ri > 32767.0f || ri < -32768.0f) + (uint32_t)(rq > 32767.0f || rq < -32768.0f);
    return ((uint32_t)sc16_sat(ri) & 0xffffu) | ((uint32_t)sc16_sat(rq) << 16);
}
// The sc16 store of every terminal TX kernel: lane `valid` writes sample v to row[idx]; clip != nullptr adds the wave's clipped components
// to *clip (the counter of this workgroup's stream) -- ballot + popcount, one atomicAdd by the first active lane, none when nothing clipped.
// The ballots see the lanes that are active at the call, and the leader is the first of THOSE: under divergence each group of lanes reduces and adds
// its own share, so the sum stays exact wherever this is called (lanes that left the kernel earlier, or that sit in another branch, are simply not in
// it).  Calling it with the wave converged is a matter of cost only: then a wave issues at most one atomic per store.
__device__ __forceinline__ void sc16_store(uint32_t* row, size_t idx, float2 v, bool valid, float scale, uint32_t* clip)
{
    uint32_t nclip;
    const uint32_t w = f2_to_sc16(v, scale, nclip);
    if (valid) row[idx] = w;
    if (clip) {
        if (!valid) nclip = 0;
        const uint32_t n = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nclip >= 1u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nclip == 2u));
        const uint64_t act = __builtin_amdgcn_ballot_w64(true);
        if (n && (int)__lane_id() == __ffsll((unsigned long long)act) - 1) atomicAdd(clip, n);
    }
}

// ---- float -> int8 in front of the transmitters' sc8 stores (qrl_*_process_sc8): the same rule one format narrower ----
// per component r = rintf(x * scale), saturated to [-128, 127]; NaN gives 0.  nclip = components with r > 127 or r < -128 (+-inf included,
// NaN not; -128 reached by rounding, as from -128.5, is in range).  The pair is packed I low byte, Q high byte: one 2-byte store.
__device__ __forceinline__ int sc8_sat(float r) { return r != r ? 0 : (int)fminf(fmaxf(r, -128.0f), 127.0f); }
__device__ __forceinline__ uint16_t f2_to_sc8(float2 v, float scale, uint32_t& nclip)
{
    const float ri = rintf(v.x * scale), rq = rintf(v.y * scale);
    nclip = (uint32_t)(ri > 127.0f || ri < -128.0f) + (uint32_t)(rq > 127.0f || rq < -128.0f);
    return (uint16_t)(((uint32_t)sc8_sat(ri) & 0xffu) | (((uint32_t)sc8_sat(rq) & 0xffu) << 8));
}
// The sc8 store of every terminal TX kernel, under sc16_store's divergence rule.  A sample is ONE 2-byte store: the other half of the 32-bit word
// belongs to the neighbouring sample, which another lane, wave or workgroup (or, behind a row's end, the caller) owns, and is never written here.
__device__ __forceinline__ void sc8_store(uint16_t* row, size_t idx, float2 v, bool valid, float scale, uint32_t* clip)
{
    uint32_t nclip;
    const uint16_t w = f2_to_sc8(v, scale, nclip);
    if (valid) row[idx] = w;
    if (clip) {
        if (!valid) nclip = 0;
        const uint32_t n = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nclip >= 1u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(nclip == 2u));
        const uint64_t act = __builtin_amdgcn_ballot_w64(true);
        if (n && (int)__lane_id() == __ffsll((unsigned long long)act) - 1) atomicAdd(clip, n);
    }
}

__device__ __forceinline__ float phase_wrap(float phase)
{
    const double TWO_PI = 6.283185307179586476925286766559;
    // same loops as gr::blocks::control_loop::phase_wrap; the common case (no lane of the wave out of range) is one uniform branch
    if (__builtin_amdgcn_ballot_w64(phase > (float)TWO_PI || phase < (float)(-TWO_PI)) == 0) return phase;
    while (phase > (float)TWO_PI) phase = (float)((double)phase - TWO_PI);
    while (phase < (float)(-TWO_PI)) phase = (float)((double)phase + TWO_PI);
    return phase;
}

// log2 of a float, the same bits on the host (oracle/orc_blocks.c orc_det_log2f) and on the device: libm's log2f is not the same
// function on both sides, IEEE double arithmetic in a fixed order is.  x = 2^e m, m in [sqrt(1/2), sqrt(2)), t = (m - 1) / (m + 1),
// ln m = 2 atanh t as an odd series to t^13 (|t| <= 0.172: truncation 4e-13), rounded to float once.  Stands in for log2f in
// nlog10_ff / volk_32fc_s32f_power_spectrum_32f (VOLK's log2f_non_ieee: +-inf becomes +-127).
__host__ __device__ inline float det_log2f(float x)
{
    if (!(x > 0.0f)) return x == 0.0f ? -127.0f : __builtin_nanf("");   // log2f(0) = -inf -> -127; negative -> nan
    if (x > 3.4028234e38f) return 127.0f;                                // log2f(inf) = inf -> 127
    int adj = 0;
    if (x < 1.17549435e-38f) { x *= 18446744073709551616.0f; adj = -64; }   // subnormal: scale by 2^64 (exact)
    unsigned bits = __builtin_bit_cast(unsigned, x);
    int e = (int)(bits >> 23) - 127 + adj;
    float m = __builtin_bit_cast(float, (bits & 0x007fffffu) | 0x3f800000u);   // [1, 2)
    if (m > 1.41421354f) { m *= 0.5f; e += 1; }
    const double md = (double)m;
    const double t = (md - 1.0) / (md + 1.0);
    const double t2 = t * t;
    double s = 2.0 / 13.0;
    s = s * t2 + 2.0 / 11.0;
    s = s * t2 + 2.0 / 9.0;
    s = s * t2 + 2.0 / 7.0;
    s = s * t2 + 2.0 / 5.0;
    s = s * t2 + 2.0 / 3.0;
    s = s * t2 + 2.0;
    s = s * t;
    return (float)((double)e + s * 1.4426950408889634);
}

// log10 of a positive finite float, the same bits on the host (oracle/orc_side.c orc_det_log10f) and on the device: the log2 above kept in double,
// times log10(2), rounded to float once (within half a unit in the last place of the true value but for double-rounding ties; libm's log10f and
// the device library's differ from each other in the last place).  rssi_tag_block's 10 log10f(level + 1e-20) takes it: the argument is >= 1e-20.
__host__ __device__ inline float det_log10f(float x)
{
    if (!(x > 0.0f)) return x == 0.0f ? -__builtin_inff() : __builtin_nanf("");
    if (x > 3.4028234e38f) return __builtin_inff();
    int adj = 0;
    if (x < 1.17549435e-38f) { x *= 18446744073709551616.0f; adj = -64; }
    unsigned bits = __builtin_bit_cast(unsigned, x);
    int e = (int)(bits >> 23) - 127 + adj;
    float m = __builtin_bit_cast(float, (bits & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421354f) { m *= 0.5f; e += 1; }
    const double md = (double)m;
    const double t = (md - 1.0) / (md + 1.0);
    const double t2 = t * t;
    double s = 2.0 / 13.0;
    s = s * t2 + 2.0 / 11.0;
    s = s * t2 + 2.0 / 9.0;
    s = s * t2 + 2.0 / 7.0;
    s = s * t2 + 2.0 / 5.0;
    s = s * t2 + 2.0 / 3.0;
    s = s * t2 + 2.0;
    s = s * t;
    return (float)(((double)e + s * 1.4426950408889634) * 0.30102999566398120);
}

}  // namespace qrl
