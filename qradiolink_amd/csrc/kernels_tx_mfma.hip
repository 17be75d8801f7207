// kernels_tx_mfma.hip — the gr_mod_base back-end interpolator on the f32 matrix pipe (gfx950 / CDNA4).
//
//  k_tx_interp_mfma : rational_resampler_ccf(I, 1, low_pass(I, I * 1e6, 480k, 20k, BH)), I = device rate / 1e6
//                     [gr_mod_base.cpp:215-258]; the interpolator of TxBackEnd::run (tx_common.cpp) from kTxMfmaMinInterp up.
//
// The interpolator is a matrix product:  Y[ph, c] = sum_j H[ph, j] X[c - j],  H[ph, j] = h[ph + j I],  output sample c I + ph.
//   A (32 phases x 2 lags per step)  = the tap table in the host's layout [phase tile][lag][phase in tile], zero where ph + j I >= nt and
//                                      for phase rows >= I;  lane l of step s reads float 64 s + l of the tile: one linear ds_read_b32.
//   B (2 lags x 32 columns per step) = a Toeplitz view of the rotated 1 Msps ring, B[j, c] = X[c - j]; re and im are separate planes in
//                                      LDS, so lane (k = l >> 5, col = l & 31) reads word col - k - 2 s of a plane: consecutive lanes,
//                                      consecutive words, and the two lane halves never meet on a bank (they are served separately).
//   K runs over j = 0 .. 209 ascending across the 105 chained v_mfma_f32_32x32x2_f32 of one accumulator, which starts at +0.
// On gfx950 that chain is bit for bit fmaf(h_j, x_{c-j}, acc) in ascending j, the sum of the oracle's resampler (oracle/orc_blocks.c, orc_resamp_ccf): no wider
// internal sum, one rounding per product.  The padded steps are exact on finite input: fmaf(0, x, acc) = acc, and where the oracle stops
// its chain at c - j < 0 the ring holds +0 after reset, fmaf(h, +0, acc) = acc (acc starts at +0 and zero products cannot make it -0).
// A non-finite x under a padded zero tap is NaN where the oracle never reads that lag: see device_samp_rate in qrl_hip.h.
//
// Geometry: grid = (c-chunks, stream, phase tile), 256 threads.  A workgroup stages its phase tile's 210 x 32 taps (26.25 KB) into LDS
// once and walks `cpw` blocks of 128 ring samples; per block the window c0 - 210 .. c0 + 127 of the ring goes to LDS once (re plane, im
// plane) and each of the 4 waves computes one 32 phases x 32 samples tile: 2 x 105 MFMAs, 3 ds_read_b32 per MFMA pair.
// Store: direct from the accumulators.  A lane holds, for one c, four groups of four consecutive phases = four runs of 32 contiguous
// bytes (cf32), 16 (sc16) or 8 (sc8, as four 2-byte stores); the two lane halves hold the two halves of a 64-byte run, and a wave's stores of one tile fill 32 runs of
// 256 contiguous bytes (32 phases of one c), which the L2 merges before they leave for HBM.  Partial c-tiles and phase tiles are computed
// padded and their stores predicated per element.
#include <algorithm>
#include "devmath.hpp"
#include "engine.hpp"

namespace qrl {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TXM_CB = 128;                          // ring samples per block: 4 waves x 32 columns
constexpr int TXM_WIN = TXM_CB + kTxMfmaLags;        // the block's window of the ring

template <int FMT>
__global__ __launch_bounds__(256) void k_tx_interp_mfma(const TxInterpMfmaParams P)
{
    __shared__ __align__(16) float taps_s[kTxMfmaLags * kTxMfmaPhases];
    __shared__ float xre[TXM_WIN], xim[TXM_WIN];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, pt = blockIdx.z;
    {
        const float4* tp = reinterpret_cast<const float4*>(P.taps + (size_t)pt * (kTxMfmaLags * kTxMfmaPhases));
        for (int k = tid; k < kTxMfmaLags * kTxMfmaPhases / 4; k += 256) reinterpret_cast<float4*>(taps_s)[k] = tp[k];
    }
    const float2* ring = P.in.p + (size_t)b * (P.in.mask + 1u);
    const int col = lane & 31, h = lane >> 5;
    const float* ap = taps_s + lane;
    const int bo = 32 * wave + col - h + kTxMfmaLags;   // window word of lag 0 (h = 0) / lag 1 (h = 1) of this lane's column
    const int I = P.interp;
    uint32_t nclip = 0;
    for (uint32_t i = 0; i < P.cpw; ++i) {
        const uint32_t c0 = (blockIdx.x * P.cpw + i) * (uint32_t)TXM_CB;   // this block's first sample, counted from the call's first
        if (c0 >= P.n1) break;
        __syncthreads();   // the previous block's operand reads are done (first pass: nothing to wait for)
        for (int k = tid; k < TXM_WIN; k += 256) {
            // window word k = sample n0 + c0 + k - 210; before the stream's start the index wraps to ring items that reset left at +0
            const float2 x = ring[(uint32_t)(P.n0 + c0 + (uint64_t)k - (uint64_t)kTxMfmaLags) & P.in.mask];
            xre[k] = x.x; xim[k] = x.y;
        }
        __syncthreads();
        const uint32_t cw = c0 + 32u * (uint32_t)wave;
        if (cw >= P.n1) continue;   // wave-uniform: nothing of this tile is stored
        f32x16 ar, ai;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ar[r] = 0.0f; ai[r] = 0.0f; }
#pragma unroll 21
        for (int s = 0; s < kTxMfmaLags / 2; ++s) {
            const float a = ap[64 * s];
            const float xr = xre[bo - 2 * s], xi = xim[bo - 2 * s];
            ar = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xr, ar, 0, 0, 0);
            ai = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xi, ai, 0, 0, 0);
        }
        // C/D layout: column (sample) = lane & 31, row (phase) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const uint32_t c = cw + (uint32_t)col;
        if (c < P.n1) {
            const size_t t0 = (size_t)c * (size_t)I;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ph0 = pt * kTxMfmaPhases + 8 * g + 4 * h;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (ph0 + r < I) {
                        const float2 y = make_float2(ar[4 * g + r], ai[4 * g + r]);
                        if constexpr (FMT == OUT_SC16) {
                            uint32_t nc;
                            reinterpret_cast<uint32_t*>(P.out)[(size_t)b * P.out_stride + t0 + (size_t)(ph0 + r)] = f2_to_sc16(y, P.sc.scale, nc);
                            nclip += nc;
                        } else if constexpr (FMT == OUT_SC8) {
                            uint32_t nc;
                            reinterpret_cast<uint16_t*>(P.out)[(size_t)b * P.out_stride + t0 + (size_t)(ph0 + r)] = f2_to_sc8(y, P.sc.scale, nc);
                            nclip += nc;
                        } else {
                            P.out[(size_t)b * P.out_stride + t0 + (size_t)(ph0 + r)] = y;
                        }
                    }
                }
            }
        }
    }
    if constexpr (FMT != OUT_CF32) {
        // clipped components of everything this wave stored: one atomic per wave, none when nothing clipped
        if (P.sc.clip) {
#pragma unroll
            for (int o = 32; o; o >>= 1) nclip += __shfl_xor(nclip, o);
            if (nclip && lane == 0) atomicAdd(P.sc.clip + b, nclip);
        }
    }
}

void launch_tx_interp_mfma(const TxInterpMfmaParams& p, int batch, hipStream_t s)
{
    if (!p.n1) return;
    TxInterpMfmaParams q = p;
    const uint32_t nblk = (p.n1 + TXM_CB - 1) / TXM_CB, ptiles = ((uint32_t)p.interp + kTxMfmaPhases - 1) / kTxMfmaPhases;
    // consecutive blocks per workgroup: enough to amortise the 26 KB tap load, few enough to keep ~4k workgroups
    const uint64_t total = (uint64_t)nblk * (uint64_t)batch * ptiles;
    q.cpw = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, total / 4096));
    const dim3 grid((nblk + q.cpw - 1) / q.cpw, batch, ptiles);
    const auto kern = p.sc.fmt == OUT_SC8 ? k_tx_interp_mfma<OUT_SC8> : p.sc.fmt == OUT_SC16 ? k_tx_interp_mfma<OUT_SC16> : k_tx_interp_mfma<OUT_CF32>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, q);
}

}  // namespace qrl
