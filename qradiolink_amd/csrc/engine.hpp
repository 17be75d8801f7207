// engine.hpp — device-side parameter blocks and kernel launch entry points of the RX engine.
// Every inter-kernel stream is a per-stream ring in HBM addressed by ABSOLUTE item index
// (idx & mask), so FIR history, loop state and block alignment carry across process() calls
// and results do not depend on how the caller cuts the stream into chunks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "zero_runs.hpp"   // struct ZeroRun
#include "decim_plan.hpp"  // which decimator a geometry gets, its sizes, the split of a call: host arithmetic free of HIP
#include "fsk2_tail_geo.hpp"   // k_2fsk_tail: which calls get it, its windows, rings and LDS size (HIP-free as well)

namespace qrl {

// Raises a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize).  The attribute belongs to the CURRENT
// DEVICE: it is set once per (kernel, device), from any thread; the HIP error is returned, never swallowed.
hipError_t dyn_lds_limit(const void* kernel, int bytes);
// launch_* helpers that could not set the attribute skip their launch and leave a per-thread mark; every process() entry point
// ends with take_launch_error() and turns it into QRL_ERR_HIP.
bool take_launch_error();

// A handle-internal stream, optionally confined to a set of compute units (round 6, VERDICT r5 #4: partition the chip in SPACE).
// QRL_CU_<ROLE>="first:count" (CUs PER XCD, 32 each on MI355X) turns the stream of that role into a CU-masked one
// (hipExtStreamCreateWithCUMask); unset = hipStreamCreateWithPriority as before.  Mask bit i = CU (i / 8) of XCD (i % 8): the driver
// deals the bits of a queue's mask round-robin over the XCDs, so a per-XCD range [first, first + count) is bits 8 * first ... 8 * (first + count) - 1.
// A masked stream has a hardware queue of its own (the mask is a queue property), so it cannot share one with another stream of the handle.
int create_role_stream(hipStream_t* s, int priority, const char* role);

struct RingC { float2* p; uint32_t mask; };   // complex ring, stream stride = mask+1 items
struct RingF { float* p; uint32_t mask; };
struct RingB { uint8_t* p; uint32_t mask; };
// item i of stream b; an item in front of the stream start is zero
__device__ __forceinline__ float2 ringc_at(const RingC& r, int b, int64_t i)
{
    if (i < 0) return make_float2(0.f, 0.f);
    return r.p[(size_t)b * (r.mask + 1u) + ((uint32_t)i & r.mask)];
}
__device__ __forceinline__ float ringf_at(const RingF& r, int b, int64_t i)
{
    if (i < 0) return 0.f;
    return r.p[(size_t)b * (r.mask + 1u) + ((uint32_t)i & r.mask)];
}

// ---- per-stream rotator (qrl_*_set_carrier_offsets) ----
// A parameter block with rot_acc_s != nullptr carries one NCO per stream: stream b's (acc, inc) are rot_acc_s[b], rot_inc_s[b] and its fine
// table is rot_lo + 512 b; rot_nbase stays shared.  Kernels take the form as a template flag PS and launchers pick it from the pointer, so a
// handle that never had per-stream offsets launches the shared-form code (PS = false) unchanged.  ROT_VIEW(T, PS, P, SRC, b) declares
// `const T& P`: SRC itself for PS = false, a copy of SRC with stream b's rotator in the shared fields for PS = true.
template <class Pp>
__device__ __forceinline__ void rot_select(Pp& c, const Pp& p, uint32_t b)
{
    c = p; c.rot_acc = p.rot_acc_s[b]; c.rot_inc = p.rot_inc_s[b]; c.rot_lo = p.rot_lo + (size_t)b * 512;
}
#define ROT_VIEW(T, PS, P, SRC, B) T P##_ps_; if constexpr (PS) rot_select(P##_ps_, SRC, (uint32_t)(B)); const T& P = (PS) ? P##_ps_ : SRC
// host side: struct Rotator (host_common.hpp) owns the arrays
std::vector<float2> rot_fine_table(uint64_t inc);   // the 512-entry fine table of an increment (sincos_turn_host)
void launch_rot_ps_advance(uint64_t* acc, const uint64_t* inc, int B, uint64_t delta, hipStream_t s);
void launch_rot_ps_fill(uint64_t* acc, uint64_t* inc, float2* lo, int B, int set_acc, uint64_t acc0, uint64_t inc0, const float2* lo0, hipStream_t s);

// ---- format of the caller's IQ (qrl_demod_process / qrl_demod_process_sc16) ----
// IN_SC16: `in` points at interleaved int16 I, Q pairs (4 bytes per sample, in_stride still in samples) and a sample is
// x = (float)v * in_scale per component: one exact int -> float conversion, one rounded multiply, in front of the rotator.  Only the kernels
// that read the caller's buffer know the format (the front-end stage -- without a front end, under QRL_OPT_SC16_BASEBAND, the mode's first stage and the
// scope tap -- and k_hist); history, edge scratch and rings stay rotated cf32.
// IN_SC8 / IN_CU8 (qrl_demod_process_sc8 / _cu8; handles with a front end, or a 1 Msps handle under QRL_OPT_IQ8_BASEBAND): `in` points at interleaved 8-bit I, Q pairs, 2 bytes per sample.
// ONE device path serves both: u = byte ^ mask (0x80 for sc8, 0 for cu8), x = ((float)u - in_bias) * in_scale -- one exact conversion, one f32
// subtract, one rounded f32 multiply.  (float)(uint8_t)(v ^ 0x80) - 128.0f == (float)v exactly for every int8 v, so the host hands sc8 the bias 128
// and the result is (float)v * scale; for cu8 the bias is the caller's (default 127.5).
enum { IN_CF32 = 0, IN_SC16 = 1, IN_SC8 = 2, IN_CU8 = 3 };
enum { IN_W_CF32 = 0, IN_W_SC16 = 1, IN_W_IQ8 = 2 };   // sample width class: what the kernels with an instantiation per format are instantiated on
__device__ __forceinline__ float2 sc16_to_f2(uint32_t w, float scale)
{
    return make_float2((float)(int16_t)(w & 0xffffu) * scale, (float)((int32_t)w >> 16) * scale);
}
__device__ __forceinline__ uint32_t iq8_mask(int fmt) { return fmt == IN_SC8 ? 0x8080u : 0u; }   // wave uniform
// the 16-bit word of one 8-bit sample (I in the low byte), any upper bits ignored
__device__ __forceinline__ float2 iq8_to_f2(uint32_t w, uint32_t mask, float bias, float scale)
{
    const uint32_t u = w ^ mask;
    return make_float2(((float)(u & 0xffu) - bias) * scale, ((float)((u >> 8) & 0xffu) - bias) * scale);
}
// sample r of stream b of the caller's buffer of a parameter block (DecimParams, HistParams), converted.  in_load: the format read from
// the block (the checked per-sample paths); in_load_as<W>: the width class a compile-time value (kernels that have an instantiation per format,
// so that their cf32 code stays what it was); a block without in_bias (ChanParams) is never instantiated with IN_W_IQ8
template <class Pp, class = void> struct in_has_iq8 { static constexpr bool value = false; };   // blocks with an in_bias take 8-bit pairs (ChanParams: cf32 and int16 only)
template <class Pp> struct in_has_iq8<Pp, decltype((void)Pp::in_bias)> { static constexpr bool value = true; };
template <class Pp>
__device__ __forceinline__ float2 in_load(const Pp& P, size_t b, size_t r)
{
    if (P.in_fmt == IN_SC16) return sc16_to_f2(reinterpret_cast<const uint32_t*>(P.in)[b * P.in_stride + r], P.in_scale);
    if constexpr (in_has_iq8<Pp>::value) if (P.in_fmt >= IN_SC8) return iq8_to_f2(reinterpret_cast<const uint16_t*>(P.in)[b * P.in_stride + r], iq8_mask(P.in_fmt), P.in_bias, P.in_scale);
    return P.in[b * P.in_stride + r];
}
template <int W, class Pp>
__device__ __forceinline__ float2 in_load_as(const Pp& P, size_t b, size_t r)
{
    if constexpr (W == IN_W_IQ8) return iq8_to_f2(reinterpret_cast<const uint16_t*>(P.in)[b * P.in_stride + r], iq8_mask(P.in_fmt), P.in_bias, P.in_scale);
    else if constexpr (W == IN_W_SC16) return sc16_to_f2(reinterpret_cast<const uint32_t*>(P.in)[b * P.in_stride + r], P.in_scale);
    else return P.in[b * P.in_stride + r];
}

// ---- format of the caller's TX buffer (qrl_*_process / qrl_*_process_sc16 / qrl_*_process_sc8) ----
// fmt = OUT_CF32 (0, what a zeroed block means): `out` is float2.  OUT_SC16: `out` points at packed int16 I, Q pairs (4 bytes per sample, out_stride
// still in samples) and the terminal kernel stores through sc16_store (devmath.hpp).  OUT_SC8: int8 I, Q pairs (2 bytes per sample, rows 2-byte aligned
// only) through sc8_store, one 2-byte store per sample.  clip = nullptr or the caller's [batch] counters of clipped components of that format.
// Kernels take the format as a template parameter and launchers pick it from `fmt`, so the cf32 and sc16 instantiations keep their code.
enum { OUT_CF32 = 0, OUT_SC16 = 1, OUT_SC8 = 2 };
struct TxOut { int fmt; float scale; uint32_t* clip; };

// ---- K1: rotator + decimating FIR (rotator_cc + rational_resampler_ccf(1,D)) ----
struct DecimParams {
    const float2* in; size_t in_stride;  // caller IQ (or nullptr when in_ring is used); in_fmt below says what it points at
    RingC in_ring;                       // alternative input: an engine ring (second-stage decimators)
    uint64_t n0; uint32_t n;             // absolute index of in[0], samples in this call
    float in_bias;                       // IN_SC8 / IN_CU8: x = ((float)u - in_bias) * in_scale (in what was padding: no other field moves)
    const float2* hist; uint32_t hist_len;  // last hist_len (rotated) samples before n0, per stream
    RingC out;
    uint64_t m0; uint32_t m_count;       // absolute first output, number of outputs
    const float* taps;                   // [D][Jpad], taps[p*Jpad + j] = h[p + j*D], zero padded
    int D, Jpad;
    int rot_enable; uint64_t rot_acc; uint64_t rot_inc; uint64_t rot_nbase; const float2* rot_lo;
    uint32_t tiles;                      // tiles per stream
    // MFMA variant (kernels_decim_mfma.hip): banded-Toeplitz A operands [S steps][64 lanes], S steps of 4
    const float* gtab; int S; int nt; uint32_t magic_blk, magic_seg;   // gtab: zero-padded taps, hp[k + 4S - nt + 1] = h[k]
    uint32_t tpw, nchunks; int nhi; int dbg;               // consecutive tiles per workgroup; rotator coarse-table entries
    int nld;                                                // 16-byte loads per thread a tile needs (<= the kernel's NLD)
    int hist_raw;                                           // hist holds UN-rotated samples (MFMA variant only): rotate on fetch
    uint32_t out_row_mul_m1, out_row_add;                   // output ring row of stream b = b * (mul_m1 + 1) + add (MFMA / phase-lane variants)
    // phase-lane variant (kernels_decim_pl.hip): lane tap table [J][64]; the launcher fills the segment geometry
    const float* pl_taps; int pl_J; uint32_t pl_S, pl_nseg, pl_batch; uint64_t pl_m_begin, pl_m_end;
    int pl_E, pl_R; const float* pl_hraw;                   // samples per lane and block, outputs per block; raw taps h[k] (k_decim_pl_gen)
    // edge segment (outputs whose window starts in front of this call's buffer): per-stream scratch of ROTATED samples (carried
    // history + head of the buffer), one extra unit per stream behind the regular ones reads it with identity phasors
    float2* pl_edge; uint32_t pl_edge_stride, pl_edge_cap; uint64_t pl_edge_ms, pl_edge_me;
    // host side only: when set, the edge scratch is staged on THIS stream (k_pl_edge_stage reads the caller's buffer and the carried history,
    // nothing the call before produces on the launch stream), `pre_event` is recorded behind it and the launch stream waits for that
    hipStream_t pre_stream; hipEvent_t pre_event;
    const uint64_t* rot_acc_s; const uint64_t* rot_inc_s;   // per-stream rotator (see rot_select below), or nullptr: the shared one above
    int in_fmt; float in_scale;                             // IN_CF32 (0, what a zeroed block means) | IN_SC16 | IN_SC8 | IN_CU8 and its scale
};
// the format of one call as the host hands it to a parameter block (DecimParams, HistParams)
struct InFormat { int fmt; float scale, bias; };
template <class Pp> inline void in_format_fill(Pp& p, const InFormat& f) { p.in_fmt = f.fmt; p.in_scale = f.scale; p.in_bias = f.bias; }
struct HistParams {
    const float2* in; size_t in_stride; uint64_t n0; uint32_t n;
    float in_bias;                       // as in DecimParams, in what was padding
    const float2* hist_old; float2* hist_new; uint32_t hist_len;
    int rot_enable; uint64_t rot_acc; uint64_t rot_inc; uint64_t rot_nbase; const float2* rot_lo;
    const uint64_t* rot_acc_s; const uint64_t* rot_inc_s;
    int in_fmt; float in_scale;
};
void launch_decim(const DecimParams& p, int batch, int variant, hipStream_t s);
// 1:2 decimator + the channel FIR behind it in one kernel (kernels_frontend.hip k_dec2_fir): d = the decimator's input side (out unused)
struct Dec2FirParams { DecimParams d; const float* taps; RingC out; float2* port; size_t port_cap; uint32_t* counts; };
bool dec2_fir_supported(int nt1, int D, int nt2);
uint32_t dec2_fir_lookback();
std::vector<float> dec2_fir_table(const std::vector<float>& h1, const std::vector<float>& h2);
void launch_dec2_fir(const Dec2FirParams& p, int batch, hipStream_t s);
void launch_hist_save(const HistParams& p, int batch, hipStream_t s);
// f32-MFMA decimator (D >= 8): contract "m16" of oracle/orc_blocks.c
int launch_decim_mfma(const DecimParams& p, int batch, hipStream_t s);   // 0, or -1 when the kernel attribute could not be set
void decim_mfma_prof_read(unsigned long long* out8);
void decim_mfma_prof_enable(int on);
// register-resident phase-lane decimator (32 < D <= 64, <= 16 taps per phase): contract "pl" of oracle/orc_blocks.c
std::vector<float> decim_pl_layout(const std::vector<float>& h, int D);
int launch_decim_pl(const DecimParams& p, int batch, hipStream_t s);
// phase-major matrix-pipe decimator (32 < D <= 52, <= 16 taps per phase): contract "pm" of oracle/orc_blocks.c
std::vector<float> decim_pm_layout(const std::vector<float>& h, int D);
int launch_decim_pm(const DecimParams& p, int batch, hipStream_t s);

// ---- K2: rational resampler I/D on a ring (optionally with rotator on a caller buffer) ----
struct ResampParams {
    const float2* in; size_t in_stride; uint64_t n0; uint32_t n;  // caller IQ path (rotator-only front end)
    int in_fmt;                           // ... IN_CF32 (0) | IN_SC16: what `in` points at (qrl_chan_process_sc16, single carrier); in what was padding, as in ChanParams
    const float2* hist; uint32_t hist_len;
    float in_scale;
    RingC in_ring;                        // ring path
    RingC out;
    uint64_t q0; uint32_t q_count;        // outputs to produce
    float in_bias;                        // IN_SC8 / IN_CU8: x = ((float)u - in_bias) * in_scale (in what was padding: no other field moves)
    const float* taps;                    // [I][Jp]: taps[ph*Jp + j] = h[ph + j*I]
    int I, D, Jp;
    int rot_enable; uint64_t rot_acc; uint64_t rot_inc; uint64_t rot_nbase; const float2* rot_lo;
    float2* port; size_t port_cap; uint32_t* port_counts;   // optional copy of this call's outputs to a caller port (counts[b*4+0])
    const uint64_t* rot_acc_s; const uint64_t* rot_inc_s;
};
void launch_resamp(const ResampParams& p, int batch, hipStream_t s);

// ---- small feed-forward kernels at the decimated rate ----
struct FirCcfParams { RingC in; RingC out; uint64_t q0; uint32_t count; const float* taps; int nt;
                      float2* port; size_t port_cap; uint32_t* counts; };  // optional copy to a caller port buffer; counts[b*4+0]
struct FirFffParams { RingF in; RingF out; uint64_t q0; uint32_t count; const float* taps; int nt; };
struct QuadDemodParams { RingC in; RingF out; uint64_t q0; uint32_t count; float gain; const float* atan_tab;
                         RingF out2; float gain2;      // out2.p != nullptr: a second discriminator with its own gain on the same input (C4: MMDVM FM path + 4FSK tail)
                         int16_t* s16; size_t s16_cap; float s16_level, s16_scale; uint32_t* s16_counts; };   // s16 != nullptr: + multiply_const_ff(level) + float_to_short(scale) of `out` (k_f2s fused)
struct Disc2fskParams { RingC in; RingF out; uint64_t q0; uint32_t count; const float2* up; const float2* lo; int nt; };
struct Disc4fskParams { RingC in; RingC out; uint64_t q0; uint32_t count; const float2* taps; int nt; };   // taps[4][nt]
void launch_disc_4fsk(const Disc4fskParams& p, int batch, hipStream_t s);
struct Fsk2FfParams { RingC in; RingF out; uint64_t q0; uint32_t count;
                      const float* tf; int nf; const float2* up; const float2* lo; int nb; const float* ts; int ns;
                      float2* port; size_t port_cap; uint32_t* counts; };
void launch_2fsk_ff(const Fsk2FfParams& p, int batch, hipStream_t s);   // nf/nb/ns and the tables zero padded: fsk2_ff_padded()
int fsk2_ff_padded(int n);
void launch_fir_ccf(const FirCcfParams& p, int batch, hipStream_t s);
void launch_fir_fff(const FirFffParams& p, int batch, hipStream_t s);
void launch_quad_demod(const QuadDemodParams& p, int batch, hipStream_t s);
void launch_disc_2fsk(const Disc2fskParams& p, int batch, hipStream_t s);

// ---- serial loops, one lane per stream ----
struct FllState { float phase, freq; float2 dl[32]; };
struct FllParams { RingC in; RingC out; uint64_t q0; uint32_t count; FllState* st;
                   const float2* lower; const float2* upper; int nt; float alpha, beta, max_freq;
                   int slim; };   // 1: single-wave workgroups with a 16-sample window (3 KB LDS): fits beside a CU full of front-end workgroups (overlapped mode)
void launch_fll(const FllParams& p, int batch, hipStream_t s);
// k_fll<16> + k_2fsk_ff<11, 11, 7> as one wave-specialised kernel (kernels_2fsk_tail.hip; which calls get it: fsk2_tail_eligible).  fll.out is
// unused; ff.in is the r2l ring, of which the kernel reads the 104 items in front of q0 and writes the call's last windows of y
struct Fsk2TailParams { FllParams fll; Fsk2FfParams ff; };
void launch_2fsk_tail(const Fsk2TailParams& p, int batch, hipStream_t s);
size_t fsk2_tail_lds_bytes();

struct SymSyncState { uint64_t ii; uint64_t oo; float mu, avg, inst; float x0, x1, x2, d0, d1, d2; };
struct SymSyncParams {
    RingF in; uint64_t avail;              // samples available (absolute count)
    RingB soft;                            // soft symbols out (absolute symbol index)
    SymSyncState* st;
    const float* mmse;                     // 129 x 8
    float alpha, beta, maxp, minp;
    int ted; float soft_mul, soft_add;
    int slicer;                            // 0: bpsk sign, 1: constellation_rect{-1.5,-0.5,0.5,1.5}
    float tail_scale;                      // tail 1: _level_control in front of the phase modulator (0.9 gr_demod_dmr, 1 gr_demod_m17)
    int tail;                              // 0: soft symbols for the Viterbi; 1: DMR / M17 tail (x scale, phase_modulator, slicer, map) -> bits port;
                                           // 2: native 4FSK (FM) tail: phase_modulator -> (imag, real) soft pairs for the Viterbi
    uint8_t* bits; size_t bits_cap;        // tail 1: two bits per symbol, counts[b*4+2]
    float2* port; size_t port_cap; uint32_t* counts;  // constellation port (this call), counts[b*4+1]
    int slim;                              // 1: the <16 streams, 96-sample window> geometry, 25 KB of LDS (multi-carrier receiver)
};
void launch_symsync_ff(const SymSyncParams& p, int batch, hipStream_t s);

// ---- QPSK recursive chain (agc2 -> costas -> symbol_sync_cc -> costas -> diff_phasor -> rotate), one lane per stream ----
struct QpskState {
    uint64_t ii, oo;                 // symbol-sync read cursor (absolute sample), symbols produced
    float gain;                      // agc2
    float c1_phase, c1_freq;         // first Costas loop (sample rate)
    float mu, avg, inst;             // clock tracking loop
    float2 x0, x1, x2, d0, d1, d2;   // TED history
    float c2_phase, c2_freq;         // second Costas loop (symbol rate)
    float2 dprev;                    // diff_phasor
    float2 hist[16];                 // last 16 outputs of the first Costas loop
};
struct QpskParams {
    RingC in; uint64_t np0, avail;   // RRC-filtered input ring; samples processed before this call / available now
    RingB soft; QpskState* st;
    const float* mmse; const float* tanh_tab;
    float c1_alpha, c1_beta, c2_alpha, c2_beta;
    float ss_alpha, ss_beta, ss_maxp, ss_minp;
    float2 rot; float soft_mul, soft_add;
    int mode;                        // 0: gr_demod_qpsk chain; 1: gr_demod_bpsk chain (agc2 -> clock_recovery_mm_cc -> costas order 2);
                                     // 2: symbol_sync_cc alone on the 4-level rect constellation (gr_demod_4fsk non-FM branch)
    float cr_gain_omega, cr_gain_mu, cr_omega_mid, cr_omega_lim;   // mode 1
    float2* port; size_t port_cap; uint32_t* counts;   // constellation port (this call), counts[b*4+1]
    uint64_t* oo_snap;               // [batch] symbols produced up to the end of this call (what this call's decoder may consume)
};
void launch_qpsk_loops(const QpskParams& p, int batch, hipStream_t s);

// ---- FEC tail: K=7 r=1/2 Viterbi (spiral-kernel semantics) + descrambler ----
struct FecState { uint64_t consumed; uint32_t start_state; uint32_t last_bits; };
struct FecParams {
    RingB soft; const uint64_t* avail; size_t avail_stride; uint32_t avail_mul;   // available soft symbols of stream b = *(avail + b*stride bytes) * mul
    FecState* st;                          // [batch][2]
    uint8_t* bits_a; uint8_t* bits_b; size_t bits_cap; uint32_t* counts;  // counts[b*4+2], [b*4+3]
    int branches;
};
void launch_fec(const FecParams& p, int batch, hipStream_t s);
void launch_fec_gate(unsigned us, hipStream_t s);

// ---- gr_dmr_dmo_sink on the device (kernels_dmo.hip): correlator slicer behind port 3 of gr_demod_dmr ----
struct DmoState {
    uint32_t bitBuffer[5];
    uint16_t syncPtr, startPtr, endPtr, pad0;
    float maxCorr, centre[4], threshold[4];
    uint8_t averagePtr, syncCount, state, control, n, colorCode, pad1[2];
};
struct DmoParams { RingF in; uint64_t q0; uint32_t count; DmoState* st; const uint32_t* golay; uint8_t* out; uint32_t cap; uint32_t* counts; };
void launch_dmo_sink(const DmoParams& p, int batch, hipStream_t s);
std::vector<uint32_t> golay1987_table();

// ---- gr_deframer_bb on the device (kernels_deframe.hip) ----
struct DeframeState { uint32_t reg, found, idx, pad; };
struct DeframeParams {
    const uint8_t* bits; size_t stride; uint32_t n;          // unpacked bits [batch][stride]; n valid per stream unless counts != NULL
    const uint32_t* counts; size_t count_stride;             // device-side valid counts: counts[b * count_stride]
    int type; uint32_t buf_len; DeframeState* st;
    uint8_t* out; size_t out_cap; uint32_t* out_counts;
};
void launch_deframe(const DeframeParams& p, int batch, hipStream_t s);
struct FrameSyncState { uint32_t reg, found, idx, ftype, modem_sync, pad[3]; };
struct FrameSyncParams {
    const uint8_t* bits; size_t stride; uint32_t n; const uint32_t* counts; size_t count_stride;
    int cls; uint32_t bit_buf_len, frame_length;           // sync-word class (0: 1k modes, 1: fast modes, 2: rest), mode table
    FrameSyncState* st; uint8_t* bitbuf; size_t bitbuf_stride;
    uint8_t* out; size_t out_cap; uint32_t* out_counts;    // records; out_counts[2b] = bytes, [2b + 1] = frames
    uint32_t* activity;                                    // optional [batch]: bits collected into a frame while a sync was held, this call
};
void launch_framesync(const FrameSyncParams& p, int batch, hipStream_t s);

// ---- multi-carrier MMDVM RX (kernels_chan.hip) ----
struct ChanParams {
    const float2* in; size_t in_stride; uint64_t n0; uint32_t n;   // wideband caller IQ of this call (n multiple of M)
    int in_fmt;                                                    // IN_CF32 (0, what a zeroed block means) | IN_SC16: what `in` points at (history stays cf32)
    const float2* hist; uint32_t hist_len;                         // last hist_len samples before n0
    float in_scale;                                                // IN_SC16: x = (float)v * in_scale.  (Both sit in what was padding: the offsets of every other field,
                                                                   // and so the kernel-argument loads of the cf32 kernels, are those of the block without them)
    RingC out; uint64_t m0; uint32_t m_count;                      // channel rings [batch * c_count], output instants
    const float* taps; const float2* twiddle;                      // taps[p + M k] zero padded to J*M; W[q] = e^{+j 2 pi q / M}
    int M, J, c_first, c_count;
    int legacy;                 // qrl_chan_set_option(QRL_CHAN_OPT_LEGACY_PFB), tests: 1 = the general-M kernel also for M = 64
    // row_cpd > 0: output rows grouped by destination rank -- row = ((cc / row_cpd) * batch + b) * row_cpd + cc % row_cpd
    // (the send layout of an all-to-all that gives rank r the channels [r row_cpd, (r + 1) row_cpd) of every stream);
    // out_pitch > 0: linear rows of out_pitch items, item m - m0 (a caller buffer instead of an engine ring)
    uint32_t row_cpd; size_t out_pitch;
};
struct F2sParams { RingF in; uint64_t q0; uint32_t count; float level, scale; int16_t* out; size_t cap; uint32_t* counts; };
struct RssiParams { RingC in; uint64_t j0; uint32_t count; float calibration; float* out; size_t cap; uint32_t* counts; };
void launch_rssi_tag(const RssiParams& p, int batch, hipStream_t s);
// the per-channel chain of gr_demod_mmdvm_multi2 behind the channelizer as one kernel (kernels_chan_tail.hip): 24/25 resampler,
// channel filter, RSSI tags, FM discriminator -> int16, and the symbol demodulator's discriminator + RRC into the symbol-sync ring
struct ChanTailParams {
    RingC in;                               // channel ring at 25 ksps, one row per (stream, channel)
    // form 3 (round 5): the call's channel samples where the exchange put them, lin[row * lin_pitch + (a - lin_base)] for absolute items
    // a in [lin_base, lin_base + lin_n), and the hist_len items in front of them in hist[row * hist_len + ...] (k_hist keeps them from call to
    // call) -- no copy into a ring.  lin == nullptr: the ring.
    const float2* lin; size_t lin_pitch; uint64_t lin_base; uint32_t lin_n; const float2* hist; uint32_t hist_len;
    uint64_t q0; uint32_t count;            // outputs of this call at 24 ksps: [q0, q0 + count)
    const float* tab_a; const float* tab_b; const float* tab_e;   // step-major tap tables (chan_tail_tables; tab_e unused when out_sym.p == nullptr)
    const float* atan_tab;                  // 257
    float gain, gain2, level, scale;
    int16_t* s16; size_t s16_cap; uint32_t* s16_counts;
    RingF out_sym;                          // RRC output (symbol sync input); p == nullptr: no symbol tail
    float* rssi; size_t rssi_cap; uint32_t* rssi_counts; float rssi_cal; uint64_t tag0; uint32_t ntags;
};
void launch_chan_tail(const ChanTailParams& p, int streams, hipStream_t s);
bool chan_tail_supported(int rs_I, int rs_D, int rs_Jp, int filt_nt, int rrc_nt);
std::vector<float> chan_tail_tables(int which, const float* taps);   // 0: resampler (phase-major taps [24][35]), 1: channel filter, 2: RRC
uint32_t chan_tail_lookback();
void launch_pfb_chan(const ChanParams& p, int batch, hipStream_t s);
void launch_ring_store(RingC in, uint64_t q0, uint32_t count, float2* out, size_t cap, uint32_t* counts, int rows, hipStream_t s);
void launch_ring_load(const float2* in, size_t pitch, RingC out, uint64_t q0, uint32_t count, int rows, hipStream_t s);
void launch_f2s(const F2sParams& p, int batch, hipStream_t s);
size_t chan_lds_bytes(int M, int J);
// ---- multi-carrier MMDVM TX (kernels_chan.hip) ----
struct S2fInParams { const int16_t* in; size_t in_stride; RingF out; uint64_t q0; uint32_t count; float scale, level; };
struct SynthParams {
    RingC in; int nch;                                   // channel rings [batch * nch] at 25 ksps
    int port_chan[16];                                   // port p <- channel ring port_chan[p], -1 = idle port
    uint64_t blk0; uint32_t nblk;                        // absolute first block, blocks of this call
    const float* taps; const float2* twiddle; int M, J;  // taps[i + M j] zero padded to J*M; W[q] = e^{+j 2 pi q / M}
    float level, bb_gain;
    float2* out; size_t out_stride, out_cap;
    TxOut sc;
};
void launch_s2f_in(const S2fInParams& p, int streams, hipStream_t s);
void launch_scale_c(RingC r, uint64_t q0, uint32_t count, float k, int streams, hipStream_t s);
void launch_zero_runs(RingC r, const ZeroRun* runs, uint32_t nruns, uint64_t lo, uint64_t hi, hipStream_t s);   // gr_zero_idle_bursts
void launch_pfb_synth(const SynthParams& p, int batch, hipStream_t s);
// items [q0, q0 + count) of every ring row, converted, to out[row * out_stride + t] (qrl_synth single carrier: the resampler's ring -> the caller's sc16 or sc8 buffer)
void launch_ring_store_fmt(RingC in, uint64_t q0, uint32_t count, void* out, size_t out_stride, TxOut sc, int rows, hipStream_t s);
size_t synth_lds_bytes(int M, int J);

// ---- TX: gr_mod_qpsk (kernels_tx.hip) ----
struct TxState { uint32_t sr, enc, prev, pad; };   // scrambler register, last 6 scrambled bits, last differential symbol
struct TxBitsParams {
    const uint8_t* bytes; size_t stride; uint32_t nbytes; uint32_t L;   // L bits per lane (multiple of 32)
    uint8_t tl_pow[6][8];                                                // T^(L 2^d), d = 0..5, of the zero-input scrambler: column masks
    int mode;                                                            // 0: QPSK differential symbols, 1: coded bits (2 per input bit)
    TxState* st; RingB sym; uint64_t s0;                                 // symbol ring, absolute index of this call's first symbol
};
struct TxInterpParams {
    RingB sym; uint64_t n0; uint32_t count;      // absolute first output sample, outputs of this call
    const float* taps; int nt; int interp; float2 table[4]; float amp, bb_gain;
    float2* out; size_t out_stride;
    TxOut sc;
};
struct TxShapeParams { RingB sym; RingF out; uint64_t n0; uint32_t count; int sps; const float* taps; int nt;   // nt = 0: repeat
                       int levels; float scale; };   // levels 2 | 4; scale 0 = none
struct TxFmParams { RingF in; RingC out; uint64_t n0; uint32_t count; float k, amp; float* phase; };
struct TxInterpCParams { RingC in; uint64_t n0; uint32_t count; const float* taps; int nt; int interp; float2* out; size_t out_stride;
                         int decim; RingC out_ring; TxOut sc; };   // out_ring.p != nullptr: the samples go to ring item n0 + t instead of out (gr_mod_am: a filter follows)   // decim > 1: rational_resampler_ccf(interp, decim) (gr_mod_m17: 125 / 3)
// k_tx_interp_mfma (kernels_tx_mfma.hip): the back-end interpolator on the f32 matrix pipe.  taps: the layout of tx_mfma_taps (tx_common.cpp),
// [phase tile][lag][phase in tile], kTxMfmaLags x kTxMfmaPhases floats per tile, zero where ph + lag I >= nt and for phases >= I.
// in: the rotated 1 Msps ring; sample n0 + c of it, c < n1, gives outputs c I .. c I + I - 1 of this call in out (cf32, sc16 or sc8 by sc.fmt).
constexpr int kTxMfmaPhases = 32, kTxMfmaLags = 210;   // an MFMA tile's rows; lags per phase of low_pass(I, I * 1e6, 480k, 20k, BH) (209 or 210), even
struct TxInterpMfmaParams { RingC in; uint64_t n0; uint32_t n1; const float* taps; int interp; uint32_t cpw;   // cpw: blocks per workgroup (launcher)
                            float2* out; size_t out_stride; TxOut sc; };
void launch_tx_interp_mfma(const TxInterpMfmaParams& p, int batch, hipStream_t s);
void launch_tx_spread(RingB coded, RingB chips, uint64_t c0, uint32_t ncoded, int batch, hipStream_t s);   // gr_mod_dsss: Barker-13 spreading
void launch_tx_f2c(RingF in, RingC out, uint64_t n0, uint32_t count, float g, int batch, hipStream_t s);
void launch_tx_raw_dibits(const uint8_t* bytes, size_t stride, uint32_t nbytes, RingB sym, uint64_t s0, int batch, hipStream_t s);
struct TxRotParams { const float2* in; size_t in_stride; uint64_t n0; uint32_t count; uint64_t rot_acc, rot_inc, rot_nbase; const float2* rot_lo;
                     RingC out_ring; float2* out; size_t out_stride; const uint64_t* rot_acc_s; const uint64_t* rot_inc_s; TxOut sc; };
void launch_tx_rot(const TxRotParams& p, int batch, hipStream_t s);
void launch_tx_shape(const TxShapeParams& p, int batch, hipStream_t s);
void launch_tx_fm(const TxFmParams& p, int batch, hipStream_t s);
void launch_tx_interp_c(const TxInterpCParams& p, int batch, hipStream_t s);
void launch_tx_qpsk_bits(const TxBitsParams& p, int batch, hipStream_t s);
void launch_tx_interp(const TxInterpParams& p, int batch, hipStream_t s);

// ---- DSSS mode (kernels_dsss.hip) ----
struct DsssState { float phase, freq, gain, pad; };
struct DsssLoopParams { RingC in, out; uint64_t q0; uint32_t count; DsssState* st; const float* tanh_tab; float alpha, beta; };
void launch_dsss_loop(const DsssLoopParams& p, int mode, int batch, hipStream_t s);   // 0: costas(order 2, snr), 1: agc2(0.1, 0.1)
struct DsssMfParams { RingC in, out; uint64_t i0; uint32_t count; const float* taps; };
void launch_dsss_mf(const DsssMfParams& p, int batch, hipStream_t s);
struct DsssTailState { uint64_t ii, oo; float mu, omega, phase, freq; float2 p0, p1, p2, c0, c1, c2; };
struct DsssTailParams { RingC in; uint64_t avail; RingB soft; DsssTailState* st; const float* mmse;
                        float gain_omega, gain_mu, omega_mid, omega_lim, alpha, beta;
                        float2* port; size_t port_cap; uint32_t* counts; };
void launch_dsss_tail(const DsssTailParams& p, int batch, hipStream_t s);

// ---- analogue voice receivers (kernels_analog.hip) ----
constexpr int AN_MAX_RAMP = 1024;
struct FirCccParams { RingC in, out; uint64_t q0; uint32_t count; const float2* taps; int nt; float2* port; size_t port_cap; uint32_t* counts;
                      TxOut sc; };   // sc.fmt != OUT_CF32: `port` is the caller's sc16 / sc8 buffer (gr_mod_am's channel filter as the terminal kernel)
void launch_an_fir_ccc(const FirCccParams& p, int batch, hipStream_t s);
// g / g_prev: items that passed the gating squelch up to the end of this / the previous call
struct AnState { double pwr, iir_y, de_y; uint64_t g, g_prev; float2 prev; float iir_x, de_x, gain, env; int state, ramped; };
struct AnGateParams { RingC in; RingF out; RingC outc; uint64_t q0; uint32_t count; AnState* st; const float* atan_tab; const float* env; int ramp;
                      double alpha, one_minus_alpha, threshold; float gain, attack, decay, ref, clip; double ff0, ff1, fb1; };
void launch_an_gate(const AnGateParams& p, int kind, int batch, hipStream_t s);   // kind 0 NBFM, 1 AM, 2 WBFM, 3 SSB (complex out)
struct AnResampParams { RingF in, out; const AnState* st; const float* taps; int nt, I, D; float* port; size_t port_cap; uint32_t* counts;
                        uint64_t q0; uint32_t count; };   // st == nullptr: outputs q0 .. q0 + count (host-side counts: the TX chains)
void launch_an_resamp(const AnResampParams& p, uint32_t max_out, int batch, hipStream_t s);
// analog::ctcss_squelch_ff between the audio resampler and the audio filter (gr_demod_nbfm::set_ctcss, gr_demod_nbfm.cpp:59-60,97-123):
// per stream the three Goertzel filters, the squelch_base state machine and the count of items that passed the gate (g2)
struct CtcssState { float d1[3], d2[3]; int processed, mute, state, ramped; double env; uint64_t g2, g2_prev; };
struct CtcssParams { RingF in, out; const AnState* st; CtcssState* cs; int I, D; float wr[3], wi[3]; double level; int len, ramp; const double* env; };
void launch_an_ctcss(const CtcssParams& p, int batch, hipStream_t s);
struct AnFirParams { RingF in, out; const AnState* st; const float* taps; int nt, I, D; float* port; size_t port_cap; uint32_t* counts;
                     const CtcssState* cs; };   // cs != nullptr: the call's output range is the CTCSS gate's (g2_prev .. g2)
void launch_an_fir(const AnFirParams& p, uint32_t max_out, int batch, hipStream_t s);
struct AnDeemphParams { RingF in; AnState* st; int I, D; double ff0, ff1, fb1; float* port; size_t port_cap; uint32_t* counts; const CtcssState* cs; };
void launch_an_deemph(const AnDeemphParams& p, int batch, hipStream_t s);
// I == 0 in AnFirParams / AnStretchParams: the output range of the call is the cessb stretcher's, 1024 floor((g - 2) / 1024)
// analogue modulators (gr_mod_nbfm): linear audio -> ring; x gain -> two-tap IIR in double (lane per stream)
struct AmAgcParams { RingF in, out; uint64_t n0; uint32_t count; float attack, decay, ref, max_gain, lo, hi, scale; float* gain; };   // gr_mod_am: agc2_ff -> rail_ff -> multiply_const_ff
void launch_am_agc_rail(const AmAgcParams& p, int batch, hipStream_t s);
void launch_am_carrier(RingF in, RingC out, uint64_t n0, uint32_t count, float carrier, int batch, hipStream_t s);
struct AmLoadParams { const float* in; size_t in_stride; RingF out; uint64_t n0; uint32_t count; };
void launch_am_load(const AmLoadParams& p, int batch, hipStream_t s);
struct AmToneParams { RingF out; uint64_t n0; uint32_t count; const float* tab; uint32_t inc; uint64_t k0; double ampl; float offset; };
void launch_am_tone(const AmToneParams& p, int batch, hipStream_t s);
struct AmIirState { double y1; float x1, pad; };
struct AmIirParams { RingF in, out; uint64_t n0; uint32_t count; float gain; double ff0, ff1, fb1; AmIirState* st;
                     // gr_mod_nbfm::set_ctcss: add_ff(audio, sig_source_f(8000, GR_COS_WAVE, tone, 0.15)) in front of the filter -- the fixed-point NCO of
                     // oracle/orc_chains.c orc_sig_source_cos: sample k (tone_k0 + t) = (float)(cos_fx(k * tone_inc) * tone_ampl); tone_tab == nullptr: no tone
                     const float* tone_tab; uint32_t tone_inc; uint64_t tone_k0; double tone_ampl; };
void launch_am_iir(const AmIirParams& p, int batch, hipStream_t s);
// gr_mod_ssb: float_to_complex + cessb clipper (f32 ring -> complex ring), cessb stretcher with complex output over [q0, q0 + count)
struct AmClipParams { RingF in; RingC out; uint64_t n0; uint32_t count; float clip; const float* atan_tab; };
void launch_am_clip(const AmClipParams& p, int batch, hipStream_t s);
struct AmStretchParams { RingC in, out; uint64_t q0; uint32_t count; };
void launch_am_stretch(const AmStretchParams& p, int batch, hipStream_t s);
struct AnStretchParams { RingC in; RingF out; const AnState* st; float level; };
void launch_an_stretch(const AnStretchParams& p, uint32_t max_out, int batch, hipStream_t s);

// ---- frame FEC (kernels_framefec.hip): bursts [n][33] <-> payloads [n][12]; M17 frames [n][48] -> records [n][40] ----
void launch_bptc_decode(const uint8_t* bursts, size_t n, uint8_t* payloads, hipStream_t s);
void launch_bptc_encode(const uint8_t* payloads, size_t n, uint8_t* bursts, hipStream_t s);
void launch_m17_decode(const uint8_t* frames, size_t n, uint8_t* records, hipStream_t s);
void launch_m17_encode(const uint8_t* records, size_t n, uint8_t* frames, hipStream_t s);
// ---- DMR layer 2 (kernels_dmr_l2.hip): mailbox records [batch][cap][40] -> [batch][cap][80]; rate 3/4 bursts [n][33] <-> payloads [n][18] ----
void launch_dmr_l2(const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap, int audio_fec, uint8_t* out, hipStream_t s);
void launch_trellis34_decode(const uint8_t* bursts, size_t n, uint8_t* payloads, uint8_t* ok, hipStream_t s);
void launch_trellis34_encode(const uint8_t* payloads, size_t n, uint8_t* bursts, hipStream_t s);
// ---- DMR layer 2 transmit (kernels_dmr_tx.hip): TX records [batch][cap][48], or calls [batch][40] + codec frames [batch][n][27], -> bursts
//      out[b * out_stride + i * slot_bytes], 33 bytes and zeros up to slot_bytes ----
void launch_dmr_tx(const uint8_t* records, const uint32_t* counts, size_t batch, size_t cap, uint8_t* out, size_t out_stride, size_t slot_bytes,
                   hipStream_t s);
void launch_dmr_tx_call(const uint8_t* calls, const uint8_t* voice, const uint32_t* first, size_t batch, size_t n_bursts, uint8_t* out,
                        size_t out_stride, size_t slot_bytes, hipStream_t s);
// ---- DMR receive call layer (kernels_dmr_rx.hip): layer-2 records [batch][cap][80] -> call records [batch][cap][128] through the per-stream
//      states [batch] (dmr_rx_core.hpp's dmr_rx_state); the public 12 bytes of every state ----
constexpr size_t DMR_RX_RECORD_BYTES = 128, DMR_RX_STATE_BYTES = 128, DMR_RX_PUBLIC_BYTES = 12;   // kernels_dmr_rx.hip holds them to the core
//      slot_info: the slot records [batch][cap][16] of the repeater-mode sink, or null; repeater 1: DMRControl outside DMO mode, on `timeslot`
void launch_dmr_rx(const uint8_t* l2, const uint32_t* counts, size_t batch, size_t cap, int color_code, int promiscuous, void* states, uint8_t* out,
                   hipStream_t s, const uint8_t* slot_info = nullptr, int repeater = 0, int timeslot = 1);
void launch_dmr_rx_state(const void* states, size_t batch, uint8_t* out, hipStream_t s);
// ---- DMR repeater-mode burst sink (kernels_dmr_sink.hip): unpacked bits bits[b * stride + i], i < min(n, counts[b * count_stride]), -> frame
//      records [batch][cap][40] and slot records [batch][cap][16] through the per-stream states [batch] (dmr_sink_core.hpp's dmr_sink_state) ----
constexpr size_t DMR_SINK_STATE_BYTES = 160;   // kernels_dmr_sink.hip holds it to the core
struct DmrSinkParams {
    const uint8_t* bits; size_t stride; uint32_t n; const uint32_t* counts; size_t count_stride;
    void* st; uint8_t* frames; uint8_t* info; uint32_t cap; uint32_t* out_counts;
};
void launch_dmr_sink(const DmrSinkParams& p, int batch, hipStream_t s);
void launch_dmr_sink_flush(void* states, int batch, hipStream_t s);
// ---- M17 link layer (kernels_m17_link.hip): the frame synchroniser's records frames[b * frame_stride + 56 i], i < min(counts[2 b + 1], cap), ->
//      decode records scratch [batch][cap][40] -> link records [batch][cap][64] through the per-stream states [batch] (m17_link_core.hpp's
//      m17_rx_state); the public 16 bytes of every state; every state to a fresh decoder's ----
constexpr size_t M17_RX_RECORD_BYTES = 64, M17_RX_STATE_BYTES = 64, M17_RX_PUBLIC_BYTES = 16, M17_FS_RECORD_BYTES = 56,
                 M17_DEC_RECORD_BYTES = 40;   // kernels_m17_link.hip holds them to the core
void launch_m17_rx(const uint8_t* frames, size_t frame_stride, const uint32_t* counts, size_t batch, size_t cap, int can_rx, int decode_all_can,
                   uint8_t* scratch, void* states, uint8_t* out, hipStream_t s);
void launch_m17_rx_state(const void* states, size_t batch, uint8_t* out, hipStream_t s);
void launch_m17_rx_reset(void* states, size_t batch, hipStream_t s);
//      transmit: call descriptors [batch][32] -> kind 0: preamble + LSF frame (96 bytes a row), 1: stream frames first[b] + i with payloads
//      [batch][n][16] at out[b * out_stride + i * slot_bytes], 2: the last frame + the EOT bytes (64 bytes a row)
void launch_m17_call(int kind, const uint8_t* calls, const uint8_t* payloads, const uint32_t* first, size_t batch, size_t n, uint8_t* out,
                     size_t out_stride, size_t slot_bytes, hipStream_t s);

// ---- side outputs (kernels_side.hip): rssi_block on port 0, rx_fft_c on the device-rate IQ ----
constexpr uint32_t RSSI_RING = 4096;   // |x|^2 look-back ring per stream (moving_average_ff(2000) reads 1999 items back)
struct RssiState { double prev; uint64_t n; float sum, last; };
struct RssiBlockParams {
    const float2* in; size_t in_stride; uint32_t n;       // port-0 items of this call: in[b * in_stride + i]
    const uint32_t* counts; size_t count_stride;         // per-stream item count (device), or nullptr: n for every stream
    RssiState* st; float* ring; int batch;
    float level, n_log2_10;
    float* out; size_t out_cap; float* last; uint32_t* out_counts;
};
void launch_rssi(const RssiBlockParams& p, hipStream_t s);
// in_fmt IN_SC16: `in` points at int16 I, Q pairs and a sample is converted ((float)v * in_scale) in front of the window multiply;
// IN_SC8 / IN_CU8: 8-bit pairs, ((float)u - in_bias) * in_scale (iq8_to_f2)
void launch_fft_fill(const float2* in, size_t in_stride, uint32_t i0, uint32_t count, const float* win, uint32_t counter, float2* buf, uint32_t N, int batch, hipStream_t s,
                     int in_fmt = IN_CF32, float in_scale = 0.0f, float in_bias = 0.0f);
void launch_fft_power(const float2* X, float* out, uint32_t N, int batch, hipStream_t s);
void launch_fft_shift(const float* pts, float* out, size_t out_stride, uint32_t N, int batch, hipStream_t s);

}  // namespace qrl
