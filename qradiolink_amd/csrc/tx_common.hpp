// tx_common.hpp — what the transmitters (tx.cpp, amod.cpp, synth.cpp) share on the host side: the gr_mod_base back end, the sc16 and sc8
// output sinks and the device step of the gr_zero_idle_bursts run list.  Host only, like host_common.hpp.
#pragma once
#include "host_common.hpp"

namespace qrl {

constexpr size_t kTapPad = 64;   // zeros behind every tap table of the transmitters: k_tx_interp_sym reads its I x J = 64 taps unguarded

constexpr int kTxMaxRate = 183000000;   // device rates: 1e6, or a multiple of 1e6 in [2e6, 183e6], as on the receivers
// Which kernel interpolates to the device rate: k_tx_interp_mfma (kernels_tx_mfma.hip) from this many device samples per 1 Msps sample up,
// k_tx_interp_c (kernels_tx.hip) below.  A 32-row phase tile is mostly padding at small ratios; docs/MEASUREMENT.md, "TX back end rates",
// has the A/B behind the value.  Both kernels give the same bits.
constexpr int kTxMfmaMinInterp = 4;
// the taps h of the back-end interpolator in k_tx_interp_mfma's layout [phase tile][lag][phase in tile] (engine.hpp)
std::vector<float> tx_mfma_taps(const std::vector<float>& h, int interp);

// gr_mod_base back end (reference src/gr/gr_mod_base.cpp:38,215-258) behind a modulator chain that ends at 1 Msps: the carrier rotator,
// then the interpolator to the device rate.  Off (rate 0 or 1e6 and a zero offset): the chain's last kernel stores to the caller's buffer.
struct TxBackEnd {
    // range check of the device rate (message prefixed by `who`; `noun` names the handle in the retunes' refusal); bb_stride = the chain's
    // 1 Msps samples per stream and call at most
    int init(const char* who, const char* noun, int rate, double offset_hz, int batch, size_t bb_stride);
    int reset(hipStream_t s);   // interpolator history, sample counter and every phase to 0; the offsets stay
    // phase-continuous like rotator_cc::set_phase_inc; both refuse a handle without the back end and drain s before the tables are rewritten
    int retune(double hz, hipStream_t s);
    int retune_streams(const double* hz, int batch, hipStream_t s);
    // where the chain's last kernel stores and in which format: the caller's buffer, or bb (cf32) when the back end is on
    struct Target { float2* out; size_t stride; TxOut sc; };
    Target target(void* iq, size_t out_stride, TxOut sc) const
    {
        return on_ ? Target{bb.p, bb_stride, TxOut{}} : Target{reinterpret_cast<float2*>(iq), out_stride, sc};
    }
    // n1 samples per stream at 1 Msps are in bb: rotator (+ interpolator) to iq.  Nothing when the back end is off or n1 = 0.
    void run(uint32_t n1, void* iq, size_t out_stride, TxOut sc, int batch, hipStream_t s);
    int interp() const { return interp_; }   // device samples per 1 Msps sample
private:
    const char* noun_ = "";
    bool on_ = false, mfma_ = false; int interp_ = 1, nt = 0; DevBuf<float> taps;   // taps: h, or tx_mfma_taps(h) when mfma_
    DevBuf<float2> bb; size_t bb_stride = 0;       // the chain's output, linear, one call's worth
    DevBuf<float2> ring; uint32_t mask = 0;        // rotated 1 Msps signal (interpolator history)
    Rotator rot; uint64_t n_bb = 0;                // carrier NCO at 1 Msps; n_bb: samples through it so far
    int refuse() const { return qrl_set_error(QRL_ERR_ARG, std::string(noun_) + " was created without the gr_mod_base back end"); }
};

// qrl_*_process_sc16 of a transmitter: the format belongs to the call, scale and clip counters to the handle
struct Sc16Sink {
    float scale = 32767.0f; uint32_t* clip = nullptr;
    int set_scale(const char* who, float v) { if (!sc16_scale_ok(who, v)) return QRL_ERR_ARG; scale = v; return QRL_OK; }
    int set_clip(uint32_t* counts) { clip = counts; return QRL_OK; }
    int for_call(const char* who, const void* iq, TxOut& out) const
    {
        if (reinterpret_cast<uintptr_t>(iq) & 3u) return qrl_set_error(QRL_ERR_ARG, std::string(who) + ": iq must be 4-byte aligned (one packed store per sample)");
        out = TxOut{OUT_SC16, scale, clip};
        return QRL_OK;
    }
};

// qrl_*_process_sc8 of a transmitter: a scale and clip counters of its own beside the sc16 ones; a sample is one 2-byte store
struct Sc8Sink {
    float scale = 127.0f; uint32_t* clip = nullptr;
    int set_scale(const char* who, float v) { if (!sc16_scale_ok(who, v)) return QRL_ERR_ARG; scale = v; return QRL_OK; }
    int set_clip(uint32_t* counts) { clip = counts; return QRL_OK; }
    int for_call(const char* who, const void* iq, TxOut& out) const
    {
        if (reinterpret_cast<uintptr_t>(iq) & 1u) return qrl_set_error(QRL_ERR_ARG, std::string(who) + ": iq must be 2-byte aligned (one 2-byte store per sample)");
        out = TxOut{OUT_SC8, scale, clip};
        return QRL_OK;
    }
};

// the run list (zero_runs.hpp) with its device copy
struct ZeroRuns : ZeroRunList {
    // zeroes what the runs cover of items [lo, hi) of ring r, then forgets the runs that end there.  Host-synchronous on s when a run is live.
    int apply(RingC r, uint64_t lo, uint64_t hi, hipStream_t s);
private:
    DevBuf<ZeroRun> dev;
};

}  // namespace qrl
