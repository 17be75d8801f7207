// demod.hpp — the receiver handle behind qrl_demod_*.  Host only, included by the receiver files only: engine.cpp (the digital families, the C ABI),
// demod_analog.cpp and demod_dsss.cpp (the two families that leave process() behind the first resampler and run on the main stream alone).
#pragma once
#include "host_common.hpp"
#include "firdes.hpp"
#include <utility>

namespace qrl {

// polyphase layout for k_decim: taps[p*Jpad + j] = h[p + j*D]
inline std::vector<float> decim_layout(const std::vector<float>& h, int D, int Jpad)
{
    std::vector<float> t((size_t)D * Jpad, 0.0f);
    for (size_t k = 0; k < h.size(); ++k) t[(k % D) * Jpad + k / D] = h[k];
    return t;
}
inline std::vector<float> resamp_layout(const std::vector<float>& h, int I, int Jp)
{
    std::vector<float> t((size_t)I * Jp, 0.0f);
    for (size_t k = 0; k < h.size(); ++k) t[(k % I) * Jp + k / I] = h[k];
    return t;
}
inline std::vector<float2> to_f2(const std::vector<std::complex<float>>& v)
{
    std::vector<float2> r(v.size());
    for (size_t i = 0; i < v.size(); ++i) r[i] = make_float2(v[i].real(), v[i].imag());
    return r;
}

struct DecimStage {
    bool used = false;
    DecimChoice c{DECIM_CLASS_GENERIC, DECIM_R4_J12, 0};   // kernel class of the geometry (decim_plan.hpp)
    int D = 1, nt = 0, S = 0;
    DevBuf<float> taps;
    DevBuf<float2> edge, edge_b; uint32_t edge_len = 0;   // phase-lane kernels: per-stream scratch for the call's edge outputs (two: staged a call ahead)
    int alloc_edge(int B, bool two = false) {
        edge_len = (uint32_t)(c.cls == DECIM_CLASS_PM ? decim_pm_edge_len(nt, D) : c.cls == DECIM_CLASS_PL ? decim_pl_edge_len(nt, D) : 0);
        if (!edge_len) return QRL_OK;
        if (int r = edge.alloc((size_t)B * edge_len)) return r;
        return two ? edge_b.alloc((size_t)B * edge_len) : QRL_OK;
    }
    int plan(const std::vector<float>& h, int D_) {
        used = true; D = D_; nt = (int)h.size();
        c = decim_choose(nt, D);
        switch (c.cls) {
        case DECIM_CLASS_PM: return taps.upload(decim_pm_layout(h, D));
        case DECIM_CLASS_PL: return taps.upload(decim_pl_layout(h, D));
        case DECIM_CLASS_M16: {
            // zero-padded tap vector the MFMA A operands are read from: hp[k + (4S - nt + 1)] = h[k]
            S = decim_mfma_steps(nt, D);
            std::vector<float> g((size_t)decim_mfma_hpn(nt, D), 0.0f);
            for (int k = 0; k < nt; ++k) g[(size_t)k + (size_t)(4 * S - nt + 1)] = h[k];
            return taps.upload(g);
        }
        case DECIM_CLASS_GENERIC: return taps.upload(decim_layout(h, D, c.Jpad));
        default: return QRL_ERR_ARG;
        }
    }
    uint32_t lookback() const { return decim_lookback(c, nt, D); }
    const char* kernel_name() const { return c.cls == DECIM_CLASS_PM ? "k_decim_pm" : c.cls == DECIM_CLASS_PL ? "k_decim_plx" : c.cls == DECIM_CLASS_M16 ? "k_decim_mfma" : "k_decim"; }
    int launch(DecimParams& p, int B, hipStream_t s, int parity = 0) const {
        p.nt = nt;
        float2* e = parity && edge_b.p ? edge_b.p : edge.p;
        if (c.cls == DECIM_CLASS_PM || c.cls == DECIM_CLASS_PL) {
            p.pl_taps = taps.p; p.pl_edge = e; p.pl_edge_stride = edge_len; p.pl_edge_cap = edge_len;
            return c.cls == DECIM_CLASS_PM ? launch_decim_pm(p, B, s) : launch_decim_pl(p, B, s);
        }
        if (c.cls == DECIM_CLASS_M16) { p.gtab = taps.p; p.S = S; return launch_decim_mfma(p, B, s); }
        launch_decim(p, B, c.variant, s);
        return 0;
    }
};

struct PortC { float2* p; size_t cap; };       // a complex side port of one call: the caller's buffer (or null) and its capacity per stream
struct CallCounts { size_t n1, n2, nsym; };    // upper bounds on what a call of n input samples produces: 1 Msps items, target-rate items, symbols

// analogue voice receivers (gr_demod_nbfm / gr_demod_am / gr_demod_wbfm / gr_demod_ssb): kernels_analog.hip.  `d` is the handle that owns the chain
struct AnalogChain {
    int kind = 0; bool lsb = false;                        // 0 NBFM, 1 AM, 2 WBFM, 3 SSB (lsb: lower sideband)
    DevBuf<float2> c1;                                        // SSB: clipped complex items behind the gate
    DevBuf<float2> filt_c; int nfc = 0;                    // AM channel filter (complex taps)
    DevBuf<float> env, rtaps, ftaps; int ramp = 0, nr = 0, nf = 0, I = 2, D = 5;
    DevBuf<float> f1, f2, f3; uint32_t m1 = 0, m2 = 0; DevBuf<AnState> st;
    // gr_demod_nbfm::set_ctcss: ctcss_squelch_ff between audio resampler and audio filter, band-pass audio filter while it is on
    float tone = 0.0f; DevBuf<CtcssState> cs; DevBuf<float> f4, ftaps_ct; DevBuf<double> env_ct; int nf_ct = 0;
    float wr[3] = {0, 0, 0}, wi[3] = {0, 0, 0};
    double threshold = 1e-14, ff[2] = {0, 0}, fb1 = 0, de_ff[2] = {0, 0}, de_fb1 = 0;
    float gain = 1.f, attack = 0.1f, decay = 0.1f, if_gain = 0.9f;
    int build(qrl_demod& d, size_t max2);         // max2: target-rate items per call
    int init_state(qrl_demod& d);
    int stages(qrl_demod& d, uint64_t n2_0, uint64_t n2_1, const qrl_demod_out* out, uint32_t* counts);
};

// DSSS mode (gr_demod_dsss.cpp:30-111): behind the 1:50 stage (ring s2, 20 ksps) a 13/50 resampler to 5 200 samples/s, Costas,
// channel filter, agc2, Barker-13 matched filter (16 symbols/s), clock recovery + Costas (kernels_dsss.hip)
struct DsssChain {
    DevBuf<float> rs, filt, mf; int Jp = 0, nf = 0;
    DevBuf<float2> ra, rb, rc, rd, sym; uint32_t mask = 0, sym_mask = 0;
    DevBuf<DsssState> st; DevBuf<DsssTailState> tail;
    float a1 = 0, b1 = 0, a2 = 0, b2 = 0;
    uint64_t n5 = 0, nsy = 0;   // items so far at 5 200 samples/s, matched-filter outputs so far
    int build(qrl_demod& d, size_t max2);
    int init_state(qrl_demod& d);
    int stages(qrl_demod& d, uint64_t n2_0, uint64_t n2_1, const qrl_demod_out* out, uint32_t* counts);
};

}  // namespace qrl

using namespace qrl;   // for the three receiver files, which are all that include this header (every host .cpp of the library has the directive)

struct qrl_demod {
    qrl_ctx* ctx = nullptr;
    qrl_demod_config cfg{};
    // Streams in front of the events and fences: the events are destroyed first.
    HandleStream stream;   // the caller's, or the handle's own
    // the serial tail (symbol sync + Viterbi: a handful of waves) runs on its own stream so that it overlaps the
    // HBM-facing kernels of the NEXT call instead of idling 250 CUs
    HandleStream tail;
    // QPSK / BPSK / 4FSK-discriminator families: the recursive chain (k_qpsk_*: latency bound, 64 streams per workgroup) runs on
    // `tail`, the Viterbi decoder on `fecs`: call k's decoder, call k + 1's recursion and call k + 2's front end run side by side.
    // The rings between them hold two calls; ev_q / ev_fec guard their reuse two calls later.
    HandleStream fecs;
    HandleStream pre;   // HELPER STREAM of the front end, below
    // STICKY fences (host_common.hpp), one per ring slot: the recursion and the decoder of the call in slot k & 1
    Fence ev_q[2], ev_fec[2];
    // GROUPED ORDER (gr_demod_qpsk chain whose recursion kernel has a workgroup for at least every second CU): k_qpsk_pipe4 is a serial
    // walk, one workgroup of 6 waves and 137 KB of LDS per 64 streams.  Left to the three streams, the front end of call k + 1 (tens of
    // thousands of small workgroups) and the decoder of call k - 1 (a wave per two trellises, for its whole run) take every LDS byte
    // and wave slot the moment they free up, and the recursion of call k is only placed once both have drained: (front end || decoder)
    // 2.6 ms, then the recursion alone 1.9 ms (profiles/r04_c5_rx_timeline.log).  Grouped: the front end of call k + 1 waits for the
    // recursion of call k, and the decoder of call k - 1 is LAUNCHED with the recursion of call k (behind the same front-end event),
    // which leaves front end alone -> recursion || decoder.  The deferred launch is flushed by everything that waits for results
    // (qrl_demod_sync, qrl_demod_stream_wait, reset, destroy), so a caller never sees the difference.
    bool grouped = false, grouped_capable = false, fec_deferred = false; FecParams fec_pending{}; int fec_pending_slot = 0;
    DevBuf<uint64_t> qp_snap;   // [2][B] symbols produced up to the end of call k (slot k & 1): what that call's decoder may read
    Event ev_ff; Fence ev_tail;   // ev_tail: ONE-SHOT, taken by the next call's stage that rewrites ring r3 (serial order only)
    // HELPER STREAM of the front end (round 6): k_hist (the rotated tail of this call's IQ, kept for the next call) and k_pl_edge_stage (the
    // next call's edge scratch: that history + the head of the next buffer) read the caller's buffers only, yet they sat between two front-end
    // launches on the handle's stream -- 0.2 - 0.29 ms of C1's 8 ms step (profiles/r06_c1_helper_stream.log).  On `pre` they run BESIDE the
    // front end: edge(k) behind hist(k - 1); hist(k) behind the front end of call k - 1 (the last reader of the history buffer it overwrites);
    // the front end of call k waits for ev_pre.  The history and the edge scratch are double buffers.
    // Only with QRL_OPT_INPUT_RESIDENT: the helpers then read a call's IQ WITHOUT waiting for what the caller queued on the handle's stream before the call.
    Fence ev_pre, ev_fe[2];   // ev_pre: ONE-SHOT (also recorded by the launchers, DecimParams::pre_event: created with the stream); ev_fe: STICKY
    bool input_resident = false;
    Event ev_user[4];   // qrl_demod_stream_wait
    // overlapped mode (2FSK / GMSK / 4FSK families): everything behind the first decimated ring runs on the tail stream while
    // the front end of the NEXT call already runs on the main stream; ring s2 holds two calls, ev_tail2 guards its reuse
    bool qpsk_fll = false, fsk4_disc = false;
    bool m17 = false;   // F_DMR family, gr_demod_m17 variant: channel filter behind the resampler (port 0), mod-M&M TED, no level control
    DevBuf<float2> s2g, disc4_taps; DevBuf<float> sym4_taps; int disc4_nt = 0, sym4_nt = 0;   // 4FSK non-FM branch
    bool fll_slim = false;   // QRL_OPT_FLL_SLIM: single-wave FLL workgroups (3 KB of LDS) that fit beside four front-end workgroups
    bool d2f_capable = false, d2f = false; DevBuf<float> d2f_taps;   // 1:2 decimator + shaping filter in one kernel (k_dec2_fir)
    bool overlap = false, overlap_capable = false; Fence ev_tail2[2]; uint64_t call_no = 0;   // ev_tail2: STICKY
    enum Family { F_2FSK, F_GMSK, F_QPSK, F_DMR, F_4FSK, F_BPSK, F_DSSS, F_ANALOG } fam = F_2FSK;
    int branches = 2;

    // derived chain parameters (gr_demod_2fsk.cpp:39-63, gr_demod_gmsk.cpp:39-63)
    int fe_decim = 1, interp = 1, decim = 1, target = 0, sps_eff = 0;
    bool fm = false;

    // stage objects
    DecimStage fe;      // gr_demod_base resampler (device rate >= 2 Msps)
    DecimStage first;   // per-mode _resampler when interp == 1
    // time-domain scope tap (gr_demod_base.cpp:62-63, 1115-1147, 988-1018): _demod_valve -> rational_resampler_ccf(1, 10, low_pass(1, 1e6,
    // 50000, 25000, HAMMING)) -> gr_sample_sink; off until qrl_demod_set_time_domain_output gives it a buffer
    DecimStage scope; DevBuf<float2> s_scope; uint32_t scope_mask = 0; uint64_t n_scope = 0; int scope_D = 10;
    float2* scope_out = nullptr; size_t scope_cap = 0; uint32_t* scope_counts = nullptr;
    DevBuf<float> rs_taps; int rs_Jp = 0;  // per-mode _resampler when interp > 1
    DevBuf<float> filt_taps; int filt_nt = 0;
    DevBuf<float> symf_taps; int symf_nt = 0;
    DevBuf<float2> disc_up, disc_lo; int disc_nt = 0;
    DevBuf<float> ff_tf, ff_ts; DevBuf<float2> ff_up, ff_lo;   // zero-padded copies for the fused 2FSK kernel (k_2fsk_ff)
    DevBuf<float2> fll_lo, fll_up; float fll_alpha = 0, fll_beta = 0, fll_maxf = 0;
    DevBuf<float> atan_tab, mmse_tab;
    float demod_gain = 0;
    float ss_alpha = 0, ss_beta = 0, ss_maxp = 0, ss_minp = 0;

    // rotator (gr_demod_base.cpp:57,1220-1225): exact 2^-64-turn NCO
    Rotator rot;

    // rings and state
    DevBuf<float2> hist_a, hist_b; uint32_t hist_len = 0; bool hist_flip = false;
    DevBuf<float2> s1, s2, s2l, s2f; DevBuf<float> s2d, s3; DevBuf<uint8_t> soft;
    uint32_t s1_mask = 0, s2_mask = 0, soft_mask = 0;
    DevBuf<FllState> fll_st; DevBuf<SymSyncState> ss_st; DevBuf<FecState> fec_st;
    // a37b: gr_dmr_dmo_sink behind port 3 of gr_demod_dmr (qrl_demod_set_dmo_output)
    DevBuf<DmoState> dmo_st; DevBuf<uint32_t> dmo_golay; uint8_t* dmo_out = nullptr; uint32_t dmo_cap = 0; uint32_t* dmo_counts = nullptr;
    // QPSK (gr_demod_qpsk.cpp:97-126)
    DevBuf<QpskState> qp_st; DevBuf<float> tanh_tab;
    float c1_alpha = 0, c1_beta = 0, c2_alpha = 0, c2_beta = 0; float2 qp_rot{};
    DevBuf<uint32_t> counts_scratch;
    AnalogChain an;   // fam == F_ANALOG
    DsssChain ds;     // fam == F_DSSS
    uint64_t n_in = 0, n1 = 0, n2 = 0;  // items so far: device rate, 1 Msps, target rate
    bool profiling = false;
    ProfSpans prof;   // the HBM-facing kernel of each profiled call

    int flush_fec(bool behind_front_end);   // engine.cpp: launches the decoder call the grouped order holds back, if any
    int sync_all() {
        if (int r = flush_fec(false)) return r;
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipStreamSynchronize(tail));
        HIPCHK(hipStreamSynchronize(fecs));
        if (pre) HIPCHK(hipStreamSynchronize(pre));
        return QRL_OK;
    }
    bool loops_family() const { return fam == F_QPSK || fam == F_BPSK || fsk4_disc; }
    int init_state();
    int build();
    // fmt: IN_CF32 (iq = interleaved floats) | IN_SC16 (iq = interleaved int16 pairs, stride in samples of 4 bytes; handles with a front end, or sc16_baseband)
    // | IN_SC8 | IN_CU8 (8-bit pairs, stride in samples of 2 bytes; handles with a front end, or iq8_baseband).
    // The format belongs to the CALL: history, edge scratch and rings are rotated cf32 whatever the calls before were fed.
    int process(const void* iq, size_t stride, size_t n, const qrl_demod_out* out, int fmt = IN_CF32);
    float sc16_scale = 1.0f / 32768.0f;   // qrl_demod_set_sc16_scale
    float sc8_scale = 1.0f / 128.0f;      // qrl_demod_set_sc8_scale
    float cu8_scale = 1.0f / 128.0f, cu8_bias = 127.5f;   // qrl_demod_set_cu8_scale
    // what the kernels that read the caller's buffer get for a call of format fmt (sc8 runs the unsigned path on v ^ 0x80 with the bias 128: exact)
    InFormat in_format(int fmt) const {
        return fmt == IN_SC8 ? InFormat{fmt, sc8_scale, 128.0f} : fmt == IN_CU8 ? InFormat{fmt, cu8_scale, cu8_bias} : InFormat{fmt, sc16_scale, 0.0f};
    }
    bool sc16_baseband = false;           // QRL_OPT_SC16_BASEBAND: a handle without a front end takes int16 IQ (its first stage reads the raw pairs)
    bool iq8_baseband = false;            // QRL_OPT_IQ8_BASEBAND: the same for sc8 / cu8 (independent of sc16_baseband)
    int init_dmo_state() { DmoState x; std::memset(&x, 0, sizeof x); x.endPtr = 9999; return dmo_st.fill(cfg.batch, x); }
    CallCounts call_counts(size_t n) const {
        const size_t c1 = fe.used ? n / fe_decim + 2 : n, c2 = c1 * interp / decim + 2;
        return {c1, c2, c2 / (size_t)(sps_eff > 1 ? sps_eff - 1 : 1) + 8};
    }
    // ports 0 and 1 of the hier block as this call's caller wants them: nothing without enable_side_outputs or without `out`
    PortC filtered_port(const qrl_demod_out* out) const { return cfg.enable_side_outputs && out ? PortC{reinterpret_cast<float2*>(out->filtered), out->filtered_cap} : PortC{nullptr, 0}; }
    PortC constellation_port(const qrl_demod_out* out) const { return cfg.enable_side_outputs && out ? PortC{reinterpret_cast<float2*>(out->constellation), out->constellation_cap} : PortC{nullptr, 0}; }
    // input of a stage that reads items src0 .. src1 of the 1 Msps signal: ring s1 behind the front end, else the caller's IQ (rotated on the fly; hist_old: the call before)
    // fmt: what `in` points at (without a front end IN_SC16: QRL_OPT_SC16_BASEBAND, IN_SC8 / IN_CU8: QRL_OPT_IQ8_BASEBAND); the ring behind a front end is cf32 whatever the call was fed
    template <class P> void input_source(P& p, const float2* in, size_t stride, const float2* hist_old, uint64_t src0, uint64_t src1, int fmt) const {
        if (fe.used) { p.in = nullptr; p.in_ring = RingC{s1.p, s1_mask}; }
        else { p.in = in; p.in_stride = stride; p.hist = hist_old; p.hist_len = hist_len; p.rot_enable = 1; rot.fill(p); in_format_fill(p, in_format(fmt)); }
        p.n0 = src0; p.n = (uint32_t)(src1 - src0);
    }
};
