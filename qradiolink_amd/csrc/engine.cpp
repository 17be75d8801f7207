// engine.cpp — host side of libqrl_hip.so: builds the per-mode kernel pipeline the reference builds
// as a GNU Radio flowgraph (gr_demod_base.cpp:299-828 connects rotator -> resampler -> gr_demod_X),
// owns all device state, and exposes it through the C ABI of include/qrl_hip.h.
// There is NO CPU fallback: without a usable HIP device qrl_init() fails.
#include "demod.hpp"
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>

#ifndef QRL_FEC_GATE_US
#define QRL_FEC_GATE_US 30u   // grouped order: head start of the recursion kernel over the decoder (profiles/r04_c5_rx_timeline.log: without it the decoder takes every wave slot first)
#endif
#ifndef QRL_DEV_SKIP
#define QRL_DEV_SKIP 0   // developer builds only (tools/engine_variants.sh): bit 0 no FLL, 1 no fused 2FSK feed-forward kernel, 2 no symbol sync, 3 no decoder launch -- WRONG results, timing experiments on who stretches the front end
#endif

// the entry point an 8-bit call came through, for the error text
static const char* in_fmt_entry(int fmt) { return fmt == IN_SC8 ? "qrl_demod_process_sc8" : "qrl_demod_process_cu8"; }

int qrl_demod::flush_fec(bool behind_front_end)
{
    if (!fec_deferred) return QRL_OK;
    fec_deferred = false;
    QRLCHK(ev_q[fec_pending_slot].wait(fecs));   // (armed: the call that deferred the decoder recorded it)
    if (behind_front_end) {   // starts with the recursion of the next call, not beside its front end -- and a moment AFTER it (k_fec_gate)
        QRLCHK(ev_ff.wait(fecs));
        launch_fec_gate(QRL_FEC_GATE_US, fecs);
    }
    launch_fec(fec_pending, cfg.batch, fecs);
    QRLCHK(ev_fec[fec_pending_slot].record(fecs));
    return QRL_OK;
}

int qrl_demod::init_state()
{
    int r;
    for (auto* b : {&hist_a, &hist_b, &s1, &s2, &s2l, &s2f}) if (b->p && (r = b->zero())) return r;
    for (auto* b : {&s2d, &s3}) if (b->p && (r = b->zero())) return r;
    if (s_scope.p && (r = s_scope.zero())) return r;
    n_scope = 0;
    if ((r = soft.zero())) return r;
    if (fll_st.p && (r = fll_st.zero())) return r;
    if (loops_family()) {
        QpskState q; std::memset(&q, 0, sizeof q); q.gain = 1.0f; q.avg = q.inst = (float)sps_eff; q.mu = fam == F_BPSK ? 0.5f : 0.0f;   // BPSK: clock_recovery_mm_cc(mu = 0.5), gr_demod_bpsk.cpp:58-60
        if ((r = qp_st.fill(cfg.batch, q))) return r;
    }
    if (dmo_st.p && (r = init_dmo_state())) return r;
    SymSyncState ss; std::memset(&ss, 0, sizeof ss); ss.avg = ss.inst = (float)sps_eff;
    FecState fs; std::memset(&fs, 0, sizeof fs); fs.last_bits = 0xFE;   // descrambler seed 0x7F, newest bit first
    if ((r = ss_st.fill(cfg.batch, ss)) || (r = fec_st.fill((size_t)cfg.batch * 2, fs))) return r;
    if (qp_snap.p && (r = qp_snap.zero())) return r;
    if ((fam == F_DSSS && (r = ds.init_state(*this))) || (fam == F_ANALOG && (r = an.init_state(*this)))) return r;
    for (Fence* f : {&ev_q[0], &ev_q[1], &ev_fec[0], &ev_fec[1], &ev_tail2[0], &ev_tail2[1], &ev_fe[0], &ev_fe[1], &ev_tail, &ev_pre}) f->disarm();
    call_no = 0;
    fec_deferred = false;
    n_in = n1 = n2 = 0;
    hist_flip = false;
    return rot.reset(stream);   // per-stream phases restart too; the offsets stay
}

int qrl_demod::build()
{
    int r;
    const int sps = cfg.sps, samp_rate = cfg.samp_rate, fw = cfg.filter_width;
    if (fam == F_2FSK) {
        if (sps == 10)     { target = 20000; sps_eff = sps;     decim = 50; interp = 1; }
        else if (sps >= 5) { target = 40000; sps_eff = sps * 2; decim = 25; interp = 1; }
        else if (sps == 1) { target = 80000; sps_eff = 4;       decim = 25; interp = 2; }
        else return qrl_set_error(QRL_ERR_ARG, "2fsk: unsupported sps");
    } else if (fam == F_GMSK) {
        if (sps == 10)     { target = 20000; sps_eff = sps;     decim = 50; interp = 1; }
        else if (sps == 5) { target = 40000; sps_eff = sps * 2; decim = 25; interp = 1; }
        else if (sps == 1) { target = 80000; sps_eff = 4;       decim = 25; interp = 2; }
        else return qrl_set_error(QRL_ERR_ARG, "gmsk: unsupported sps");
    } else if (fam == F_DMR) {
        // gr_demod_dmr.cpp:36-58, gr_demod_m17.cpp:38-58: 3/125 resampler to 24 ksps, 5 samples per symbol
        target = 24000; sps_eff = 5; decim = 125; interp = 3; branches = 1;
    } else if (fam == F_4FSK) {
        // gr_demod_4fsk.cpp:45-82 (FM branch only; the non-FM discriminator bank of 4FSK2K is not built)
        fsk4_disc = !cfg.fm;   // ModemType4FSK2K: four band-pass magnitudes -> gr_4fsk_discriminator -> symbol_sync_cc (:110-127,165-181)
        if (fsk4_disc && sps == 2) return qrl_set_error(QRL_ERR_ARG, "4fsk: the sps = 2 geometry exists as FM variant only (gr_demod_4fsk.cpp:78-85 sets no rs/bw)");
        if (sps == 1)       { target = 80000;  sps_eff = 8;  decim = 25;  interp = 2; }
        else if (sps == 5)  { target = 20000;  sps_eff = 10; decim = 50;  interp = 1; }
        else if (sps == 10) { target = 10000;  sps_eff = 10; decim = 100; interp = 1; }
        else if (sps == 2)  { target = 500000; sps_eff = 5;  decim = 2;   interp = 1; }
        else return qrl_set_error(QRL_ERR_ARG, "4fsk: unsupported sps");
        branches = 1;
    } else if (fam == F_DSSS) {
        // gr_demod_dsss.cpp:37-59: 1:50 to 20 ksps (this stage), then 13/50 to 5 200 samples/s (ds.stages); sps = samples per chip
        if (sps != 25) return qrl_set_error(QRL_ERR_ARG, "dsss: sps must be 25 (make_gr_demod_dsss(25, ...), gr_demod_base.cpp:218)");
        target = 20000; sps_eff = 10; decim = 50; interp = 1;
    } else if (fam == F_ANALOG) {
        // gr_demod_nbfm.cpp:39,50 / gr_demod_am.cpp:36,44: 1:50 to 20 ksps; gr_demod_wbfm.cpp:37,49: 1:5 to 200 ksps (sps is unused there)
        // gr_demod_ssb.cpp:35,41-43: 1:sps (125) to 8 ksps
        target = an.kind == 2 ? 200000 : an.kind == 3 ? 8000 : 20000; decim = an.kind == 2 ? 5 : an.kind == 3 ? 125 : 50; interp = 1; sps_eff = 10; branches = 1;
        if (an.kind == 3 && sps != 125) return qrl_set_error(QRL_ERR_ARG, "ssb: sps must be 125 (make_gr_demod_ssb(125, ...), gr_demod_base.cpp:226-227)");
    } else if (fam == F_BPSK) {
        // gr_demod_bpsk.cpp:40-52: 1:50 to 20 ksps, sps samples per symbol
        if (sps != 10 && sps != 5) return qrl_set_error(QRL_ERR_ARG, "bpsk: sps must be 10 (BPSK1K) or 5 (BPSK2K)");
        target = 20000; sps_eff = sps; decim = 50; interp = 1;
    } else {
        // gr_demod_qpsk.cpp:39-60: sps <= 4 (QPSK250K / video: 1:2, no FLL), 4 < sps < 125 (QPSK20K: 1:25 to 40 ksps),
        // sps >= 125 (QPSK2K: 1:100 to 10 ksps); the last two run fll_band_edge_cc in front of the shaping filter (:130-138)
        if (sps < 2) return qrl_set_error(QRL_ERR_ARG, "qpsk: sps must be >= 2");
        if (sps > 4 && sps < 125) { target = 40000; sps_eff = sps * 4 / 25; decim = 25; }
        else if (sps >= 125)      { target = 10000; sps_eff = sps / 25;     decim = 100; }
        else                      { target = 500000; sps_eff = sps;         decim = 2; }
        if (sps_eff < 2 || sps_eff > 10) return qrl_set_error(QRL_ERR_ARG, "qpsk: unsupported samples per symbol");
        interp = 1; branches = 1; qpsk_fll = sps > 4;
    }
    fm = cfg.fm != 0;
    const int B = cfg.batch;

    // --- front end (gr_demod_base.cpp:1317-1340)
    fe_decim = 1;
    if (cfg.device_samp_rate >= 2000000) {
        fe_decim = cfg.device_samp_rate / 1000000;
        if ((r = fe.plan(low_pass(1, cfg.device_samp_rate, 480000, 100000, WIN_BLACKMAN_HARRIS), fe_decim))) return qrl_set_error(r, "front-end plan");
        if ((r = fe.alloc_edge(cfg.batch))) return qrl_set_error(r, "front-end edge scratch");
    }
    if ((r = rot.init(phase_inc_to_turn(2 * M_PI * -cfg.carrier_offset_hz / cfg.device_samp_rate)))) return r;

    // --- per-mode first resampler (gr_demod_2fsk.cpp:82-88, gr_demod_gmsk.cpp:80-83)
    const std::vector<float> rtaps = fam == F_DMR && m17
        ? low_pass(3, (double)samp_rate * 3, target / 2, target / 2, WIN_BLACKMAN_HARRIS)                    // gr_demod_m17.cpp:55-58
        : fam == F_DMR
        ? low_pass_2(3, (double)samp_rate * 3, 5000, 2000, 60, WIN_BLACKMAN_HARRIS)                          // gr_demod_dmr.cpp:55-58
        : fam == F_QPSK
        ? low_pass_2(interp, (double)interp * samp_rate, target / 2, target / 10, 60, WIN_BLACKMAN_HARRIS)   // gr_demod_qpsk.cpp:92-96
        : low_pass(interp, (double)interp * samp_rate, target / 2, target / 2, WIN_BLACKMAN_HARRIS);
    if (interp == 1) { if ((r = first.plan(rtaps, decim))) return qrl_set_error(r, "resampler plan"); if (!fe.used && (r = first.alloc_edge(cfg.batch))) return qrl_set_error(r, "resampler edge scratch"); }
    else {
        rs_Jp = ((int)rtaps.size() + interp - 1) / interp;
        if ((r = rs_taps.upload(resamp_layout(rtaps, interp, rs_Jp)))) return r;
    }

    // QPSK-250k class (gr_demod_qpsk.cpp:92-103 with sps <= 4): 1:2 resampler and the RRC behind it run as ONE kernel
    std::vector<float> d2f_rrc;
    if (fam == F_QPSK && !qpsk_fll && interp == 1) {
        d2f_rrc = root_raised_cosine(sps_eff, sps_eff, 1, 0.35, 11 * sps_eff);
        d2f_capable = d2f = dec2_fir_supported((int)rtaps.size(), decim, (int)d2f_rrc.size());
        if (d2f && (r = d2f_taps.upload(dec2_fir_table(rtaps, d2f_rrc)))) return r;
    }
    const uint32_t first_look = interp == 1 ? std::max<uint32_t>(first.lookback(), d2f ? dec2_fir_lookback() : 0u) : 0u;
    // --- the scope tap's 1:10 decimator on the 1 Msps signal (planned here so that the history below covers it; its ring is allocated on first use)
    {
        const int sr = cfg.time_domain_samp_rate;
        if (sr < 0 || sr > 500000 || cfg.time_domain_filter_width < 0 || cfg.time_domain_filter_width > 500000) return qrl_set_error(QRL_ERR_ARG, "time_domain_samp_rate / filter_width out of range");
        scope_D = sr > 0 ? 1000000 / sr : 10;
        if (sr > 0 && sr / 2 - sr / 8 <= 0) return qrl_set_error(QRL_ERR_ARG, "time_domain_samp_rate too small");
        const std::vector<float> h = cfg.time_domain_filter_width > 0 ? low_pass(1, 1000000, cfg.time_domain_filter_width, cfg.time_domain_filter_width, WIN_HAMMING)   // gr_demod_base.cpp:1292-1301
                                   : sr > 0 ? low_pass(1, 1000000, sr / 2 - sr / 8, sr / 4, WIN_HAMMING)                                                                  // :1249-1290
                                            : low_pass(1, 1000000, 50000, 25000, WIN_HAMMING);                                                                            // :62-63
        if (h.size() > 4096) return qrl_set_error(QRL_ERR_ARG, "time-domain filter too long (> 4096 taps)");
        if ((r = scope.plan(h, scope_D))) return qrl_set_error(r, "scope plan");
    }
    if (!fe.used && (r = scope.alloc_edge(cfg.batch))) return qrl_set_error(r, "scope edge scratch");
    // --- history of the caller's IQ kept by whichever stage reads it
    if (fe.used) hist_len = fe.lookback();
    else if (interp == 1) hist_len = std::max(first_look, scope.lookback());
    else hist_len = std::max((uint32_t)(rs_Jp + decim + 2), scope.lookback());
    if ((r = hist_a.alloc((size_t)B * hist_len)) || (r = hist_b.alloc((size_t)B * hist_len))) return r;

    // --- rings
    const CallCounts mx = call_counts(cfg.max_chunk);   // per call: 1 Msps items (behind the front end, else the caller's), target-rate items, symbols
    if (fe.used) {
        const size_t look = std::max<size_t>(interp == 1 ? first_look : (size_t)(rs_Jp + decim + 2), scope.lookback());
        s1_mask = pow2_at_least(mx.n1 + look + 64, 64) - 1;
        if ((r = s1.alloc((size_t)B * (s1_mask + 1)))) return r;
    }
    // default: only the 2FSK family, whose FLL + discriminator kernels are a third of a call (measured, C1: 15.2 -> 12.9 ms per
    // step); for the light GMSK / 4FSK tails the extra stream hand-over costs more than it hides (C2: 2.86 -> 3.05 ms).
    // Measured on C1 (round 3, same box): 8.79 instead of 9.49 ms per step, while the front-end kernel, sharing the GPU, stretches
    // from 6.33 to 8.04 ms -- the recursion kernels are only placed once front-end workgroups drain, and a 68 KB FLL workgroup then
    // takes the place of two of them.
    overlap_capable = fam == F_2FSK;
    grouped_capable = fam == F_QPSK && !fsk4_disc;   // the chain whose recursion is k_qpsk_pipe4
    {
        int dev = 0, cus = 256; hipDeviceProp_t pr;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) cus = pr.multiProcessorCount;
        grouped = grouped_capable && 2 * ((B + 63) / 64) >= cus;   // (below that the recursion's workgroups leave CUs free: the front end of the next call belongs beside it -- C3)
    }
    overlap = overlap_capable;   // round 3: ON by default for the 2FSK family (same-box A/B on C1: 8.79 against 9.49 ms per step); qrl_demod_set_option(QRL_OPT_OVERLAP, 0) gives the serial order
    s2_mask = pow2_at_least((overlap_capable || loops_family() ? 2 : 1) * mx.n2 + (fam == F_DMR ? 2048 : fam == F_ANALOG ? 4096 : 1024), 64) - 1;   // DMR: the DMO slicer looks back 1440 samples   // history needs: <= 501 taps downstream; overlapped mode: two calls
    const size_t ring2 = (size_t)B * (s2_mask + 1);
    if ((r = s2.alloc(ring2)) || (r = s2f.alloc(ring2)) || (r = s2d.alloc(ring2)) || (r = s3.alloc(ring2))) return r;
    if ((fam == F_2FSK || fam == F_BPSK || (fam == F_QPSK && qpsk_fll)) && (r = s2l.alloc(ring2))) return r;
    soft_mask = pow2_at_least((loops_family() ? 2 : 1) * (fam == F_QPSK || fam == F_4FSK ? 2 : 1) * mx.nsym + 512, 64) - 1;   // loops families: two calls (decoder of call k beside the recursion of call k + 1)
    if ((r = soft.alloc((size_t)B * (soft_mask + 1)))) return r;

    // --- decimated-rate filters
    {
        const std::vector<float> f = fam == F_QPSK
            ? root_raised_cosine(sps_eff, sps_eff, 1, 0.35, 11 * sps_eff)      // _shaping_filter, gr_demod_qpsk.cpp:100-103
            : fam == F_BPSK
            ? root_raised_cosine(sps_eff, sps_eff, 1, 0.35, 15 * sps_eff)      // _shaping_filter, gr_demod_bpsk.cpp:64-66
            : fam == F_4FSK
            ? low_pass(1, target, fw, fw / 2, WIN_BLACKMAN_HARRIS)             // _filter, gr_demod_4fsk.cpp:108-109
            : fam == F_ANALOG
            ? (an.kind == 2 ? low_pass_2(1, target, fw, 600, 90, WIN_BLACKMAN_HARRIS)      // gr_demod_wbfm.cpp:52-53
                            : low_pass_2(1, target, fw, 3500, 60, WIN_BLACKMAN_HARRIS))    // gr_demod_nbfm.cpp:53-54 (AM: an.filt_c)
            : low_pass(1, target, fw, fw, WIN_BLACKMAN_HARRIS);
        filt_nt = (int)f.size();
        if ((r = filt_taps.upload(f))) return r;
    }
    if ((r = atan_tab.upload(atan_table())) || (r = mmse_tab.upload(mmse_table()))) return r;
    if (fam == F_2FSK) {
        std::vector<std::complex<float>> lo, up;
        fll_band_edge_taps((float)sps_eff, 0.1f, 16, lo, up);
        if ((r = fll_lo.upload(to_f2(lo))) || (r = fll_up.upload(to_f2(up)))) return r;
        control_loop_gains((float)(24 * M_PI / 100), fll_alpha, fll_beta);
        fll_maxf = (float)(2 * M_PI * (2.0 / sps_eff));
        if ((r = fll_st.alloc(B))) return r;
        if (fm) {
            int nfilts = (sps == 1 ? 125 : 35) * sps_eff;
            if ((nfilts % 2) == 0) nfilts += 1;
            const std::vector<float> rrc = root_raised_cosine(1, target, target / sps_eff, 0.2, nfilts);
            symf_nt = (int)rrc.size();
            if ((r = symf_taps.upload(rrc))) return r;
            demod_gain = (float)(sps_eff / (1 * M_PI / 2));
        } else {
            const auto up2 = complex_band_pass(1, target, -fw, 0, fw, WIN_BLACKMAN_HARRIS);
            const auto lo2 = complex_band_pass(1, target, 0, fw, fw, WIN_BLACKMAN_HARRIS);
            disc_nt = (int)up2.size();
            // the discriminator kernels use the pair as what it is -- lower = conj(upper), bit for bit (same prototype, cos(-x) = cos(x),
            // sin(-x) = -sin(x)) -- and run the shared real-tap chains once (oracle orc_fir_ccc_conj_pair)
            for (size_t k = 0; k < up2.size(); ++k) {
                const float ur = up2[k].real(), ui = -up2[k].imag(), lr = lo2[k].real(), li = lo2[k].imag();
                if (std::memcmp(&ur, &lr, sizeof ur) || std::memcmp(&ui, &li, sizeof ui)) return qrl_set_error(QRL_ERR_ARG, "2FSK discriminator filters are not a conjugate pair");
            }
            if ((r = disc_up.upload(to_f2(up2))) || (r = disc_lo.upload(to_f2(lo2)))) return r;
            const std::vector<float> sf = low_pass(1.0, target, target / sps_eff, target / sps_eff, WIN_HAMMING);
            symf_nt = (int)sf.size();
            if ((r = symf_taps.upload(sf))) return r;
            // zero-padded copies for the fused kernel (4 A + 1 taps, tables of 4 (A + 1) entries)
            auto padf = [](std::vector<float> v) { v.resize((size_t)fsk2_ff_padded((int)v.size()) + 3, 0.0f); return v; };
            auto padc = [](std::vector<float2> v) { v.resize((size_t)fsk2_ff_padded((int)v.size()) + 3, make_float2(0.f, 0.f)); return v; };
            const std::vector<float> ftaps = low_pass(1, target, fw, fw, WIN_BLACKMAN_HARRIS);
            if ((r = ff_tf.upload(padf(ftaps))) || (r = ff_ts.upload(padf(sf))) || (r = ff_up.upload(padc(to_f2(up2)))) ||
                (r = ff_lo.upload(padc(to_f2(lo2))))) return r;
        }
        const float symbol_rate = (float)target / (float)sps_eff;
        const float dev = 200.0f / symbol_rate;
        clock_loop_gains((float)(2 * M_PI / (symbol_rate / 10)), 1.0f, 0.2869f, ss_alpha, ss_beta);
        ss_maxp = (float)sps_eff + dev; ss_minp = (float)sps_eff - dev;
    } else if (fam == F_DMR && m17) {
        const std::vector<float> rrc = root_raised_cosine(1.5, target, target / sps_eff, 0.5, 50 * sps_eff); // gr_demod_m17.cpp:64-67
        symf_nt = (int)rrc.size();
        if ((r = symf_taps.upload(rrc))) return r;
        demod_gain = (float)(sps_eff / M_PI);                                                                // :63
        const float symbol_rate = (float)target / (float)sps_eff;
        clock_loop_gains((float)(2 * M_PI / (symbol_rate / 50)), 1.0f, 0.2869f, ss_alpha, ss_beta);          // :70-71
        ss_maxp = (float)sps_eff + 500.0f / symbol_rate; ss_minp = (float)sps_eff - 500.0f / symbol_rate;
    } else if (fam == F_DMR) {
        const std::vector<float> rrc = root_raised_cosine(1, target, target / sps_eff, 0.2, 25 * sps_eff);   // gr_demod_dmr.cpp:62-66
        symf_nt = (int)rrc.size();
        if ((r = symf_taps.upload(rrc))) return r;
        demod_gain = (float)(target / (M_PI / 2 * (float)(target / sps_eff)));                               // :72
        clock_loop_gains((float)(2 * M_PI / 100.0f), 1.0f, 0.2869f, ss_alpha, ss_beta);                      // :70-71
        ss_maxp = (float)sps_eff + 0.06f; ss_minp = (float)sps_eff - 0.06f;
    } else if (fam == F_4FSK && fsk4_disc) {
        const int rs = sps == 1 ? 10000 : sps == 5 ? 2000 : 1000, bw = sps == 10 ? 2000 : 4000;           // gr_demod_4fsk.cpp:45-76
        const int lo_[4] = {-fw, -fw + rs, 0, fw - rs}, hi_[4] = {-fw + rs, 0, fw - rs, fw};                  // _filter1..4, :112-119
        std::vector<float2> bt;
        for (int q = 0; q < 4; ++q) {
            const auto t4 = complex_band_pass(1, target, lo_[q], hi_[q], bw, WIN_BLACKMAN_HARRIS);
            disc4_nt = (int)t4.size();
            const auto f2 = to_f2(t4);
            bt.insert(bt.end(), f2.begin(), f2.end());
        }
        if ((r = disc4_taps.upload(bt))) return r;
        const std::vector<float> st4 = low_pass(1.0, target, target / sps_eff, target / sps_eff / 20, WIN_BLACKMAN_HARRIS);   // :103-105
        sym4_nt = (int)st4.size();
        if ((r = sym4_taps.upload(st4)) || (r = s2g.alloc(ring2)) || (r = s2l.alloc(ring2))) return r;
        if ((r = tanh_tab.upload(tanh_table())) || (r = qp_st.alloc(B))) return r;
        clock_loop_gains((float)(2 * M_PI / 200.0f), 1.0f, 0.2869f, ss_alpha, ss_beta);                      // :138-140
        ss_maxp = (float)sps_eff + 0.05f; ss_minp = (float)sps_eff - 0.05f;
    } else if (fam == F_4FSK) {
        int nfilts = (sps == 1 ? 32 : sps == 2 ? 50 : 25) * sps_eff;                                         // gr_demod_4fsk.cpp:45-84
        if ((nfilts % 2) == 0) nfilts += 1;
        const std::vector<float> rrc = root_raised_cosine(1.5, target, target / sps_eff, 0.2, nfilts);       // :130-133
        symf_nt = (int)rrc.size();
        if ((r = symf_taps.upload(rrc))) return r;
        demod_gain = (float)(sps_eff / (1 * M_PI));                                                          // :129
        clock_loop_gains((float)(2 * M_PI / 200.0f), 1.0f, 0.2869f, ss_alpha, ss_beta);                      // :135-137
        ss_maxp = (float)sps_eff + 0.05f; ss_minp = (float)sps_eff - 0.05f;
    } else if (fam == F_BPSK) {
        std::vector<std::complex<float>> lo, up;
        fll_band_edge_taps((float)sps_eff, 0.35f, 32, lo, up);                                               // gr_demod_bpsk.cpp:63
        if ((r = fll_lo.upload(to_f2(lo))) || (r = fll_up.upload(to_f2(up)))) return r;
        control_loop_gains((float)(8 * M_PI / 100), fll_alpha, fll_beta);
        fll_maxf = (float)(2 * M_PI * (2.0 / sps_eff));
        if ((r = fll_st.alloc(B))) return r;
        if ((r = tanh_tab.upload(tanh_table())) || (r = qp_st.alloc(B))) return r;
        control_loop_gains((float)(2 * M_PI / 200), c2_alpha, c2_beta);                                      // _costas_loop, :61
    } else if (fam == F_QPSK) {
        if ((r = tanh_tab.upload(tanh_table())) || (r = qp_st.alloc(B))) return r;
        control_loop_gains((float)(M_PI / 200 / sps_eff), c1_alpha, c1_beta);     // _costas_pll, gr_demod_qpsk.cpp:110
        control_loop_gains((float)(qpsk_fll ? M_PI / 200 : M_PI / 400), c2_alpha, c2_beta);   // _costas_loop, :44,67,112
        if (qpsk_fll) {   // _fll = fll_band_edge_cc(sps, 0.35, 32, 2 pi / 100), :98-99
            std::vector<std::complex<float>> lo, up;
            fll_band_edge_taps((float)sps_eff, 0.35f, 32, lo, up);
            if ((r = fll_lo.upload(to_f2(lo))) || (r = fll_up.upload(to_f2(up)))) return r;
            control_loop_gains((float)(2 * M_PI / 100), fll_alpha, fll_beta);
            fll_maxf = (float)(2 * M_PI * (2.0 / sps_eff));
            if ((r = fll_st.alloc(B))) return r;
        }
        const float symbol_rate = (float)target / (float)sps_eff;
        const float dev = 200.0f / symbol_rate;
        clock_loop_gains((float)(2 * M_PI / (symbol_rate / 10)), 1.0f, 0.2869f, ss_alpha, ss_beta);
        ss_maxp = (float)sps_eff + dev; ss_minp = (float)sps_eff - dev;
        const float ang = (float)(-3 * M_PI / 4);
        qp_rot = make_float2((float)std::cos((double)ang), (float)std::sin((double)ang));
    } else {
        const std::vector<float> sf = low_pass(1, target, target / sps_eff, target / sps_eff, WIN_HAMMING);
        symf_nt = (int)sf.size();
        if ((r = symf_taps.upload(sf))) return r;
        demod_gain = (float)(sps_eff / (M_PI / 2));
        clock_loop_gains((float)(2 * M_PI / 200.0f), 1.0f, 0.2869f, ss_alpha, ss_beta);
        ss_maxp = (float)sps_eff + 0.05f; ss_minp = (float)sps_eff - 0.05f;
    }
    if ((r = ss_st.alloc(B)) || (r = fec_st.alloc((size_t)B * 2)) || (r = counts_scratch.alloc((size_t)B * 4))) return r;
    if (loops_family() && (r = qp_snap.alloc((size_t)B * 2))) return r;
    if ((fam == F_ANALOG && (r = an.build(*this, mx.n2))) || (fam == F_DSSS && (r = ds.build(*this, mx.n2)))) return r;
    return init_state();
}

int qrl_demod::process(const void* iq, size_t stride, size_t n, const qrl_demod_out* out, int fmt)
{
    if (fmt >= IN_SC8 && !fe.used && !iq8_baseband)   // (QRL_OPT_SC16_BASEBAND admits int16 only; 8-bit calls have QRL_OPT_IQ8_BASEBAND)
        return qrl_set_error(QRL_ERR_ARG, std::string(in_fmt_entry(fmt)) + ": 8-bit input needs the device-rate front end (device_samp_rate >= 2000000); this handle runs at 1 Msps and its missing front end is what converts");
    if (fmt == IN_SC16 && !fe.used && !sc16_baseband)
        return qrl_set_error(QRL_ERR_ARG, "qrl_demod_process_sc16: int16 input needs the device-rate front end (device_samp_rate >= 2000000); this handle runs at 1 Msps");
    if (n > cfg.max_chunk) return qrl_set_error(QRL_ERR_TOO_BIG, "n exceeds max_chunk");
    if (fmt >= IN_SC8) {
        if (!iq8_rows_ok(in_fmt_entry(fmt), iq, stride)) return QRL_ERR_ARG;
    } else if (fmt == IN_SC16) {
        if (!sc16_rows_ok("qrl_demod_process_sc16", iq, stride)) return QRL_ERR_ARG;
    } else if ((reinterpret_cast<uintptr_t>(iq) & 15u) || (stride & 1u)) return qrl_set_error(QRL_ERR_ARG, "iq must be 16-byte aligned, stride even");
    const int B = cfg.batch;
    uint32_t* counts = (out && out->counts) ? out->counts : counts_scratch.p;
    hipStream_t cs = overlap ? tail : stream;   // stream of stage C (decimated-rate feed-forward kernels)
    const int slot = (int)(call_no & 1);
    if (overlap) {
        // ring s2 is about to be overwritten two calls behind: the tail of call k - 2 must be through
        QRLCHK(ev_tail2[slot].wait(stream));
    } else {
        HIPCHK(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(uint32_t), stream));
    }
    // loops families: the rings the recursion reads hold two calls; call k - 2's recursion must be through before they are rewritten
    if (loops_family()) QRLCHK(ev_q[slot].wait(stream));
    if (grouped) QRLCHK(ev_q[slot ^ 1].wait(stream));   // grouped order: this front end behind the recursion of the call before
    QRLCHK(ev_pre.wait_once(stream));   // k_hist of the call before (helper stream)
    const bool use_pre = pre && input_resident;
    const float2* in = reinterpret_cast<const float2*>(iq);   // (IN_SC16, IN_SC8, IN_CU8: integer pairs behind it; only the kernels that read the caller's buffer know: the front end or, without one, what input_source feeds, and k_hist)
    const float2* hist_old = hist_flip ? hist_b.p : hist_a.p;
    const PortC fport = filtered_port(out), cport = constellation_port(out);
    float2* hist_new = hist_flip ? hist_a.p : hist_b.p;

    const uint64_t n_in0 = n_in, n_in1 = n_in + n;
    uint64_t n1_0 = n1, n1_1 = n1;
    RingC r2{s2.p, s2_mask}, r2l{s2l.p, s2_mask}, r2f{s2f.p, s2_mask};
    RingF r2d{s2d.p, s2_mask}, r3{s3.p, s2_mask};

    // the HBM-facing kernel is the first launch that reads the caller's IQ
    if (profiling) QRLCHK(prof.begin(stream));
    // ---- stage A: gr_demod_base front end
    if (fe.used) {
        n1_1 = decim_count(n_in1, 1, fe_decim);
        DecimParams p{};
        p.in = in; p.in_stride = stride; p.n0 = n_in0; p.n = (uint32_t)n;
        p.hist = hist_old; p.hist_len = hist_len;
        p.out = RingC{s1.p, s1_mask}; p.m0 = n1_0; p.m_count = (uint32_t)(n1_1 - n1_0);
        p.taps = fe.taps.p; p.D = fe.D; p.Jpad = fe.c.Jpad;
        p.rot_enable = 1; rot.fill(p);
        in_format_fill(p, in_format(fmt));
        if (use_pre) { p.pre_stream = pre; p.pre_event = ev_pre; }
        if (fe.launch(p, B, stream, use_pre ? slot : 0)) return qrl_set_error(QRL_ERR_HIP, "front-end launch: hipFuncSetAttribute failed");
    }
    if (profiling && fe.used) QRLCHK(prof.end(stream));
    // ---- stage B: per-mode resampler
    const uint64_t src0 = fe.used ? n1_0 : n_in0, src1 = fe.used ? n1_1 : n_in1;
    const uint64_t n2_0 = n2, n2_1 = decim_count(src1, interp, decim);
    if (interp == 1) {
        DecimParams p{};
        input_source(p, in, stride, hist_old, src0, src1, fmt);
        p.out = r2; p.m0 = n2_0; p.m_count = (uint32_t)(n2_1 - n2_0);
        p.taps = first.taps.p; p.D = first.D; p.Jpad = first.c.Jpad;
        if (d2f) {   // + _shaping_filter -> port 0 and the filtered ring, in the same kernel
            Dec2FirParams f{};
            f.d = p; f.taps = d2f_taps.p; f.out = RingC{s2f.p, s2_mask};
            f.port = fport.p; f.port_cap = fport.cap; f.counts = counts;
            launch_dec2_fir(f, B, stream);
        } else {
            if (use_pre && !fe.used) { p.pre_stream = pre; p.pre_event = ev_pre; }   // (device rate 1 Msps: this stage is the one that reads the caller's IQ)
            if (first.launch(p, B, stream, use_pre && !fe.used ? slot : 0)) return qrl_set_error(QRL_ERR_HIP, "first-stage launch: hipFuncSetAttribute failed");
        }
    } else {
        ResampParams p{};
        input_source(p, in, stride, hist_old, src0, src1, fmt);
        p.out = r2; p.q0 = n2_0; p.q_count = (uint32_t)(n2_1 - n2_0);
        p.taps = rs_taps.p; p.I = interp; p.D = decim; p.Jp = rs_Jp;
        if (fam == F_DMR && !m17) {   // port 0 of gr_demod_dmr is the resampler output (gr_demod_dmr.cpp:89)
            p.port = fport.p; p.port_cap = fport.cap; p.port_counts = counts;
        }
        launch_resamp(p, B, stream);
    }
    if (profiling && !fe.used) QRLCHK(prof.end(stream));
    // ---- time-domain scope tap: the 1 Msps signal behind the front end (the caller's rotated IQ when the device runs at 1 Msps) -> 1:10
    if (scope_out) {
        const uint64_t ns_1 = decim_count(src1, 1, scope_D);
        DecimParams p{};
        input_source(p, in, stride, hist_old, src0, src1, fmt);
        p.out = RingC{s_scope.p, scope_mask}; p.m0 = n_scope; p.m_count = (uint32_t)(ns_1 - n_scope);
        p.taps = scope.taps.p; p.D = scope.D; p.Jpad = scope.c.Jpad;
        if (scope.launch(p, B, stream)) return qrl_set_error(QRL_ERR_HIP, "scope launch: hipFuncSetAttribute failed");
        launch_ring_store(RingC{s_scope.p, scope_mask}, n_scope, (uint32_t)(ns_1 - n_scope), scope_out, scope_cap, scope_counts, B, stream);
        n_scope = ns_1;
    }
    // keep the tail of the caller's IQ (rotated) for the next call
    {
        HistParams h{};
        h.in = in; h.in_stride = stride; h.n0 = n_in0; h.n = (uint32_t)n;
        h.hist_old = hist_old; h.hist_new = hist_new; h.hist_len = hist_len;
        h.rot_enable = 1; rot.fill(h);
        in_format_fill(h, in_format(fmt));
        if (pre) QRLCHK(ev_fe[slot].record(stream));   // everything of this call that reads the history on the handle's stream has been launched
        if (use_pre) {
            QRLCHK(ev_fe[slot ^ 1].wait(pre));   // hist_new was the history of the call before
            launch_hist_save(h, B, pre);
            QRLCHK(ev_pre.record(pre));
        } else launch_hist_save(h, B, stream);
        hist_flip = !hist_flip;
    }
    if (overlap) {
        QRLCHK(ev_ff.relay(stream, tail));
        HIPCHK(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(uint32_t), tail));
    }
    // ---- stage C: decimated-rate feed-forward (+ FLL for 2FSK)
    const uint32_t c2 = (uint32_t)(n2_1 - n2_0);
    if (fam == F_DSSS || fam == F_ANALOG) {
        if (int rr = fam == F_DSSS ? ds.stages(*this, n2_0, n2_1, out, counts) : an.stages(*this, n2_0, n2_1, out, counts)) return rr;
        HIPCHK(hipGetLastError());
        if (take_launch_error()) return QRL_ERR_HIP;
        n_in = n_in1; n1 = n1_1; n2 = n2_1; ++call_no;
        return QRL_OK;
    }
    RingC filt_in = r2;
    const bool fused_2fsk = fam == F_2FSK && !fm && filt_nt <= 41 && disc_nt <= 41 && symf_nt <= 25;
    // the FLL and the three FIR stages in one kernel (k_2fsk_tail): gr_demod_2fsk's 41 + 41 + 25 designs; QRL_OPT_FLL_SLIM = 1 keeps the pair of kernels
    const bool tail_fused = fsk2_tail_eligible(fused_2fsk, 16, fsk2_ff_padded(filt_nt), fsk2_ff_padded(disc_nt), fsk2_ff_padded(symf_nt), fll_slim);
    FllParams fllp{};
    if (fam == F_2FSK || fam == F_BPSK || (fam == F_QPSK && qpsk_fll)) {
        FllParams& f = fllp;
        f.in = r2; f.out = r2l; f.q0 = n2_0; f.count = c2; f.st = fll_st.p;
        f.lower = fll_lo.p; f.upper = fll_up.p; f.nt = fam == F_2FSK ? 16 : 32; f.alpha = fll_alpha; f.beta = fll_beta; f.max_freq = fll_maxf;
        // (slim single-wave FLL workgroups under an 8-wave-workgroup front end were measured in round 3: the front end alone slows from
        //  6.57 to 7.24 ms with 8-wave workgroups and stretches to 8.4 - 9.1 ms when it shares the SIMDs; 9.47 ms per step against 9.29)
        f.slim = fll_slim ? 1 : 0;
        if (!(QRL_DEV_SKIP & 1) && !tail_fused) launch_fll(f, B, cs);
        filt_in = r2l;
    }
    if (fam == F_DMR) {
        RingC dem_in = r2;
        if (m17) {   // gr_demod_m17.cpp:60-61,89-90: channel filter behind the resampler, its output is port 0
            FirCcfParams f{};
            f.in = r2; f.out = r2f; f.q0 = n2_0; f.count = c2; f.taps = filt_taps.p; f.nt = filt_nt;
            f.port = fport.p; f.port_cap = fport.cap; f.counts = counts;
            launch_fir_ccf(f, B, cs);
            dem_in = r2f;
        }
        QuadDemodParams q{}; q.in = dem_in; q.out = r2d; q.q0 = n2_0; q.count = c2; q.gain = demod_gain; q.atan_tab = atan_tab.p;
        launch_quad_demod(q, B, cs);
        if (!overlap) QRLCHK(ev_tail.wait_once(stream));
        FirFffParams f{}; f.in = r2d; f.out = r3; f.q0 = n2_0; f.count = c2; f.taps = symf_taps.p; f.nt = symf_nt;
        launch_fir_fff(f, B, cs);
        if (!overlap) QRLCHK(ev_ff.relay(stream, tail));
    } else if (fused_2fsk) {
        if (!overlap) QRLCHK(ev_tail.wait_once(stream));
        Fsk2FfParams f{};
        f.in = filt_in; f.out = r3; f.q0 = n2_0; f.count = c2;
        f.tf = ff_tf.p; f.nf = fsk2_ff_padded(filt_nt); f.up = ff_up.p; f.lo = ff_lo.p; f.nb = fsk2_ff_padded(disc_nt);
        f.ts = ff_ts.p; f.ns = fsk2_ff_padded(symf_nt);
        f.port = fport.p; f.port_cap = fport.cap; f.counts = counts;
        if (tail_fused) {   // r2l keeps only the call's last windows of y: the history both forms start from
            Fsk2TailParams t{}; t.fll = fllp; t.ff = f;
            if (!(QRL_DEV_SKIP & 3)) launch_2fsk_tail(t, B, cs);
        } else if (!(QRL_DEV_SKIP & 2)) launch_2fsk_ff(f, B, cs);
        if (!overlap) QRLCHK(ev_ff.relay(stream, tail));
    } else {
        if (!d2f) {
            FirCcfParams f{};
            f.in = filt_in; f.out = r2f; f.q0 = n2_0; f.count = c2; f.taps = filt_taps.p; f.nt = filt_nt;
            f.port = fport.p; f.port_cap = fport.cap; f.counts = counts;
            launch_fir_ccf(f, B, cs);
        }
        if (fam == F_QPSK || fam == F_BPSK) {
            // recursive chain + Viterbi below; nothing else at the sample rate
        } else if (fsk4_disc) {
            RingC r2l4{s2l.p, s2_mask}, r2g{s2g.p, s2_mask};
            Disc4fskParams d{}; d.in = r2f; d.out = r2l4; d.q0 = n2_0; d.count = c2; d.taps = disc4_taps.p; d.nt = disc4_nt;
            launch_disc_4fsk(d, B, cs);
            FirCcfParams f{}; f.in = r2l4; f.out = r2g; f.q0 = n2_0; f.count = c2; f.taps = sym4_taps.p; f.nt = sym4_nt;   // _symbol_filter
            launch_fir_ccf(f, B, cs);
        } else if (fam == F_GMSK || fam == F_4FSK || fm) {
            QuadDemodParams q{}; q.in = r2f; q.out = r2d; q.q0 = n2_0; q.count = c2; q.gain = demod_gain; q.atan_tab = atan_tab.p;
            launch_quad_demod(q, B, cs);
        } else {
            Disc2fskParams d{}; d.in = r2f; d.out = r2d; d.q0 = n2_0; d.count = c2; d.up = disc_up.p; d.lo = disc_lo.p; d.nt = disc_nt;
            launch_disc_2fsk(d, B, cs);
        }
        if (fam == F_QPSK || fam == F_BPSK || fsk4_disc) {
            // the tail reads r2f (written by k_fir_ccf above): it runs on the handle's own stream for these families
        } else {
            // r3 is what the previous call's tail (other stream) may still be reading
            if (!overlap) QRLCHK(ev_tail.wait_once(stream));
            FirFffParams f{}; f.in = r2d; f.out = r3; f.q0 = n2_0; f.count = c2; f.taps = symf_taps.p; f.nt = symf_nt;
            launch_fir_fff(f, B, cs);
            if (!overlap) QRLCHK(ev_ff.relay(stream, tail));
        }
    }
    // ---- stage D: symbol sync + FEC
    if (fam == F_QPSK || fam == F_BPSK || fsk4_disc) {
        QpskParams q{};
        q.in = fsk4_disc ? RingC{s2g.p, s2_mask} : r2f; q.np0 = n2_0; q.avail = n2_1; q.soft = RingB{soft.p, soft_mask}; q.st = qp_st.p;
        q.mmse = mmse_tab.p; q.tanh_tab = tanh_tab.p;
        q.c1_alpha = c1_alpha; q.c1_beta = c1_beta; q.c2_alpha = c2_alpha; q.c2_beta = c2_beta;
        q.ss_alpha = ss_alpha; q.ss_beta = ss_beta; q.ss_maxp = ss_maxp; q.ss_minp = ss_minp;
        q.rot = qp_rot; q.soft_mul = 48.0f; q.soft_add = 128.0f;
        if (fsk4_disc) { q.mode = 2; q.soft_mul = 128.0f; }   // gr_demod_4fsk.cpp:138-146,186-195
        if (fam == F_BPSK) {   // gr_demod_bpsk.cpp:54-62,67
            q.mode = 1; q.soft_mul = 64.0f;
            const float gain_omega = 0.005f;
            q.cr_gain_omega = gain_omega * gain_omega; q.cr_gain_mu = 0.05f;
            q.cr_omega_mid = (float)sps_eff; q.cr_omega_lim = 0.001f * (float)sps_eff;
        }
        q.port = cport.p; q.port_cap = cport.cap; q.counts = counts;
        q.oo_snap = qp_snap.p + (size_t)slot * B;
        // recursion on `tail` behind this call's feed-forward kernels, decoder on `fecs` behind the recursion
        QRLCHK(ev_ff.relay(stream, tail));
        QRLCHK(ev_fec[slot].wait(tail));   // the soft ring holds two calls: decoder of call k - 2 done (grouped order: launched, and this recorded, by the call between)
        launch_qpsk_loops(q, B, tail);
        QRLCHK(ev_q[slot].record(tail));
        QRLCHK(flush_fec(true));                                    // grouped order: the decoder of the call before goes with this recursion
        if (!grouped) QRLCHK(ev_q[slot].wait(fecs));
        FecParams f{};
        f.soft = RingB{soft.p, soft_mask};
        f.avail = q.oo_snap; f.avail_stride = sizeof(uint64_t); f.avail_mul = fam == F_BPSK ? 1 : 2;
        f.st = fec_st.p;
        f.bits_a = out ? out->bits_a : nullptr; f.bits_b = fam == F_BPSK && out ? out->bits_b : nullptr; f.bits_cap = out ? out->bits_cap : 0;
        f.counts = counts; f.branches = fam == F_BPSK ? 2 : 1;
        if (grouped) { fec_pending = f; fec_pending_slot = slot; fec_deferred = true; }
        else {
            launch_fec(f, B, fecs);
            QRLCHK(ev_fec[slot].record(fecs));
        }
    } else {
        SymSyncParams s{};
        s.in = r3; s.avail = n2_1; s.soft = RingB{soft.p, soft_mask}; s.st = ss_st.p; s.mmse = mmse_tab.p;
        s.alpha = ss_alpha; s.beta = ss_beta; s.maxp = ss_maxp; s.minp = ss_minp;
        s.ted = fam == F_DMR && !m17 ? 0 : 1; s.soft_mul = 128.0f; s.soft_add = 128.0f;
        s.tail_scale = m17 ? 1.0f : 0.9f;
        // overlapped order: the 25 KB geometry (k_symsync_ff<16, 96>), whose workgroups fit beside two front-end workgroups on a CU.  The
        // 74 KB one was placed only as the front end of the next call drained -- 4.1 ms instead of 0.25, the decoder behind it, and the
        // front end after next waiting 0.5 ms per step for the ring this tail frees (profiles/r04_c1_timeline.log).
        s.slim = overlap ? 1 : 0;
        s.slicer = fam == F_DMR || fam == F_4FSK ? 1 : 0; s.tail = fam == F_DMR ? 1 : fam == F_4FSK ? 2 : 0;
        s.bits = out ? out->bits_a : nullptr; s.bits_cap = out ? out->bits_cap : 0;
        s.port = cport.p; s.port_cap = cport.cap; s.counts = counts;
        if (!(QRL_DEV_SKIP & 4)) launch_symsync_ff(s, B, tail);
        if (fam == F_DMR && !m17 && dmo_out) {   // gr_dmr_dmo_sink on port 3 (= ring r3) of this call
            DmoParams dp{}; dp.in = r3; dp.q0 = n2_0; dp.count = (uint32_t)(n2_1 - n2_0); dp.st = dmo_st.p; dp.golay = dmo_golay.p;
            dp.out = dmo_out; dp.cap = dmo_cap; dp.counts = dmo_counts;
            launch_dmo_sink(dp, B, tail);
        }
        if (fam == F_DMR) QRLCHK(ev_tail.record(tail));
        FecParams f{};
        f.soft = RingB{soft.p, soft_mask}; f.avail = &ss_st.p[0].oo; f.avail_stride = sizeof(SymSyncState); f.avail_mul = fam == F_4FSK ? 2 : 1; f.st = fec_st.p;
        f.bits_a = out ? out->bits_a : nullptr; f.bits_b = out ? out->bits_b : nullptr; f.bits_cap = out ? out->bits_cap : 0;
        f.counts = counts; f.branches = branches;
        if (fam != F_DMR) {
            if (!(QRL_DEV_SKIP & 8)) launch_fec(f, B, tail);
            QRLCHK(ev_tail.record(tail));
        }
        if (overlap) QRLCHK(ev_tail2[slot].record(tail));
    }
    HIPCHK(hipGetLastError());
    if (take_launch_error()) return QRL_ERR_HIP;   // (message already recorded by dyn_lds_limit)
    n_in = n_in1; n1 = n1_1; n2 = n2_1; ++call_no;
    return QRL_OK;
}

// One row per receiver mode: the family that runs it and, for use_mode_defaults, the literals the reference constructs it with
// (gr_demod_base.cpp:203-210: samp_rate 1 000 000, carrier_freq 1700).  kind (analogue receivers): 0 NBFM, 1 AM, 2 WBFM, 3 SSB.
namespace {
struct Mode { int modem_type; qrl_demod::Family fam; int kind; bool m17, lsb; int sps, filter_width, fm; };
const Mode kModes[] = {
    {QRL_MODEM_2FSK2KFM,  qrl_demod::F_2FSK,   0, false, false, 5,   4000,   1},
    {QRL_MODEM_2FSK1KFM,  qrl_demod::F_2FSK,   0, false, false, 10,  2500,   1},
    {QRL_MODEM_2FSK2K,    qrl_demod::F_2FSK,   0, false, false, 5,   4000,   0},
    {QRL_MODEM_2FSK1K,    qrl_demod::F_2FSK,   0, false, false, 10,  2000,   0},
    {QRL_MODEM_2FSK10KFM, qrl_demod::F_2FSK,   0, false, false, 1,   25000,  1},
    {QRL_MODEM_GMSK2K,    qrl_demod::F_GMSK,   0, false, false, 5,   4000,   0},
    {QRL_MODEM_GMSK1K,    qrl_demod::F_GMSK,   0, false, false, 10,  2000,   0},
    {QRL_MODEM_GMSK10K,   qrl_demod::F_GMSK,   0, false, false, 1,   20000,  0},
    {QRL_MODEM_QPSK250K,  qrl_demod::F_QPSK,   0, false, false, 2,   160000, 0},   // gr_demod_base.cpp:223
    {QRL_MODEM_QPSKVIDEO, qrl_demod::F_QPSK,   0, false, false, 2,   160000, 0},   // :224
    {QRL_MODEM_QPSK2K,    qrl_demod::F_QPSK,   0, false, false, 125, 1300,   0},   // :221
    {QRL_MODEM_QPSK20K,   qrl_demod::F_QPSK,   0, false, false, 25,  6500,   0},   // :222
    {QRL_MODEM_4FSK2K,    qrl_demod::F_4FSK,   0, false, false, 5,   4000,   0},   // gr_demod_base.cpp:211
    {QRL_MODEM_4FSK2KFM,  qrl_demod::F_4FSK,   0, false, false, 5,   3000,   1},   // gr_demod_base.cpp:212
    {QRL_MODEM_4FSK1KFM,  qrl_demod::F_4FSK,   0, false, false, 10,  2000,   1},   // :213
    {QRL_MODEM_4FSK10KFM, qrl_demod::F_4FSK,   0, false, false, 1,   20000,  1},   // :214
    {QRL_MODEM_4FSK100K,  qrl_demod::F_4FSK,   0, false, false, 2,   125000, 1},   // :225
    {QRL_MODEM_BPSK1K,    qrl_demod::F_BPSK,   0, false, false, 10,  1300,   0},   // :216
    {QRL_MODEM_BPSK2K,    qrl_demod::F_BPSK,   0, false, false, 5,   2400,   0},   // :217
    {QRL_MODEM_DMR,       qrl_demod::F_DMR,    0, false, false, 5,   5000,   0},   // make_gr_demod_dmr(5, 1000000) gr_demod_base.cpp:253
    {QRL_MODEM_M17,       qrl_demod::F_DMR,    0, true,  false, 125, 9000,   0},   // make_gr_demod_m17() gr_demod_base.cpp:252, defaults gr_demod_m17.h:41-42
    {QRL_MODEM_BPSK8,     qrl_demod::F_DSSS,   0, false, false, 25,  150,    0},   // make_gr_demod_dsss(25, ., 1700, 150) gr_demod_base.cpp:218
    {QRL_MODEM_NBFM2500,  qrl_demod::F_ANALOG, 0, false, false, 125, 2500,   0},   // make_gr_demod_nbfm(125, ., 1700, 2500) gr_demod_base.cpp:219
    {QRL_MODEM_NBFM5000,  qrl_demod::F_ANALOG, 0, false, false, 125, 5000,   0},   // :220
    {QRL_MODEM_AM5000,    qrl_demod::F_ANALOG, 1, false, false, 125, 5000,   0},   // make_gr_demod_am(125, ., 1700, 5000) :215
    {QRL_MODEM_WBFM,      qrl_demod::F_ANALOG, 2, false, false, 125, 75000,  0},   // make_gr_demod_wbfm(125, ., 1700, 75000) :228
    {QRL_MODEM_USB2500,   qrl_demod::F_ANALOG, 3, false, false, 125, 2700,   0},   // make_gr_demod_ssb(125, ., 1700, 2700, sb) :226-227
    {QRL_MODEM_LSB2500,   qrl_demod::F_ANALOG, 3, false, true,  125, 2700,   0},   // :227
};
}  // namespace

// =============================================================================== C ABI
extern "C" {

const char* qrl_version(void) { return "qrl_hip 0.1 (gfx950)"; }

int qrl_init(int device, qrl_ctx** ctx)
{
    if (!ctx) return QRL_ERR_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return qrl_set_error(QRL_ERR_NO_DEVICE, "hipGetDeviceCount: no device");
    if (device < 0 || device >= count) return qrl_set_error(QRL_ERR_NO_DEVICE, "device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && std::strncmp(prop.gcnArchName, "gfx94", 5) != 0)
        return qrl_set_error(QRL_ERR_NO_DEVICE, std::string("unsupported architecture ") + prop.gcnArchName);
    *ctx = new (std::nothrow) qrl_ctx{device};
    return *ctx ? QRL_OK : QRL_ERR_NOMEM;
}
void qrl_shutdown(qrl_ctx* ctx) { delete ctx; }

int qrl_demod_create(qrl_ctx* ctx, const qrl_demod_config* cfg, qrl_demod** outp)
{
    if (!ctx || !cfg || !outp) return QRL_ERR_ARG;
    if (cfg->batch < 1 || cfg->max_chunk < 1) return qrl_set_error(QRL_ERR_ARG, "batch and max_chunk must be >= 1");
    std::unique_ptr<qrl_demod> d(new (std::nothrow) qrl_demod);
    if (!d) return QRL_ERR_NOMEM;
    d->ctx = ctx;
    d->cfg = *cfg;
    qrl_demod_config& c = d->cfg;
    const Mode* mode = nullptr;
    for (const Mode& m : kModes) if (m.modem_type == c.modem_type) mode = &m;
    if (!mode) return qrl_set_error(QRL_ERR_ARG, "modem_type not supported by this build");
    if (c.use_mode_defaults) { c.samp_rate = 1000000; c.carrier_freq = 1700; c.sps = mode->sps; c.filter_width = mode->filter_width; c.fm = mode->fm; }
    d->fam = mode->fam; d->m17 = mode->m17; d->an.kind = mode->kind; d->an.lsb = mode->lsb;
    if (c.samp_rate != 1000000) return qrl_set_error(QRL_ERR_ARG, "internal samp_rate must be 1000000 (gr_demod_base.cpp:21)");
    if (c.device_samp_rate != 1000000 && (c.device_samp_rate < 2000000 || c.device_samp_rate % 1000000))
        return qrl_set_error(QRL_ERR_ARG, "device_samp_rate must be 1e6 or a multiple of 1e6 >= 2e6");
    HIPCHK(hipSetDevice(ctx->device));
    // Streams.  The tail stream has the highest priority and its kernels are small enough to take over the slot of ONE
    // retiring front-end workgroup.  (Reserving CUs for it with a CU mask was measured: it costs the front end ~18 %.)
    {
        QRLCHK(d->stream.open(c.hip_stream, "MAIN", "QRL_MAIN_PRIO_LOW"));   // (the experiment: the masked tail only outranks the front end when the front end's stream is BELOW normal)
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        // THREE DIFFERENT PRIORITIES, and not for the scheduling: the runtime multiplexes the streams of one priority onto a few hardware
        // queues (least-used first), and two streams of a handle that land on the same queue run their kernels one after the other --
        // the overlapped and grouped orders then silently degrade to the serial one (seen as C4 4.5 instead of 3.05 ms and C2 2.2 instead
        // of 1.78 ms per step in the sub-lines of a long bench process, depending on how many streams the process had created and
        // destroyed before: tools/experiments/r04_subline_order*.py).  Queues of different priorities are never shared.
        QRLCHK(d->tail.open_internal(hi, "TAIL"));
        QRLCHK(d->fecs.open_internal(lo, "FEC"));
        // the front end's helper stream: the handle's own stream only (a caller's stream may share its hardware queue with anything), normal priority
        if (d->stream.owned() && !std::getenv("QRL_NO_PRE")) { QRLCHK(d->pre.open_internal(0, "PRE")); QRLCHK(d->ev_pre.create()); }
    }
    int r = d->build();
    if (r) return r;
    *outp = d.release();
    return QRL_OK;
}
void qrl_demod_destroy(qrl_demod* d) { if (d) { (void)d->sync_all(); delete d; } }

int qrl_demod_reset(qrl_demod* d)
{
    if (!d) return QRL_ERR_ARG;
    if (int rs = d->sync_all()) return rs;
    return d->init_state();
}
int qrl_demod_set_carrier_offset(qrl_demod* d, double hz)
{
    if (!d) return QRL_ERR_ARG;
    if (int rs = d->sync_all()) return rs;
    d->cfg.carrier_offset_hz = hz;
    return d->rot.retune(d->n_in, phase_inc_to_turn(2 * M_PI * -hz / d->cfg.device_samp_rate), d->stream);   // phase-continuous
}
int qrl_demod_set_carrier_offsets(qrl_demod* d, const double* hz)
{
    if (!d || !hz) return QRL_ERR_ARG;
    std::vector<uint64_t> ni;
    if (int r = carrier_incs(hz, d->cfg.batch, -1.0, d->cfg.device_samp_rate, ni)) return r;
    if (int rs = d->sync_all()) return rs;
    return d->rot.retune_streams(d->n_in, ni, d->stream);
}
int qrl_demod_stream_wait(qrl_demod* d, void* hip_stream)
{
    if (!d) return QRL_ERR_ARG;
    if (int rf = d->flush_fec(false)) return rf;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);
    const hipStream_t from[4] = {d->stream, d->tail, d->fecs, d->pre ? d->pre : d->stream};   // ([3]: k_hist reads the caller's IQ on the helper stream)
    for (int k = 0; k < 4; ++k) QRLCHK(d->ev_user[k].record(from[k]));
    for (auto& e : d->ev_user) QRLCHK(e.wait(user));
    return QRL_OK;
}
int qrl_demod_set_dmo_output(qrl_demod* d, uint8_t* frames, size_t cap_frames, uint32_t* counts)
{
    if (!d) return QRL_ERR_ARG;
    if (d->fam != qrl_demod::F_DMR || d->m17) return qrl_set_error(QRL_ERR_ARG, "the DMO slicer sits behind port 3 of gr_demod_dmr: QRL_MODEM_DMR only");
    // kernel parameters are captured at launch: swapping the output pointers between calls needs no synchronisation (a host layer
    // that double-buffers its mailboxes calls this before every process).  Only the first use (state allocation) and switching
    // the block off wait for the work in flight.
    if (!frames) { if (int rs = d->sync_all()) return rs; d->dmo_out = nullptr; return QRL_OK; }
    if (!counts || cap_frames < 1 || cap_frames > 0xFFFFFFFFu) return QRL_ERR_ARG;
    int r;
    if (!d->dmo_st.p) {
        if (int rs = d->sync_all()) return rs;
        if ((r = d->dmo_st.alloc(d->cfg.batch)) || (r = d->dmo_golay.upload(golay1987_table()))) return r;
        if ((r = d->init_dmo_state())) return r;
    }
    d->dmo_out = frames; d->dmo_cap = (uint32_t)cap_frames; d->dmo_counts = counts;
    return QRL_OK;
}
int qrl_demod_set_option(qrl_demod* d, int option, int value)
{
    if (!d) return QRL_ERR_ARG;
    switch (option) {
    case QRL_OPT_OVERLAP:
        if (value != 0 && !d->overlap_capable) return qrl_set_error(QRL_ERR_ARG, "overlapped mode exists for the 2FSK family only");
        if (int rs = d->sync_all()) return rs;
        d->overlap = value != 0;
        d->ev_tail2[0].disarm(); d->ev_tail2[1].disarm();
        return QRL_OK;
    case QRL_OPT_FLL_SLIM:
        if (int rs = d->sync_all()) return rs;
        d->fll_slim = value != 0;
        return QRL_OK;
    case QRL_OPT_GROUPED:
        if (value != 0 && !d->grouped_capable) return qrl_set_error(QRL_ERR_ARG, "the grouped order exists for the gr_demod_qpsk chain only");
        if (int rs = d->sync_all()) return rs;
        d->grouped = value != 0;
        return QRL_OK;
    case QRL_OPT_INPUT_RESIDENT: {
        if (int rs = d->sync_all()) return rs;
        if (value != 0 && d->pre) {   // the second edge scratch of the stage that reads the caller's IQ (the helper stages a call ahead)
            DecimStage& st = d->fe.used ? d->fe : d->first;
            if (st.edge_len && !st.edge_b.p) if (int r = st.edge_b.alloc((size_t)d->cfg.batch * st.edge_len)) return qrl_set_error(r, "edge scratch");
        }
        d->input_resident = value != 0;
        return QRL_OK;
    }
    case QRL_OPT_UNFUSED_DEC2:
        if (!d->d2f_capable) return qrl_set_error(QRL_ERR_ARG, "this chain has no fused 1:2 decimator + shaping filter");
        if (d->n_in != 0) return qrl_set_error(QRL_ERR_STATE, "QRL_OPT_UNFUSED_DEC2 can only be set before the first sample (the two forms carry different state)");
        d->d2f = value == 0;
        return QRL_OK;
    case QRL_OPT_SC16_BASEBAND:
        d->sc16_baseband = value != 0;   // read by the calls from now on: no state, nothing to wait for (a handle with a front end takes int16 anyway)
        return QRL_OK;
    case QRL_OPT_IQ8_BASEBAND:
        d->iq8_baseband = value != 0;    // the same for sc8 / cu8; the two options are independent
        return QRL_OK;
    default:
        return qrl_set_error(QRL_ERR_ARG, "unknown option");
    }
}
int qrl_demod_out_caps(const qrl_demod* d, size_t n, size_t* fcap, size_t* ccap, size_t* bcap)
{
    if (!d) return QRL_ERR_ARG;
    const CallCounts cc = d->call_counts(n);
    const size_t ns = cc.nsym;
    if (fcap) *fcap = cc.n2;
    if (ccap) *ccap = ns;
    if (bcap) *bcap = d->fam == qrl_demod::F_DMR ? 2 * ns + 8 : d->fam == qrl_demod::F_QPSK || d->fam == qrl_demod::F_4FSK ? (ns / 80 + 2) * 80 : (ns / 2 / 80 + 2) * 80;
    return QRL_OK;
}
int qrl_demod_time_domain_cap(const qrl_demod* d, size_t n, size_t* cap)
{
    if (!d || !cap) return QRL_ERR_ARG;
    *cap = d->call_counts(n).n1 / (size_t)d->scope_D + 2;
    return QRL_OK;
}
int qrl_demod_set_time_domain_output(qrl_demod* d, float* samples, size_t cap, uint32_t* counts)
{
    if (!d) return QRL_ERR_ARG;
    if (samples && !counts) return qrl_set_error(QRL_ERR_ARG, "qrl_demod_set_time_domain_output: counts [batch] required");
    HIPCHK(hipSetDevice(d->ctx->device));
    if (samples && !d->s_scope.p) {   // first use: the ring of the 100 ksps scope signal (one call + the stages' block granularity)
        if (int rs = d->sync_all()) return rs;
        d->scope_mask = pow2_at_least(d->call_counts(d->cfg.max_chunk).n1 / (size_t)d->scope_D + 256, 64) - 1;
        if (int r = d->s_scope.alloc((size_t)d->cfg.batch * (d->scope_mask + 1))) return qrl_set_error(r, "scope ring");
        // the tap starts with the samples of the next call: outputs are indexed from the stream's 1 Msps position
        d->n_scope = decim_count(d->fe.used ? d->n1 : d->n_in, 1, d->scope_D);
    }
    if (samples && !d->scope_out) d->n_scope = decim_count(d->fe.used ? d->n1 : d->n_in, 1, d->scope_D);   // (re-)enabled: skip what was not tapped
    d->scope_out = reinterpret_cast<float2*>(samples); d->scope_cap = cap; d->scope_counts = counts;
    return QRL_OK;
}
int qrl_demod_process(qrl_demod* d, const float* iq, size_t stride, size_t n, const qrl_demod_out* out)
{
    if (!d || (!iq && n)) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    (void)take_launch_error();   // a mark left on this thread by an earlier call that returned before reading it must not fail this one
    return d->process(iq, stride, n, out);
}
int qrl_demod_process_sc16(qrl_demod* d, const int16_t* iq, size_t stride, size_t n, const qrl_demod_out* out)
{
    if (!d || (!iq && n)) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    (void)take_launch_error();
    return d->process(iq, stride, n, out, IN_SC16);
}
int qrl_demod_set_sc16_scale(qrl_demod* d, float scale)
{
    if (!d) return QRL_ERR_ARG;
    if (!sc16_scale_ok("qrl_demod_set_sc16_scale", scale)) return QRL_ERR_ARG;
    d->sc16_scale = scale;   // a kernel parameter of the calls from now on; calls already queued keep theirs
    return QRL_OK;
}
int qrl_demod_process_sc8(qrl_demod* d, const int8_t* iq, size_t stride, size_t n, const qrl_demod_out* out)
{
    if (!d || (!iq && n)) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    (void)take_launch_error();
    return d->process(iq, stride, n, out, IN_SC8);
}
int qrl_demod_process_cu8(qrl_demod* d, const uint8_t* iq, size_t stride, size_t n, const qrl_demod_out* out)
{
    if (!d || (!iq && n)) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    (void)take_launch_error();
    return d->process(iq, stride, n, out, IN_CU8);
}
int qrl_demod_set_sc8_scale(qrl_demod* d, float scale)
{
    if (!d) return QRL_ERR_ARG;
    if (!sc16_scale_ok("qrl_demod_set_sc8_scale", scale)) return QRL_ERR_ARG;
    d->sc8_scale = scale;   // a kernel parameter of the calls from now on; calls already queued keep theirs
    return QRL_OK;
}
int qrl_demod_set_cu8_scale(qrl_demod* d, float scale, float bias)
{
    if (!d) return QRL_ERR_ARG;
    if (!sc16_scale_ok("qrl_demod_set_cu8_scale", scale) || !iq8_bias_ok("qrl_demod_set_cu8_scale", bias)) return QRL_ERR_ARG;
    d->cu8_scale = scale; d->cu8_bias = bias;
    return QRL_OK;
}
int qrl_demod_sync(qrl_demod* d)
{
    if (!d) return QRL_ERR_ARG;
    if (int rs = d->sync_all()) return rs;
    return QRL_OK;
}
void* qrl_demod_stream(qrl_demod* d) { return d ? d->stream : nullptr; }
int qrl_demod_internal_streams(qrl_demod* d, void* out[3])
{
    if (!d || !out) return QRL_ERR_ARG;
    out[0] = d->stream; out[1] = d->tail; out[2] = d->fecs;
    return QRL_OK;
}

int qrl_demod_profile(qrl_demod* d, int enable)
{
    if (!d) return QRL_ERR_ARG;
    d->profiling = enable != 0;
    return QRL_OK;
}
int qrl_demod_profile_read(qrl_demod* d, double* kernel_ms, uint64_t* launches, const char** kernel_name)
{
    if (!d) return QRL_ERR_ARG;
    if (int rs = d->sync_all()) return rs;
    double total = 0; uint64_t count = 0;
    QRLCHK(d->prof.read(total, count));
    if (kernel_ms) *kernel_ms = total;
    if (launches) *launches = count;
    if (kernel_name) {
        const DecimStage& st = d->fe.used ? d->fe : d->first;
        *kernel_name = (!d->fe.used && d->d2f) ? "k_dec2_fir"
                     : (d->fe.used || d->interp == 1) ? st.kernel_name() : "k_resamp";
    }
    return QRL_OK;
}

/* developer aid (not part of the drop-in surface): phase profile of k_decim_mfma under QRL_DBG=32 */
void qrl_debug_decim_prof(unsigned long long* out8) { decim_mfma_prof_read(out8); }
void qrl_debug_decim_prof_enable(int on) { decim_mfma_prof_enable(on); }

// one call from and to host memory through scratch buffers of its own: `esz` bytes per sample, device rows padded to a multiple of `round` samples
static int process_host(qrl_demod* d, const void* iq_host, size_t stride, size_t n, uint8_t* bits_a_host, uint8_t* bits_b_host, size_t bits_cap,
                        uint32_t* counts_host, size_t esz, size_t round, int fmt)
{
    if (!d || !iq_host || !counts_host) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    (void)take_launch_error();
    if (fmt == IN_SC16 && !d->fe.used && !d->sc16_baseband) return d->process(nullptr, 0, 0, nullptr, IN_SC16);   // the refusal of a 1 Msps handle, before anything is allocated
    if (fmt >= IN_SC8 && !d->fe.used && !d->iq8_baseband) return d->process(nullptr, 0, 0, nullptr, fmt);
    const size_t B = (size_t)d->cfg.batch;
    const size_t st = (n + round - 1) / round * round;
    DevBuf<unsigned char> iq; DevBuf<uint8_t> ba, bb; DevBuf<uint32_t> cnt;
    int r;
    if ((r = iq.alloc(B * st * esz)) || (r = ba.alloc(B * bits_cap)) || (r = bb.alloc(B * bits_cap)) || (r = cnt.alloc(B * 4))) return r;
    HIPCHK(hipMemcpy2D(iq.p, st * esz, iq_host, stride * esz, n * esz, B, hipMemcpyHostToDevice));
    qrl_demod_out o{};
    o.bits_a = ba.p; o.bits_b = bb.p; o.bits_cap = bits_cap; o.counts = cnt.p;
    if ((r = d->process(iq.p, st, n, &o, fmt))) return r;
    if (int rs = d->sync_all()) return rs;
    if (bits_a_host) HIPCHK(hipMemcpy(bits_a_host, ba.p, B * bits_cap, hipMemcpyDeviceToHost));
    if (bits_b_host) HIPCHK(hipMemcpy(bits_b_host, bb.p, B * bits_cap, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts_host, cnt.p, B * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return QRL_OK;
}
int qrl_demod_process_host(qrl_demod* d, const float* iq_host, size_t stride, size_t n, uint8_t* bits_a_host,
                           uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host)
{
    return process_host(d, iq_host, stride, n, bits_a_host, bits_b_host, bits_cap, counts_host, sizeof(float2), 2, IN_CF32);
}
int qrl_demod_process_sc16_host(qrl_demod* d, const int16_t* iq_host, size_t stride, size_t n, uint8_t* bits_a_host,
                                uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host)
{
    return process_host(d, iq_host, stride, n, bits_a_host, bits_b_host, bits_cap, counts_host, 4, 4, IN_SC16);
}
// 2 bytes per sample staged and uploaded; the device pitch is rounded up to 8 samples (whole 16-byte pieces)
int qrl_demod_process_sc8_host(qrl_demod* d, const int8_t* iq_host, size_t stride, size_t n, uint8_t* bits_a_host,
                               uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host)
{
    return process_host(d, iq_host, stride, n, bits_a_host, bits_b_host, bits_cap, counts_host, 2, 8, IN_SC8);
}
int qrl_demod_process_cu8_host(qrl_demod* d, const uint8_t* iq_host, size_t stride, size_t n, uint8_t* bits_a_host,
                               uint8_t* bits_b_host, size_t bits_cap, uint32_t* counts_host)
{
    return process_host(d, iq_host, stride, n, bits_a_host, bits_b_host, bits_cap, counts_host, 2, 8, IN_CU8);
}

// ---- host-only design helpers
static int copy_out(const std::vector<float>& v, float* dst) { if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(float)); return (int)v.size(); }
int qrl_firdes_low_pass(double g, double fs, double fc, double tw, int w, float* t)
{ return t ? copy_out(low_pass(g, fs, fc, tw, (Window)w), t) : compute_ntaps(fs, tw, (Window)w); }
int qrl_firdes_low_pass_2(double g, double fs, double fc, double tw, double a, int w, float* t)
{ return t ? copy_out(low_pass_2(g, fs, fc, tw, a, (Window)w), t) : compute_ntaps_windes(fs, tw, a); }
int qrl_firdes_complex_band_pass(double g, double fs, double lo, double hi, double tw, int w, float* t)
{
    if (!t) return compute_ntaps(fs, tw, (Window)w);
    const auto v = complex_band_pass(g, fs, lo, hi, tw, (Window)w);
    std::memcpy(t, v.data(), v.size() * sizeof(std::complex<float>));
    return (int)v.size();
}
int qrl_firdes_root_raised_cosine(double g, double fs, double sr, double a, int n, float* t)
{ return t ? copy_out(root_raised_cosine(g, fs, sr, a, n), t) : (n | 1); }
int qrl_table_mmse(float* t) { return copy_out(mmse_table(), t); }
int qrl_table_atan(float* t) { return copy_out(atan_table(), t); }
int qrl_table_tanh(float* t) { return copy_out(tanh_table(), t); }
uint64_t qrl_phase_inc_to_turn(double r) { return phase_inc_to_turn(r); }

}  // extern "C"
