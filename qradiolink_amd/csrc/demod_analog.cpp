// demod_analog.cpp — the analogue voice receivers: everything behind the handle's first resampler, and the qrl_demod_* entry points that exist for them alone.
#include "demod.hpp"
#include <cmath>

int AnalogChain::build(qrl_demod& d, size_t max2)
{
    int r;
    const int B = d.cfg.batch, fw = d.cfg.filter_width, target = d.target;
    std::vector<float> rt, ft;
    double a[2], b[2];
    if (kind == 0) {          // gr_demod_nbfm.cpp:43-64
        ramp = 320; I = 2; D = 5;
        rt = low_pass_2(2, 2 * target, 3600, 250, 60, WIN_BLACKMAN_HARRIS);
        ft = low_pass_2(1, 8000, 3500, 200, 35, WIN_BLACKMAN_HARRIS);
        gain = (float)(target / (4 * M_PI * fw));
        deemph_taps(target, 50e-6, a, b);
        de_ff[0] = b[0]; de_ff[1] = b[1]; de_fb1 = -a[1];            // iir_filter_ffd(btaps, ataps, oldstyle = false)
    } else if (kind == 1) {   // gr_demod_am.cpp:40-61
        ramp = 0; I = 2; D = 5;
        rt = low_pass(2, 2 * target, 3600, 600, WIN_BLACKMAN_HARRIS);
        ft = low_pass(1, 8000, 3600, 300, WIN_BLACKMAN_HARRIS);
        const auto fc = complex_band_pass_2(1, target, -fw, fw, 200, 90, WIN_BLACKMAN_HARRIS);
        nfc = (int)fc.size();
        if ((r = filt_c.upload(to_f2(fc)))) return r;
        ff[0] = 1; ff[1] = -1; fb1 = 0.9999;                          // iir_filter_ffd({1, -1}, {0, 0.9999}), old style
    } else if (kind == 3) {   // gr_demod_ssb.cpp:41-58
        ramp = 0; I = 0; D = 1;                                       // I = 0: the stretcher's chunked output count
        ft = band_pass_2(1, target, 200, fw, 200, 90, WIN_BLACKMAN_HARRIS);
        const auto fc = lsb ? complex_band_pass_2(1, target, -fw, -200, 200, 90, WIN_BLACKMAN_HARRIS)
                               : complex_band_pass_2(1, target, 200, fw, 200, 90, WIN_BLACKMAN_HARRIS);
        nfc = (int)fc.size();
        if ((r = filt_c.upload(to_f2(fc)))) return r;
    } else {                     // gr_demod_wbfm.cpp:41-57
        ramp = 0; I = 1; D = 25;
        rt = low_pass(1, target, 4000, 2000, WIN_BLACKMAN_HARRIS);
        gain = (float)(target / (2 * M_PI * fw));
        deemph_taps(8000, 50e-6, a, b);
        ff[0] = b[0]; ff[1] = b[1]; fb1 = -a[1];
    }
    nr = (int)rt.size(); nf = (int)ft.size();
    if ((nr && (r = rtaps.upload(rt))) || (nf && (r = ftaps.upload(ft))) || (r = env.upload(squelch_envelope(ramp)))) return r;
    m1 = pow2_at_least(max2 + 2048, 64) - 1;                              // the audio resampler looks <= 419 gated items back, the stretcher <= 1025
    m2 = kind == 3 ? m1 : pow2_at_least(max2 * I / D + 512, 64) - 1;
    if (kind == 3) { if ((r = c1.alloc((size_t)B * (m1 + 1)))) return r; }
    else if ((r = f1.alloc((size_t)B * (m1 + 1)))) return r;
    if ((r = f2.alloc((size_t)B * (m2 + 1))) || ((kind == 0 || kind == 1) && (r = f3.alloc((size_t)B * (m2 + 1)))) || (r = st.alloc(B))) return r;
    return QRL_OK;
}

int AnalogChain::init_state(qrl_demod& d)
{
    int r;
    for (auto* b : {&f1, &f2, &f3, &f4}) if (b->p && (r = b->zero())) return r;
    if (cs.p) {   // squelch_base: muted, envelope 0 (ramp 160); the Goertzel filters empty
        CtcssState x; std::memset(&x, 0, sizeof x); x.mute = 1; x.env = 0.0;
        if ((r = cs.fill(d.cfg.batch, x))) return r;
    }
    if (c1.p && (r = c1.zero())) return r;
    AnState x; std::memset(&x, 0, sizeof x); x.env = ramp ? 0.0f : 1.0f; x.gain = 1.0f;   // agc2_ff(0.1, 0.1, 1, 1), gr_demod_am.cpp:48
    return st.fill(d.cfg.batch, x);
}

// everything of gr_demod_nbfm / gr_demod_am / gr_demod_wbfm behind the first resampler; all on the handle's main stream
int AnalogChain::stages(qrl_demod& d, uint64_t n2_0, uint64_t n2_1, const qrl_demod_out* out, uint32_t* counts)
{
    const int B = d.cfg.batch;
    RingC r2{d.s2.p, d.s2_mask}, r2f{d.s2f.p, d.s2_mask};
    const uint32_t c2 = (uint32_t)(n2_1 - n2_0);
    const PortC fp = d.filtered_port(out);
    if (kind == 3) launch_scale_c(r2, n2_0, c2, if_gain, B, d.stream);   // _if_gain, gr_demod_ssb.cpp:45 (0.9 until gr_demod_ssb::set_gain)
    if (kind == 1 || kind == 3) {   // _filter -> port 0
        FirCccParams f{}; f.in = r2; f.out = r2f; f.q0 = n2_0; f.count = c2; f.taps = filt_c.p; f.nt = nfc;
        f.port = fp.p; f.port_cap = fp.cap; f.counts = counts;
        launch_an_fir_ccc(f, B, d.stream);
    } else {
        FirCcfParams f{}; f.in = r2; f.out = r2f; f.q0 = n2_0; f.count = c2; f.taps = d.filt_taps.p; f.nt = d.filt_nt;
        f.port = fp.p; f.port_cap = fp.cap; f.counts = counts;
        launch_fir_ccf(f, B, d.stream);
    }
    const RingF q1{f1.p, m1}, q2{f2.p, m2}, q3{f3.p, m2};
    {   // _squelch and the recursions directly behind it
        AnGateParams g{}; g.in = r2f; g.out = q1; g.q0 = n2_0; g.count = c2; g.st = st.p; g.atan_tab = d.atan_tab.p;
        g.env = env.p; g.ramp = ramp; g.alpha = 0.01; g.one_minus_alpha = 1.0 - 0.01; g.threshold = threshold;
        g.gain = gain; g.attack = attack; g.decay = decay; g.ff0 = ff[0]; g.ff1 = ff[1]; g.fb1 = fb1;
        g.outc = RingC{c1.p, m1}; g.ref = 0.25f; g.clip = 0.95f;             // agc2_cc(0.1, 0.1, 0.25, 1), clipper_cc(0.95): gr_demod_ssb.cpp:52,58
        launch_an_gate(g, kind, B, d.stream);
    }
    float* aport = out ? out->audio : nullptr;
    const size_t acap = out ? out->audio_cap : 0;
    if (kind == 3) {   // _stretcher, _complex_to_real, _level_control, _audio_filter -> port 1 (whole chunks of 1024 gated items)
        const uint32_t max_chunked = c2 + 1024;
        AnStretchParams sp{}; sp.in = RingC{c1.p, m1}; sp.out = q2; sp.st = st.p; sp.level = 1.333f;
        launch_an_stretch(sp, max_chunked, B, d.stream);
        AnFirParams p{}; p.in = q2; p.out = RingF{nullptr, 0}; p.st = st.p; p.taps = ftaps.p; p.nt = nf; p.I = 0; p.D = 1;
        p.port = aport; p.port_cap = acap; p.counts = counts;
        launch_an_fir(p, max_chunked, B, d.stream);
        return QRL_OK;
    }
    const uint32_t max_out = (uint32_t)((uint64_t)c2 * I / D + 2);
    {   // _audio_resampler (WBFM: -> port 1)
        AnResampParams p{}; p.in = q1; p.out = q2; p.st = st.p; p.taps = rtaps.p; p.nt = nr; p.I = I; p.D = D;
        if (kind == 2) { p.port = aport; p.port_cap = acap; p.counts = counts; }
        launch_an_resamp(p, max_out, B, d.stream);
    }
    const bool ctcss = kind == 0 && tone != 0.0f;
    if (ctcss) {   // _ctcss (gating): audio resampler -> ring f4, item count g2 (gr_demod_nbfm.cpp:110-119)
        CtcssParams p{}; p.in = q2; p.out = RingF{f4.p, m2}; p.st = st.p; p.cs = cs.p; p.I = I; p.D = D;
        for (int k = 0; k < 3; ++k) { p.wr[k] = wr[k]; p.wi[k] = wi[k]; }
        p.level = 0.01; p.len = 8000; p.ramp = 160; p.env = env_ct.p;
        launch_an_ctcss(p, B, d.stream);
    }
    if (kind != 2) {   // _audio_filter (AM: -> port 1)
        AnFirParams p{}; p.in = q2; p.out = q3; p.st = st.p; p.taps = ftaps.p; p.nt = nf; p.I = I; p.D = D;
        if (ctcss) { p.in = RingF{f4.p, m2}; p.taps = ftaps_ct.p; p.nt = nf_ct; p.cs = cs.p; }   // band_pass_2(1, 8000, 300, 3500, 200, 35, BH), :112-113
        if (kind == 1) { p.port = aport; p.port_cap = acap; p.counts = counts; }
        launch_an_fir(p, max_out, B, d.stream);
    }
    if (kind == 0) {   // _de_emph_filter, _level_control -> port 1
        AnDeemphParams p{}; p.in = q3; p.st = st.p; p.I = I; p.D = D; p.cs = ctcss ? cs.p : nullptr;
        p.ff0 = de_ff[0]; p.ff1 = de_ff[1]; p.fb1 = de_fb1; p.port = aport; p.port_cap = acap; p.counts = counts;
        launch_an_deemph(p, B, d.stream);
    }
    return QRL_OK;
}

// ---- C ABI (C linkage from the declarations in qrl_hip.h)
int qrl_demod_audio_cap(const qrl_demod* d, size_t n, size_t* audio_cap)
{
    if (!d || !audio_cap) return QRL_ERR_ARG;
    if (d->fam != qrl_demod::F_ANALOG) { *audio_cap = 0; return QRL_OK; }
    const size_t n2 = d->call_counts(n).n2;
    *audio_cap = d->an.kind == 3 ? n2 + 1024 + 4 : n2 * d->an.I / d->an.D + 4;
    return QRL_OK;
}
int qrl_demod_set_squelch(qrl_demod* d, double db)
{
    if (!d || d->fam != qrl_demod::F_ANALOG) return QRL_ERR_ARG;
    d->an.threshold = std::pow(10.0, db / 10);   // pwr_squelch_cc::set_threshold
    return QRL_OK;
}
int qrl_demod_set_ctcss(qrl_demod* d, float tone_hz)
{
    if (!d || d->fam != qrl_demod::F_ANALOG || d->an.kind != 0) return qrl_set_error(QRL_ERR_ARG, "qrl_demod_set_ctcss: NBFM receivers only (gr_demod_nbfm::set_ctcss)");
    if (tone_hz < 0.0f || tone_hz > 1000.0f) return QRL_ERR_ARG;
    HIPCHK(hipSetDevice(d->ctx->device));
    const bool was_on = d->an.tone != 0.0f, on = tone_hz != 0.0f;
    if (int rs = d->sync_all()) return rs;
    if (on && !d->an.cs.p) {   // first use: state, the gated ring, the band-pass audio filter, the envelope of ramp 160 (double: float item x double envelope)
        int r;
        const std::vector<float> ft = band_pass_2(1, 8000, 300, 3500, 200, 35, WIN_BLACKMAN_HARRIS);       // gr_demod_nbfm.cpp:112-113
        d->an.nf_ct = (int)ft.size();
        std::vector<double> env(161);
        for (int k = 0; k <= 160; ++k) env[k] = 0.5 - std::cos(M_PI * (double)k / 160.0) / 2.0;
        if ((r = d->an.ftaps_ct.upload(ft)) || (r = d->an.env_ct.upload(env)) || (r = d->an.cs.alloc(d->cfg.batch)) ||
            (r = d->an.f4.alloc((size_t)d->cfg.batch * (d->an.m2 + 1)))) return qrl_set_error(r, "ctcss buffers");
    }
    if (on) {   // ctcss_squelch_ff::set_frequency -> update_fft_params: the tone and its neighbours in the CTCSS table (2 % at the ends / off the table)
        static const float tones[38] = {67.0f, 71.9f, 74.4f, 77.0f, 79.7f, 82.5f, 85.4f, 88.5f, 91.5f, 94.8f, 97.4f, 100.0f, 103.5f, 107.2f, 110.9f, 114.8f,
                                        118.8f, 123.0f, 127.3f, 131.8f, 136.5f, 141.3f, 146.2f, 151.4f, 156.7f, 162.2f, 167.9f, 173.8f, 179.9f, 186.2f, 192.8f,
                                        203.5f, 210.7f, 218.1f, 225.7f, 233.6f, 241.8f, 250.3f};
        int i = -1;
        for (int k = 0; k < 38; ++k) if (tones[k] == tone_hz) i = k;
        const float f[3] = {(i == -1 || i == 0) ? (float)((double)tone_hz * 0.98) : tones[i - 1], tone_hz, (i == -1 || i == 37) ? (float)((double)tone_hz * 1.02) : tones[i + 1]};   // double literals, then narrowed (ctcss_squelch_ff_impl.cc compute_freqs)
        for (int k = 0; k < 3; ++k) {
            const float w = (float)(2.0 * M_PI * f[k] / 8000);
            d->an.wr[k] = (float)(2.0 * (double)cosf(w));
            d->an.wi[k] = sinf(w);
        }
    }
    d->an.tone = tone_hz;
    // switching the block in or out re-wires the audio path (the reference disconnects / connects under lock()): the chain restarts
    // from a fresh state, like qrl_demod_reset; a new tone while it is on re-initialises the Goertzel filters only (set_frequency)
    if (was_on != on) return d->init_state();
    if (on) {
        std::vector<CtcssState> cs(d->cfg.batch);
        if (hipMemcpy(cs.data(), d->an.cs.p, cs.size() * sizeof(CtcssState), hipMemcpyDeviceToHost) != hipSuccess) return QRL_ERR_HIP;
        for (auto& x : cs) { for (int k = 0; k < 3; ++k) x.d1[k] = x.d2[k] = 0.0f; x.processed = 0; }
        if (hipMemcpy(d->an.cs.p, cs.data(), cs.size() * sizeof(CtcssState), hipMemcpyHostToDevice) != hipSuccess) return QRL_ERR_HIP;
    }
    return QRL_OK;
}
int qrl_demod_set_filter_width(qrl_demod* d, int width)
{
    if (!d || d->fam != qrl_demod::F_ANALOG)
        return qrl_set_error(QRL_ERR_ARG, "qrl_demod_set_filter_width: analogue receivers only (gr_demod_base::set_filter_width forwards to WBFM, AM, NBFM, USB, LSB)");
    // firdes' sanity checks: 0 < cutoff <= fs / 2; the SSB band starts at 200 Hz
    if (width <= 0 || 2 * width > d->target || (d->an.kind == 3 && width <= 200)) return qrl_set_error(QRL_ERR_ARG, "qrl_demod_set_filter_width: width out of range");
    HIPCHK(hipSetDevice(d->ctx->device));
    if (int rs = d->sync_all()) return rs;
    const double fs = d->target, w = width;
    int r = QRL_OK;
    // the setters do not repeat the constructors' designs (transition widths, design functions, the SSB audio filter's gain of 2)
    if (d->an.kind == 0 || d->an.kind == 2) {   // gr_demod_nbfm.cpp:82-90, gr_demod_wbfm.cpp:76-84
        const std::vector<float> f = low_pass(1, fs, w, 1200, WIN_BLACKMAN_HARRIS);
        d->filt_nt = (int)f.size();
        r = d->filt_taps.upload(f);
        d->an.gain = (float)(d->target / ((d->an.kind == 0 ? 4 : 2) * M_PI * width));
    } else if (d->an.kind == 1) {               // gr_demod_am.cpp:84-91
        const auto fc = complex_band_pass(1, fs, -w, w, 1200, WIN_BLACKMAN_HARRIS);
        d->an.nfc = (int)fc.size();
        r = d->an.filt_c.upload(to_f2(fc));
    } else {                                    // gr_demod_ssb.cpp:89-101
        const auto fc = d->an.lsb ? complex_band_pass_2(1, fs, -w, -200, 200, 90, WIN_BLACKMAN_HARRIS) : complex_band_pass_2(1, fs, 200, w, 200, 90, WIN_BLACKMAN_HARRIS);
        const std::vector<float> ft = band_pass_2(2, fs, 200, w, 200, 90, WIN_BLACKMAN_HARRIS);
        d->an.nfc = (int)fc.size(); d->an.nf = (int)ft.size();
        if (!(r = d->an.filt_c.upload(to_f2(fc)))) r = d->an.ftaps.upload(ft);
    }
    if (r) return qrl_set_error(r, "qrl_demod_set_filter_width: filter tables");
    d->cfg.filter_width = width;
    // The reference swaps the taps of a running graph under lock() / unlock(), at a sample position its scheduler decides; here the chain restarts
    // from a fresh state (like qrl_demod_reset; squelch, CTCSS and AGC settings are kept) -- what the tests compare is the chain built with the setter's designs.
    return d->init_state();
}
int qrl_demod_set_gain(qrl_demod* d, float value)
{
    if (!d || d->fam != qrl_demod::F_ANALOG || d->an.kind != 3) return qrl_set_error(QRL_ERR_ARG, "qrl_demod_set_gain: SSB receivers only (gr_demod_base::set_gain)");
    d->an.if_gain = value;   // multiply_const_cc::set_k: from the next call on, nothing restarts
    return QRL_OK;
}
int qrl_demod_set_agc(qrl_demod* d, float attack, float decay)
{
    if (!d || d->fam != qrl_demod::F_ANALOG || (d->an.kind != 1 && d->an.kind != 3)) return QRL_ERR_ARG;
    d->an.attack = attack; d->an.decay = decay;
    return QRL_OK;
}
