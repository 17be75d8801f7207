// demod_dsss.cpp — the DSSS receiver (QRL_MODEM_BPSK8, gr_demod_dsss): everything behind the handle's 1:50 stage.
#include "demod.hpp"
#include <cmath>

int DsssChain::build(qrl_demod& d, size_t max2)
{
    int r;
    const int B = d.cfg.batch;
    const std::vector<float> ti = low_pass(1, d.target, 2600, 2600, WIN_BLACKMAN_HARRIS);       // _resampler_if (13, 50), gr_demod_dsss.cpp:57-59
    Jp = ((int)ti.size() + 12) / 13;
    const std::vector<float> tf = low_pass(1, 5200, d.cfg.filter_width, 1200, WIN_BLACKMAN_HARRIS);   // _filter, :62-63
    nf = (int)tf.size();
    if ((r = rs.upload(resamp_layout(ti, 13, Jp))) || (r = filt.upload(tf)) || (r = mf.upload(dsss_matched_filter(d.cfg.sps)))) return r;
    if (!d.tanh_tab.p && (r = d.tanh_tab.upload(tanh_table()))) return r;
    control_loop_gains((float)(M_PI / 200), a1, b1);                                          // _costas_freq, :64
    control_loop_gains((float)(2 * M_PI / 100), a2, b2);                                      // _costas_loop, :63
    const size_t max5 = max2 * 13 / 50 + 2;
    mask = pow2_at_least(max5 + 2048, 64) - 1;                                                   // the matched filter looks 2 x 325 + 600 items back
    sym_mask = pow2_at_least(max5 / 325 + 64, 64) - 1;
    const size_t r5 = (size_t)B * (mask + 1);
    if ((r = ra.alloc(r5)) || (r = rb.alloc(r5)) || (r = rc.alloc(r5)) || (r = rd.alloc(r5)) ||
        (r = sym.alloc((size_t)B * (sym_mask + 1))) || (r = st.alloc(B)) || (r = tail.alloc(B))) return r;
    return QRL_OK;
}

int DsssChain::init_state(qrl_demod& d)
{
    int r;
    for (auto* b : {&ra, &rb, &rc, &rd, &sym}) if ((r = b->zero())) return r;
    DsssState x; x.phase = 0.f; x.freq = 0.f; x.gain = 10.0f; x.pad = 0.f;   // agc2_cc(0.1, 0.1, 1, 10), gr_demod_dsss.cpp:61
    DsssTailState t; std::memset(&t, 0, sizeof t); t.mu = 0.5f; t.omega = 1.0f;   // clock_recovery_mm_cc(1, ., 0.5, ., .), :69-70
    if ((r = st.fill(d.cfg.batch, x)) || (r = tail.fill(d.cfg.batch, t))) return r;
    n5 = nsy = 0;
    return QRL_OK;
}

// everything of gr_demod_dsss behind the 1:50 stage (gr_demod_dsss.cpp:57-111); all on the handle's main stream
int DsssChain::stages(qrl_demod& d, uint64_t n2_0, uint64_t n2_1, const qrl_demod_out* out, uint32_t* counts)
{
    const int B = d.cfg.batch;
    const RingC r2{d.s2.p, d.s2_mask}, wa{ra.p, mask}, wb{rb.p, mask}, wc{rc.p, mask}, wd{rd.p, mask}, ws{sym.p, sym_mask};
    const uint64_t n5_0 = n5, n5_1 = decim_count(n2_1, 13, 50);
    const uint32_t c5 = (uint32_t)(n5_1 - n5_0);
    {   // _resampler_if: rational_resampler_ccf(13, 50)
        ResampParams p{};
        p.in = nullptr; p.in_ring = r2; p.n0 = n2_0; p.n = (uint32_t)(n2_1 - n2_0);
        p.out = wa; p.q0 = n5_0; p.q_count = c5;
        p.taps = rs.p; p.I = 13; p.D = 50; p.Jp = Jp;
        launch_resamp(p, B, d.stream);
    }
    {   // _costas_freq
        DsssLoopParams p{}; p.in = wa; p.out = wb; p.q0 = n5_0; p.count = c5; p.st = st.p; p.tanh_tab = d.tanh_tab.p; p.alpha = a1; p.beta = b1;
        launch_dsss_loop(p, 0, B, d.stream);
    }
    {   // _filter -> port 0
        FirCcfParams f{};
        f.in = wb; f.out = wc; f.q0 = n5_0; f.count = c5; f.taps = filt.p; f.nt = nf;
        const PortC fp = d.filtered_port(out);
        f.port = fp.p; f.port_cap = fp.cap; f.counts = counts;
        launch_fir_ccf(f, B, d.stream);
    }
    {   // _agc
        DsssLoopParams p{}; p.in = wc; p.out = wd; p.q0 = n5_0; p.count = c5; p.st = st.p; p.tanh_tab = d.tanh_tab.p;
        launch_dsss_loop(p, 1, B, d.stream);
    }
    // _dsss_decoder: output I needs x[325 (I - 1) + 599]
    const uint64_t nsy_1 = n5_1 >= 275 ? (n5_1 - 275) / 325 + 1 : 0;
    {
        DsssMfParams p{}; p.in = wd; p.out = ws; p.i0 = nsy; p.count = (uint32_t)(nsy_1 - nsy); p.taps = mf.p;
        launch_dsss_mf(p, B, d.stream);
    }
    {   // _clock_recovery -> _costas_loop (port 1) -> soft symbols
        DsssTailParams p{};
        p.in = ws; p.avail = nsy_1; p.soft = RingB{d.soft.p, d.soft_mask}; p.st = tail.p; p.mmse = d.mmse_tab.p;
        const float gain_omega = 0.005f;
        p.gain_omega = gain_omega * gain_omega; p.gain_mu = 0.05f; p.omega_mid = 1.0f; p.omega_lim = 0.005f * 1.0f;
        p.alpha = a2; p.beta = b2;
        const PortC cp = d.constellation_port(out);
        p.port = cp.p; p.port_cap = cp.cap; p.counts = counts;
        launch_dsss_tail(p, B, d.stream);
    }
    FecParams f{};
    f.soft = RingB{d.soft.p, d.soft_mask};
    f.avail = &tail.p[0].oo; f.avail_stride = sizeof(DsssTailState); f.avail_mul = 1;
    f.st = d.fec_st.p;
    f.bits_a = out ? out->bits_a : nullptr; f.bits_b = out ? out->bits_b : nullptr; f.bits_cap = out ? out->bits_cap : 0;
    f.counts = counts; f.branches = 2;
    launch_fec(f, B, d.stream);
    n5 = n5_1; nsy = nsy_1;
    return QRL_OK;
}
