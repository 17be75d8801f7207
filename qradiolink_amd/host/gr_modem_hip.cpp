// gr_modem_hip.cpp — see gr_modem_hip.h.  Every function cites the reference lines it restates.
#include "gr_modem_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace qrl_host {

namespace {
enum {   // gr_modem_types (src/modem_types.h:5-50); the modes without a QRL_MODEM_* constant
    ModemTypeBPSK8 = 25, ModemTypeM17 = 40
};
bool is_1k(int m)   // the modes with the 8-bit FrameTypeVoice1 sync and no reserved byte (gr_modem.cpp:1143-1149, 1213-1217)
{
    return m == QRL_MODEM_BPSK1K || m == QRL_MODEM_2FSK1KFM || m == QRL_MODEM_2FSK1K || m == QRL_MODEM_GMSK1K || m == QRL_MODEM_4FSK1KFM;
}
}  // namespace

int modem_rx_frame_length(int m, int* bit_buf_len)   // gr_modem.cpp:203-322
{
    int len = 0, bits = 0;
    switch (m) {
    case QRL_MODEM_BPSK2K: case ModemTypeBPSK8: case QRL_MODEM_QPSK2K: case QRL_MODEM_4FSK2K: case QRL_MODEM_4FSK2KFM:
    case QRL_MODEM_2FSK2KFM: case QRL_MODEM_2FSK2K: case QRL_MODEM_GMSK2K: bits = 8 * 8; len = 7; break;
    case QRL_MODEM_BPSK1K: case QRL_MODEM_2FSK1KFM: case QRL_MODEM_2FSK1K: case QRL_MODEM_4FSK1KFM: case QRL_MODEM_GMSK1K: bits = 4 * 8; len = 4; break;
    case QRL_MODEM_QPSK20K: case QRL_MODEM_4FSK10KFM: case QRL_MODEM_2FSK10KFM: case QRL_MODEM_GMSK10K: bits = 48 * 8; len = 47; break;
    case QRL_MODEM_QPSKVIDEO: bits = 3123 * 8; len = 3122; break;
    case QRL_MODEM_QPSK250K: bits = 1517 * 8; len = 1516; break;
    case QRL_MODEM_4FSK100K: bits = 623 * 8; len = 622; break;
    case ModemTypeM17: bits = 46 * 8; len = 46; break;
    case QRL_MODEM_DMR: bits = 46 * 8; len = 9; break;
    default: break;
    }
    if (bit_buf_len) *bit_buf_len = bits;
    return len;
}
int modem_tx_frame_length(int m)   // gr_modem.cpp:105-199
{
    if (m == ModemTypeM17) return 16;
    return modem_rx_frame_length(m, nullptr);
}
bool modem_two_branches(int m)   // gr_modem.cpp:1048-1058
{
    switch (m) {
    case QRL_MODEM_BPSK2K: case QRL_MODEM_2FSK2KFM: case QRL_MODEM_2FSK2K: case QRL_MODEM_2FSK10KFM: case QRL_MODEM_GMSK2K: case QRL_MODEM_GMSK1K:
    case QRL_MODEM_GMSK10K: case QRL_MODEM_BPSK1K: case ModemTypeBPSK8: case QRL_MODEM_2FSK1KFM: case QRL_MODEM_2FSK1K: return true;
    default: return false;
    }
}

// ================================================================================================ gr_demod_base_hip
struct gr_demod_base_hip::slot {
    pinned_buf<gr_complex> h_iq;                          // [streams][chunk]
    dev_buf<float> d_iq;                                  // [streams][chunk] cf32 (an int16 call uses the first half of every buffer: 4-byte samples at the same pitch)
    dev_buf<float> d_filt;                                // port 0, cf32
    mirror<gr_complex> konst; bool const_copied = true;   // port 1
    mirror<uint8_t> a, b, dmo; mirror<uint32_t> cnt, dmocnt;   // dmo / dmocnt: the pinned side takes the DMO slicer's bursts or the repeater sink's
    mirror<float> rssi; bool rssi_valid = false;          // latest rssi_block value per stream
    mirror<float> audio;                                  // analogue modes: port 1
    mirror<gr_complex> scope; mirror<uint32_t> scnt; bool scoped = false;   // time-domain scope items of the call
    mirror<uint8_t> fr[2]; mirror<uint32_t> frcnt[2];     // framed records of bits A / B; counts [2 N]: bytes, frames; [N]: bits collected under a sync
    bool framed = false, bits_copied = true;
    mirror<uint8_t> rec_l2; bool l2 = false;              // DMR layer 2 records of the call's bursts (set_dmr_l2)
    mirror<uint8_t> rec_m17; bool m17 = false;            // M17 link records of the frames of bits A (set_m17_link)
    mirror<uint8_t> rec_call; bool call = false;          // DMR call records of the same bursts (set_dmr_call)
    dev_buf<uint8_t> d_rep; mirror<uint8_t> rec_info; dev_buf<uint32_t> d_repcnt; bool rep = false;   // the repeater-mode sink's bursts, their slot records (set_dmr_repeater)
    hip_event done;
};
static constexpr size_t kDmoCap = 16;
using records = std::vector<std::vector<unsigned char>>;
// record i of stream s, `bytes` long, of a pinned array of kDmoCap records per stream: appended to the stream's mailbox
static void append_record(records& box, const uint8_t* h, size_t s, size_t i, size_t bytes)
{
    const uint8_t* r = h + (s * kDmoCap + i) * bytes;
    box.emplace_back(r, r + bytes);
}
static records take_box(std::mutex& m, records& box)
{
    std::lock_guard<std::mutex> g(m);
    records out;
    out.swap(box);
    return out;
}

gr_demod_base_hip::gr_demod_base_hip(qrl_runtime& rt, int streams, int device_samp_rate, double carrier_offset_hz, size_t max_chunk)
    : d_rt(rt), d_n(streams), d_rate(device_samp_rate), d_offset(carrier_offset_hz), d_chunk(max_chunk & ~(size_t)1),
      d_offsets((size_t)std::max(streams, 0), carrier_offset_hz), d_boxa(streams), d_box1(streams), d_box2(streams), d_boxc(streams), d_boxd(streams), d_boxl(streams), d_boxe(streams), d_boxi(streams)
{
    d_boxf[0].resize(streams); d_boxf[1].resize(streams); d_boxs.resize(streams);
    for (int k = 0; k < 2; ++k) { d_fbits[k].assign(streams, 0); d_fact[k].assign(streams, 0); }
    if (streams < 1 || d_chunk < 2) throw std::invalid_argument("gr_demod_base_hip: streams >= 1, max_chunk >= 2");
}
gr_demod_base_hip::~gr_demod_base_hip()
{
    try { flush(); } catch (...) {}
    close();   // then the members, in reverse order of declaration (gr_modem_hip.h)
}
void gr_demod_base_hip::close()
{
    d_h.reset(); d_rssi.reset(); d_fft.reset(); d_fftout.reset();
    for (auto& f : d_fs) f.reset();
    for (auto& sp : d_slot) sp.reset();
    d_inflight = -1;
}
void gr_demod_base_hip::open()   // a failed open leaves the facade closed
try {
    close();
    qrl_demod_config c{};
    c.modem_type = d_mode; c.use_mode_defaults = 1; c.device_samp_rate = d_rate; c.carrier_offset_hz = d_offset;
    c.batch = d_n; c.max_chunk = d_chunk; c.enable_side_outputs = 1;
    c.time_domain_samp_rate = d_scope_rate; c.time_domain_filter_width = d_scope_fw;
    qrl_demod* h = nullptr;
    chk(qrl_demod_create(d_rt.ctx(), &c, &h), "qrl_demod_create");
    d_h.reset(h);
    chk(qrl_demod_set_sc16_scale(h, d_sc16_scale), "qrl_demod_set_sc16_scale");
    chk(qrl_demod_set_sc8_scale(h, d_sc8_scale), "qrl_demod_set_sc8_scale");
    chk(qrl_demod_set_cu8_scale(h, d_cu8_scale, d_cu8_bias), "qrl_demod_set_cu8_scale");
    chk(qrl_demod_set_option(h, QRL_OPT_SC16_BASEBAND, d_sc16_baseband ? 1 : 0), "qrl_demod_set_option");
    chk(qrl_demod_set_option(h, QRL_OPT_IQ8_BASEBAND, d_iq8_baseband ? 1 : 0), "qrl_demod_set_option");
    if (d_per_stream) chk(qrl_demod_set_carrier_offsets(h, d_offsets.data()), "qrl_demod_set_carrier_offsets");   // the new handle's phases start at 0
    chk(qrl_demod_out_caps(h, d_chunk, &d_fcap, &d_ccap, &d_bcap), "qrl_demod_out_caps");
    chk(qrl_demod_audio_cap(h, d_chunk, &d_acap), "qrl_demod_audio_cap");
    if (d_acap) chk(qrl_demod_set_squelch(h, (double)d_squelch), "qrl_demod_set_squelch");
    if (d_acap && has_agc()) chk(qrl_demod_set_agc(h, d_agc_attack, d_agc_decay), "qrl_demod_set_agc");   // the reference's _am, _usb and _lsb instances all keep the rates
    if (d_acap && d_ctcss != 0.0f && (d_mode == QRL_MODEM_NBFM2500 || d_mode == QRL_MODEM_NBFM5000)) chk(qrl_demod_set_ctcss(h, d_ctcss), "qrl_demod_set_ctcss");   // the reference's instances keep their tone across mode changes
    if (d_acap && d_width.count(d_mode)) chk(qrl_demod_set_filter_width(h, d_width[d_mode]), "qrl_demod_set_filter_width");   // ... and their set_filter_width designs
    if (d_acap && d_if_gain >= 0.0f && (d_mode == QRL_MODEM_USB2500 || d_mode == QRL_MODEM_LSB2500)) chk(qrl_demod_set_gain(h, d_if_gain), "qrl_demod_set_gain");
    const size_t N = (size_t)d_n;
    // side outputs on the copy stream: rssi_block behind port 0, rx_fft_c on the device-rate IQ (gr_demod_base.cpp:166,185,199-200)
    qrl_rssi* rssi = nullptr; qrl_fft* fft = nullptr;
    chk(qrl_rssi_create(d_rt.ctx(), d_n, d_rssi_cal, d_copy.get(), &rssi), "qrl_rssi_create");
    d_rssi.reset(rssi);
    chk(qrl_fft_create(d_rt.ctx(), d_n, d_fftsize, 5 /* WIN_BLACKMAN_HARRIS */, d_copy.get(), &fft), "qrl_fft_create");
    d_fft.reset(fft);
    chk(qrl_fft_set_enabled(fft, d_fft_on ? 1 : 0), "qrl_fft_set_enabled");
    chk(qrl_fft_set_sc16_scale(fft, d_sc16_scale), "qrl_fft_set_sc16_scale");
    chk(qrl_fft_set_sc8_scale(fft, d_sc8_scale), "qrl_fft_set_sc8_scale");
    chk(qrl_fft_set_cu8_scale(fft, d_cu8_scale, d_cu8_bias), "qrl_fft_set_cu8_scale");
    d_level.assign(N, 0.0f);
    // L1 frame synchronisers on the copy stream, behind the demodulator (digital modes with gr_modem framing: not DMR, not analogue)
    const bool fs_on = d_want_fs && !d_acap && d_mode != QRL_MODEM_DMR;
    if (fs_on) {
        for (auto& f : d_fs) {
            qrl_framesync* fs = nullptr;
            chk(qrl_framesync_create(d_rt.ctx(), d_mode, d_n, d_copy.get(), &fs), "qrl_framesync_create");
            f.reset(fs);
        }
        const size_t fb = (size_t)qrl_framesync_frame_bytes(d_fs[0].get());
        d_frcap = (d_bcap / 8 + fb + 96 + 16 * (d_bcap / std::max<size_t>(8 * fb, 8) + 2) + 3) & ~(size_t)3;   // never overflows (include/qrl_hip.h)
    }
    chk(qrl_demod_time_domain_cap(h, d_chunk, &d_scap), "qrl_demod_time_domain_cap");
    for (auto& sp : d_slot) {
        sp = std::make_unique<slot>();
        sp->scope.alloc(N * d_scap);
        sp->scnt.alloc(N);
        if (fs_on) for (int k = 0; k < 2; ++k) {
            sp->fr[k].alloc(N * d_frcap);
            sp->frcnt[k].alloc(N * 3);
        }
        if (fs_on && d_mode == QRL_MODEM_M17) sp->rec_m17.alloc(N * (d_frcap / QRL_M17_FRAMESYNC_RECORD_BYTES) * QRL_M17_RX_RECORD_BYTES);   // one link record per frame the row can hold
        sp->rssi.alloc(N);
        sp->h_iq.alloc(N * d_chunk);
        sp->d_iq.alloc(2 * N * d_chunk);
        sp->d_filt.alloc(2 * N * d_fcap);
        sp->konst.alloc(N * d_ccap);
        sp->a.alloc(N * d_bcap);
        sp->b.alloc(N * d_bcap);
        sp->cnt.alloc(N * 4);
        if (d_acap) sp->audio.alloc(N * d_acap);
        if (d_mode == QRL_MODEM_DMR) {
            sp->dmo.alloc(N * kDmoCap * QRL_DMO_RECORD_BYTES);
            sp->dmocnt.alloc(N);
            sp->rec_l2.alloc(N * kDmoCap * QRL_DMR_L2_RECORD_BYTES);
            sp->rec_call.alloc(N * kDmoCap * QRL_DMR_RX_RECORD_BYTES);
            sp->d_rep.alloc(N * kDmoCap * QRL_DMR_SINK_FRAME_BYTES);
            sp->rec_info.alloc(N * kDmoCap * QRL_DMR_SINK_INFO_BYTES);
            sp->d_repcnt.alloc(N);
        }
    }
    d_calls = 0;
    if (d_call_rx) chk(qrl_dmr_rx_reset(d_call_rx.get(), d_copy.get()), "qrl_dmr_rx_reset");   // the receiver starts afresh, and so does the call state behind it
    if (d_sink) chk(qrl_dmr_sink_reset(d_sink.get()), "qrl_dmr_sink_reset");
    if (d_m17_rx) chk(qrl_m17_rx_reset(d_m17_rx.get(), d_copy.get()), "qrl_m17_rx_reset");
} catch (...) {
    close();
    throw;
}
void gr_demod_base_hip::apply_call_mode()
{
    if (d_call_rx.get()) chk(qrl_dmr_rx_set_mode(d_call_rx.get(), d_rep_on ? QRL_DMR_MODE_REPEATER : QRL_DMR_MODE_DMO, d_rep_slot), "qrl_dmr_rx_set_mode");
}
void gr_demod_base_hip::set_dmr_repeater(bool on, int timeslot)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (on && (timeslot < 1 || timeslot > 2)) throw std::runtime_error("gr_demod_base_hip::set_dmr_repeater: timeslot outside 1..2");
    if (on) {
        if (!d_sink) { qrl_dmr_sink* h = nullptr; chk(qrl_dmr_sink_create(d_rt.ctx(), d_n, d_copy.get(), &h), "qrl_dmr_sink_create"); d_sink.reset(h); }
        else if (!d_rep_on) chk(qrl_dmr_sink_reset(d_sink.get()), "qrl_dmr_sink_reset");   // switched back on: nothing of the bits it missed
        d_rep_slot = timeslot;
    }
    if (on != d_rep_on && d_call_rx) chk(qrl_dmr_rx_reset(d_call_rx.get(), d_copy.get()), "qrl_dmr_rx_reset");   // another sink's bursts: no call goes on across the switch
    d_rep_on = on;
    apply_call_mode();
}
void gr_demod_base_hip::set_dmr_call(bool on, int colour_code, bool promiscuous)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    const qrl_dmr_rx_config c = {colour_code, promiscuous ? 1 : 0};
    if (!d_call_rx) {
        if (!on) return;
        qrl_dmr_rx* h = nullptr;
        chk(qrl_dmr_rx_create(d_rt.ctx(), (size_t)d_n, &c, &h), "qrl_dmr_rx_create");
        d_call_rx.reset(h);
        apply_call_mode();
    } else {
        chk(qrl_dmr_rx_set_config(d_call_rx.get(), &c), "qrl_dmr_rx_set_config");
        if (on && !d_call_on) chk(qrl_dmr_rx_reset(d_call_rx.get(), d_copy.get()), "qrl_dmr_rx_reset");   // switched back on: nothing of the calls it missed
    }
    d_call_on = on;
}
void gr_demod_base_hip::set_m17_link(bool on, int can_rx, bool decode_all_can)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    const qrl_m17_rx_config c = {can_rx, decode_all_can ? 1 : 0};
    if (!d_m17_rx) {
        if (!on) return;
        qrl_m17_rx* h = nullptr;
        chk(qrl_m17_rx_create(d_rt.ctx(), (size_t)d_n, &c, &h), "qrl_m17_rx_create");
        d_m17_rx.reset(h);
    } else {
        chk(qrl_m17_rx_set_config(d_m17_rx.get(), &c), "qrl_m17_rx_set_config");
        if (on && !d_m17_on) chk(qrl_m17_rx_reset(d_m17_rx.get(), d_copy.get()), "qrl_m17_rx_reset");   // switched back on: nothing of the frames it missed
    }
    d_m17_on = on;
}
void gr_demod_base_hip::set_mode(int mode)   // gr_demod_base::set_mode (src/gr/gr_demod_base.cpp:460-1090): swap the graph, drop what was queued
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    flush();
    d_mode = mode;
    try { open(); }
    catch (const std::exception& e) {
        if (d_scope_rate == 0 && d_scope_fw == 0.0) throw;
        d_scope_rate = 0; d_scope_fw = 0.0;   // set before a handle existed and only rejected now: back to the constructor's 1:10 tap
        open();
        throw std::invalid_argument(std::string("gr_demod_base_hip::set_mode: time-domain settings rejected and reset to the defaults (the mode is open): ") + e.what());
    }
    std::lock_guard<std::mutex> g(d_mutex);
    for (int s = 0; s < d_n; ++s) { d_box1[s].clear(); d_box2[s].clear(); d_boxc[s].clear(); d_boxd[s].clear(); d_boxl[s].clear(); d_boxe[s].clear(); d_boxi[s].clear(); d_boxa[s].clear(); d_boxf[0][s].clear(); d_boxf[1][s].clear(); d_boxs[s].clear(); d_fbits[0][s] = d_fbits[1][s] = d_fact[0][s] = d_fact[1][s] = 0; }
}
void gr_demod_base_hip::enable_device_framing(bool value)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_want_fs = value;
}
bool gr_demod_base_hip::takeFrames(int nr, int stream, std::vector<frame_record>& frames, size_t& bits, size_t& collected)
{
    std::lock_guard<std::mutex> g(d_mutex);
    const int k = nr == 2 ? 1 : 0;
    bits = d_fbits[k][stream]; collected = d_fact[k][stream];
    if (bits < 32) return false;   // gr_bit_sink::get_data (src/gr/gr_bit_sink.cpp:45-59): nothing below 32 bits, and nothing is consumed
    frames.clear();
    frames.swap(d_boxf[k][stream]);
    d_fbits[k][stream] = 0; d_fact[k][stream] = 0;
    return true;
}
size_t gr_demod_base_hip::peekFrameBits(int nr, int stream)
{
    std::lock_guard<std::mutex> g(d_mutex);
    return d_fbits[nr == 2 ? 1 : 0][stream];
}
std::vector<gr_demod_base_hip::frame_record> gr_demod_base_hip::getFrames(int nr, int stream)
{
    std::lock_guard<std::mutex> g(d_mutex);
    std::vector<frame_record> out;
    out.swap(d_boxf[nr == 2 ? 1 : 0][stream]);
    return out;
}
void gr_demod_base_hip::set_carrier_offset(double hz)   // gr_demod_base.cpp:1220-1225
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_offset = hz;
    d_offsets.assign((size_t)d_n, hz);
    if (d_h.get()) chk(qrl_demod_set_carrier_offset(d_h.get(), hz), "qrl_demod_set_carrier_offset");
}
void gr_demod_base_hip::set_carrier_offset(double hz, int stream)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (stream < 0 || stream >= d_n) throw std::out_of_range("gr_demod_base_hip::set_carrier_offset: stream out of range");
    std::vector<double> v = d_offsets;
    v[(size_t)stream] = hz;
    if (d_h.get()) chk(qrl_demod_set_carrier_offsets(d_h.get(), v.data()), "qrl_demod_set_carrier_offsets");
    d_offsets.swap(v);
    d_per_stream = true;
}
void gr_demod_base_hip::set_samp_rate(int device_samp_rate)   // gr_demod_base.cpp:1303-1362: the resampler is rebuilt
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    flush();
    d_rate = device_samp_rate;
    if (d_mode >= 0) open();
}
void gr_demod_base_hip::work(const gr_complex* const* iq, size_t n) { work_any(reinterpret_cast<const void* const*>(iq), n, FMT_CF32); }
// 16-bit integer I/Q as the SDR drivers deliver it (interleaved int16 I, Q): 4 bytes per sample are staged in the pinned buffer and uploaded,
// and the device-rate front end -- at 1 Msps, under set_sc16_baseband, the mode's first stage -- converts (qrl_demod_process_sc16:
// x = (float)v * scale).  Replaces the driver's sc16 -> fc32 conversion.
void gr_demod_base_hip::work(const int16_t* const* iq, size_t n) { work_any(reinterpret_cast<const void* const*>(iq), n, FMT_SC16); }
// 8-bit I/Q as an RTL-SDR (unsigned) or a HackRF (signed) delivers it: 2 bytes per sample staged and uploaded, the front end converts
// (qrl_demod_process_sc8 / _cu8) -- at 1 Msps, under set_iq8_baseband, the mode's first stage does.
void gr_demod_base_hip::work(const int8_t* const* iq, size_t n) { work_any(reinterpret_cast<const void* const*>(iq), n, FMT_SC8); }
void gr_demod_base_hip::work(const uint8_t* const* iq, size_t n) { work_any(reinterpret_cast<const void* const*>(iq), n, FMT_CU8); }
void gr_demod_base_hip::set_sc8_scale(float scale)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!std::isfinite(scale) || scale == 0.0f) throw std::invalid_argument("gr_demod_base_hip::set_sc8_scale: finite, non-zero");
    d_sc8_scale = scale;
    if (d_h.get()) chk(qrl_demod_set_sc8_scale(d_h.get(), scale), "qrl_demod_set_sc8_scale");
    if (d_fft.get()) chk(qrl_fft_set_sc8_scale(d_fft.get(), scale), "qrl_fft_set_sc8_scale");   // the spectrum tap reads the same 8-bit slot
}
void gr_demod_base_hip::set_cu8_scale(float scale, float bias)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!std::isfinite(scale) || scale == 0.0f || !std::isfinite(bias)) throw std::invalid_argument("gr_demod_base_hip::set_cu8_scale: scale finite and non-zero, bias finite");
    d_cu8_scale = scale; d_cu8_bias = bias;
    if (d_h.get()) chk(qrl_demod_set_cu8_scale(d_h.get(), scale, bias), "qrl_demod_set_cu8_scale");
    if (d_fft.get()) chk(qrl_fft_set_cu8_scale(d_fft.get(), scale, bias), "qrl_fft_set_cu8_scale");
}
void gr_demod_base_hip::set_sc16_scale(float scale)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!std::isfinite(scale) || scale == 0.0f) throw std::invalid_argument("gr_demod_base_hip::set_sc16_scale: finite, non-zero");
    d_sc16_scale = scale;
    if (d_h.get()) chk(qrl_demod_set_sc16_scale(d_h.get(), scale), "qrl_demod_set_sc16_scale");
    if (d_fft.get()) chk(qrl_fft_set_sc16_scale(d_fft.get(), scale), "qrl_fft_set_sc16_scale");   // the spectrum tap reads the same int16 slot
}
void gr_demod_base_hip::set_sc16_baseband(bool on)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_sc16_baseband = on;
    if (d_h.get()) chk(qrl_demod_set_option(d_h.get(), QRL_OPT_SC16_BASEBAND, on ? 1 : 0), "qrl_demod_set_option");
}
void gr_demod_base_hip::set_iq8_baseband(bool on)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_iq8_baseband = on;
    if (d_h.get()) chk(qrl_demod_set_option(d_h.get(), QRL_OPT_IQ8_BASEBAND, on ? 1 : 0), "qrl_demod_set_option");
}
void gr_demod_base_hip::work_any(const void* const* iq, size_t n, int fmt)
{
    const bool sc16 = fmt == FMT_SC16, iq8 = fmt == FMT_SC8 || fmt == FMT_CU8;
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!d_h) throw std::runtime_error("gr_demod_base_hip::work before set_mode");
    if (n == 0) return;
    if (n > d_chunk || (n & 1)) throw std::invalid_argument("gr_demod_base_hip::work: n must be even and <= max_chunk");
    if (sc16) {
        // the C ABI would refuse the same (QRL_ERR_ARG); checked here before anything is staged or queued
        if (d_rate < 2000000 && !d_sc16_baseband) throw std::invalid_argument("gr_demod_base_hip::work(int16): needs the device-rate front end (device_samp_rate >= 2000000)");
        if (d_chunk & 3) throw std::invalid_argument("gr_demod_base_hip::work(int16): max_chunk (the row pitch) must be a multiple of 4 samples");
    }
    if (iq8) {   // as for int16: what the C ABI would refuse, before anything is staged or queued
        if (d_rate < 2000000 && !d_iq8_baseband) throw std::invalid_argument("gr_demod_base_hip::work(8-bit): needs the device-rate front end (device_samp_rate >= 2000000)");
        if (d_chunk & 7) throw std::invalid_argument("gr_demod_base_hip::work(8-bit): max_chunk (the row pitch) must be a multiple of 8 samples");
    }
    if (!d_demod_on && !d_fft_on) return;                        // _demod_valve closed and nobody else listens: the samples are dropped
    const int cur = (int)(d_calls & 1);
    slot& sl = *d_slot[cur];
    const size_t sb = iq8 ? 2 : sc16 ? 2 * sizeof(int16_t) : sizeof(gr_complex);   // bytes per sample; the pitch stays d_chunk samples
    // the spectrum tap on the uploaded slot, in the slot's format
    auto fft_tap = [&]() {
        if (fmt == FMT_SC8) chk(qrl_fft_process_sc8(d_fft.get(), reinterpret_cast<const int8_t*>(sl.d_iq.get()), d_chunk, n), "qrl_fft_process_sc8");
        else if (fmt == FMT_CU8) chk(qrl_fft_process_cu8(d_fft.get(), reinterpret_cast<const uint8_t*>(sl.d_iq.get()), d_chunk, n), "qrl_fft_process_cu8");
        else if (sc16) chk(qrl_fft_process_sc16(d_fft.get(), reinterpret_cast<const int16_t*>(sl.d_iq.get()), d_chunk, n), "qrl_fft_process_sc16");
        else chk(qrl_fft_process(d_fft.get(), sl.d_iq.get(), d_chunk, n), "qrl_fft_process");
    };
    // slot `cur` was last used by call k - 2, which work(k - 1) has harvested: its buffers are free
    for (int s = 0; s < d_n; ++s) std::memcpy(reinterpret_cast<char*>(sl.h_iq.get()) + (size_t)s * d_chunk * sb, iq[s], n * sb);
    hipStream_t hs = static_cast<hipStream_t>(qrl_demod_stream(d_h.get())), cs = d_copy.get();
    if (!d_demod_on) {                                           // _demod_valve closed (gr_demod_base.cpp:1150-1153): only the spectrum tap, which sits in front of it
        // everything of this call on the spectrum block's own stream (d_copy): the upload, the FFT fill behind it, and the host waits for THAT
        // stream before the slot is reused (the upload used to go on the demodulator's stream, which nothing ordered the FFT behind)
        hchk(hipMemcpyAsync(sl.d_iq.get(), sl.h_iq.get(), (size_t)d_n * d_chunk * sb, hipMemcpyHostToDevice, cs), "H2D");
        fft_tap();
        hchk(hipStreamSynchronize(cs), "hipStreamSynchronize");  // (d_calls does not advance: the next call takes the same slot; no harvest belongs to this call)
        return;
    }
    hchk(hipMemcpyAsync(sl.d_iq.get(), sl.h_iq.get(), (size_t)d_n * d_chunk * sb, hipMemcpyHostToDevice, hs), "H2D");
    if (d_mode == QRL_MODEM_DMR) chk(qrl_demod_set_dmo_output(d_h.get(), sl.dmo.dev(), kDmoCap, sl.dmocnt.dev()), "qrl_demod_set_dmo_output");
    sl.scoped = d_scope_on;
    chk(qrl_demod_set_time_domain_output(d_h.get(), d_scope_on ? reinterpret_cast<float*>(sl.scope.dev()) : nullptr, d_scap, d_scope_on ? sl.scnt.dev() : nullptr), "qrl_demod_set_time_domain_output");
    qrl_demod_out o{};
    o.filtered = sl.d_filt.get(); o.filtered_cap = d_fcap; o.constellation = reinterpret_cast<float*>(sl.konst.dev()); o.constellation_cap = d_ccap;
    o.bits_a = sl.a.dev(); o.bits_b = sl.b.dev(); o.bits_cap = d_bcap; o.counts = sl.cnt.dev();
    o.audio = sl.audio.dev(); o.audio_cap = d_acap;
    if (fmt == FMT_SC8) chk(qrl_demod_process_sc8(d_h.get(), reinterpret_cast<const int8_t*>(sl.d_iq.get()), d_chunk, n, &o), "qrl_demod_process_sc8");
    else if (fmt == FMT_CU8) chk(qrl_demod_process_cu8(d_h.get(), reinterpret_cast<const uint8_t*>(sl.d_iq.get()), d_chunk, n, &o), "qrl_demod_process_cu8");
    else if (sc16) chk(qrl_demod_process_sc16(d_h.get(), reinterpret_cast<const int16_t*>(sl.d_iq.get()), d_chunk, n, &o), "qrl_demod_process_sc16");
    else chk(qrl_demod_process(d_h.get(), sl.d_iq.get(), d_chunk, n, &o), "qrl_demod_process");
    chk(qrl_demod_stream_wait(d_h.get(), cs), "qrl_demod_stream_wait");
    const size_t N = (size_t)d_n;
    if (d_acap) sl.audio.download(cs);
    sl.cnt.download(cs);
    if (sl.scoped) {
        sl.scnt.download(cs);
        sl.scope.download(cs);
    }
    sl.framed = d_fs[0] != nullptr;
    sl.m17 = false;
    sl.bits_copied = !sl.framed || d_keep_bits;
    if (sl.framed) {
        // the frame synchronisers run on the copy stream behind the demodulator (no host synchronisation in between): bits A / B of
        // this call -> records { type, nbytes | _modem_sync << 16, payload }; only those travel to the host
        for (int k = 0; k < 2; ++k) chk(qrl_framesync_set_activity_output(d_fs[k].get(), sl.frcnt[k].dev() + 2 * N), "qrl_framesync_set_activity_output");
        chk(qrl_framesync_process(d_fs[0].get(), sl.a.dev(), d_bcap, d_bcap, sl.cnt.dev() + 2, 4, sl.fr[0].dev(), d_frcap, sl.frcnt[0].dev()), "qrl_framesync_process");
        chk(qrl_framesync_process(d_fs[1].get(), sl.b.dev(), d_bcap, d_bcap, sl.cnt.dev() + 3, 4, sl.fr[1].dev(), d_frcap, sl.frcnt[1].dev()), "qrl_framesync_process");
        for (int k = 0; k < 2; ++k) {
            sl.frcnt[k].download(cs);
            sl.fr[k].download(cs);
        }
        sl.m17 = d_m17_on && d_m17_rx && sl.rec_m17.dev();
        if (sl.m17) {   // the link layer behind the synchroniser of bits A, on the same stream: the records of this call's frames
            const size_t cap = d_frcap / QRL_M17_FRAMESYNC_RECORD_BYTES;
            chk(qrl_m17_rx_process(d_m17_rx.get(), cs, sl.fr[0].dev(), d_frcap, sl.frcnt[0].dev(), cap, sl.rec_m17.dev()), "qrl_m17_rx_process");
            sl.rec_m17.download(cs);
        }
    }
    if (sl.bits_copied) {
        sl.a.download(cs);
        sl.b.download(cs);
    }
    sl.const_copied = d_const_on;
    if (d_const_on) sl.konst.download(cs);
    if (d_mode == QRL_MODEM_DMR) {
        sl.rep = d_rep_on && d_sink;
        // getDMRData(bool dmo): the bursts of the DMO slicer, or those the repeater-mode sink finds in port 2 of this call (on the copy stream, which
        // waits for the demodulator on the device); the same record either way, so everything behind it takes frames / fcnt
        const uint8_t* frames = sl.rep ? sl.d_rep.get() : sl.dmo.dev();
        const uint32_t* fcnt = sl.rep ? sl.d_repcnt.get() : sl.dmocnt.dev();
        if (sl.rep) {
            chk(qrl_dmr_sink_process(d_sink.get(), sl.a.dev(), d_bcap, d_bcap, sl.cnt.dev() + 2, 4, sl.d_rep.get(), sl.rec_info.dev(), kDmoCap, sl.d_repcnt.get()), "qrl_dmr_sink_process");
            sl.rec_info.download(cs);
        }
        sl.dmocnt.download(cs, fcnt);
        sl.dmo.download(cs, frames);
        sl.l2 = d_l2_on;
        if (sl.l2) {   // layer 2 on the copy stream, which waits for the slicer on the device: validate / FEC of the call's bursts, no host synchronisation
            chk(qrl_dmr_l2_decode(d_rt.ctx(), cs, frames, fcnt, N, kDmoCap, d_l2_fec ? 1 : 0, sl.rec_l2.dev()), "qrl_dmr_l2_decode");
            sl.rec_l2.download(cs);
        }
        sl.call = sl.l2 && d_call_on && d_call_rx;
        if (sl.call) {   // the call layer behind layer 2 on the same stream: every call of this handle goes through the copy stream, so the per-stream state is carried in order
            if (sl.rep) chk(qrl_dmr_rx_process_slots(d_call_rx.get(), cs, sl.rec_l2.dev(), sl.rec_info.dev(), fcnt, N, kDmoCap, sl.rec_call.dev()), "qrl_dmr_rx_process_slots");
            else chk(qrl_dmr_rx_process(d_call_rx.get(), cs, sl.rec_l2.dev(), fcnt, kDmoCap, sl.rec_call.dev()), "qrl_dmr_rx_process");
            sl.rec_call.download(cs);
        }
    }
    sl.rssi_valid = d_rssi_on;
    if (d_rssi_on) {   // rssi_valve open: port 0 of this call through rssi_block, the probe keeps the latest value
        chk(qrl_rssi_process(d_rssi.get(), sl.d_filt.get(), d_fcap, d_fcap, sl.cnt.dev(), 4, nullptr, 0, sl.rssi.dev(), nullptr), "qrl_rssi_process");
        sl.rssi.download(cs);
    }
    if (d_fft_on) fft_tap();
    hchk(hipEventRecord(sl.done.get(), cs), "hipEventRecord");
    const int prev = d_inflight;
    d_inflight = cur;
    ++d_calls;
    if (prev >= 0) harvest(prev);   // the GPU already has call k queued while the host waits for call k - 1
}
void gr_demod_base_hip::harvest(int which)
{
    slot& sl = *d_slot[which];
    hchk(hipEventSynchronize(sl.done.get()), "hipEventSynchronize");
    std::lock_guard<std::mutex> g(d_mutex);
    for (int s = 0; s < d_n; ++s) {
        const uint32_t* c = sl.cnt.host() + 4 * (size_t)s;
        if (sl.rssi_valid && c[0]) d_level[s] = sl.rssi.host()[s];
        // gr_sample_sink::work (src/gr/gr_sample_sink.cpp:66-89): while more than 524288 items wait, the new ones are dropped
        if (sl.scoped && d_boxs[s].size() <= 524288) {
            const gr_complex* p = sl.scope.host() + (size_t)s * d_scap;
            d_boxs[s].insert(d_boxs[s].end(), p, p + std::min<size_t>(sl.scnt.host()[s], d_scap));
        }
        if (d_acap) {   // analogue modes: port 1 is audio (gr_audio_sink), no bit / constellation ports
            // gr_audio_sink::work (src/gr/gr_audio_sink.cpp:68-90): more than one second waiting = the reader is too slow: drop it all
            if (d_boxa[s].size() > 8000) d_boxa[s].clear();
            else d_boxa[s].insert(d_boxa[s].end(), sl.audio.host() + (size_t)s * d_acap, sl.audio.host() + (size_t)s * d_acap + c[1]);
            continue;
        }
        // gr_bit_sink::work (src/gr/gr_bit_sink.cpp:61-83): while more than 1 Mi items wait, new ones are not taken (nothing is cleared);
        // gr_const_sink::work (src/gr/gr_const_sink.cpp:64-86): the same at 256 items
        if (sl.bits_copied) {
            if (d_box1[s].size() <= 1048576) d_box1[s].insert(d_box1[s].end(), sl.a.host() + (size_t)s * d_bcap, sl.a.host() + (size_t)s * d_bcap + c[2]);
            if (d_box2[s].size() <= 1048576) d_box2[s].insert(d_box2[s].end(), sl.b.host() + (size_t)s * d_bcap, sl.b.host() + (size_t)s * d_bcap + c[3]);
        }
        if (sl.framed) for (int k = 0; k < 2; ++k) {   // the records of this call, in order
            d_fbits[k][s] += c[2 + k];
            d_fact[k][s] += sl.frcnt[k].host()[2 * (size_t)d_n + s];
            const uint8_t* p = sl.fr[k].host() + (size_t)s * d_frcap;
            const uint32_t nbytes = std::min<uint32_t>(sl.frcnt[k].host()[2 * s], (uint32_t)d_frcap);
            uint32_t index = 0;   // of the record within the row: where its M17 link record lies
            for (uint32_t pos = 0; pos + 8 <= nbytes; ++index) {
                uint32_t hdr[2];
                std::memcpy(hdr, p + pos, 8);
                const uint32_t nb = hdr[1] & 0xFFFFu, padded = (nb + 3u) & ~3u;
                if (pos + 8 + padded > nbytes) break;
                frame_record r;
                r.type = hdr[0]; r.modem_sync = hdr[1] >> 16;
                r.payload.assign(p + pos + 8, p + pos + 8 + padded);
                r.payload.resize((size_t)padded + 4, 0);   // processReceivedData reads frame_length + 1 bytes
                if (k == 0 && sl.m17) {
                    const uint8_t* e = sl.rec_m17.host() + ((size_t)s * (d_frcap / QRL_M17_FRAMESYNC_RECORD_BYTES) + index) * QRL_M17_RX_RECORD_BYTES;
                    r.m17_event.assign(e, e + QRL_M17_RX_RECORD_BYTES);
                }
                d_boxf[k][s].push_back(std::move(r));
                pos += 8 + padded;
            }
        }
        if (sl.const_copied && d_boxc[s].size() <= 256) d_boxc[s].insert(d_boxc[s].end(), sl.konst.host() + (size_t)s * d_ccap, sl.konst.host() + (size_t)s * d_ccap + c[1]);
        if (d_mode == QRL_MODEM_DMR) {
            if (sl.dmocnt.host()[s] > kDmoCap) d_dmo_dropped += sl.dmocnt.host()[s] - kDmoCap;   // more bursts in one call than the record buffer holds
            for (uint32_t i = 0; i < sl.dmocnt.host()[s] && i < kDmoCap; ++i) {
                append_record(d_boxd[s], sl.dmo.host(), (size_t)s, i, QRL_DMO_RECORD_BYTES);
                if (sl.l2) append_record(d_boxl[s], sl.rec_l2.host(), (size_t)s, i, QRL_DMR_L2_RECORD_BYTES);
                if (sl.rep) append_record(d_boxi[s], sl.rec_info.host(), (size_t)s, i, QRL_DMR_SINK_INFO_BYTES);
                if (sl.call) append_record(d_boxe[s], sl.rec_call.host(), (size_t)s, i, QRL_DMR_RX_RECORD_BYTES);
            }
        }
    }
}
void gr_demod_base_hip::flush()
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (d_inflight >= 0) { harvest(d_inflight); d_inflight = -1; }
}
std::vector<unsigned char>* gr_demod_base_hip::getData(int nr, int stream)   // gr_bit_sink::get_data: >= 32 bits or nothing (src/gr/gr_bit_sink.cpp:45-59)
{
    std::lock_guard<std::mutex> g(d_mutex);
    std::vector<unsigned char>& box = nr == 2 ? d_box2[stream] : d_box1[stream];
    if (box.size() < 32) return nullptr;
    std::vector<unsigned char>* out = new std::vector<unsigned char>;
    out->swap(box);
    return out;
}
std::vector<float>* gr_demod_base_hip::getAudio(int stream)   // gr_demod_base::getAudio (src/gr/gr_demod_base.cpp:968-976)
{
    // gr_audio_sink::get_data (src/gr/gr_audio_sink.cpp:51-66): packets of 640 samples (40 ms at 8 ksps at the least), else nothing
    std::lock_guard<std::mutex> g(d_mutex);
    std::vector<float>& box = d_boxa[stream];
    if (box.size() < 640) return nullptr;
    std::vector<float>* out = new std::vector<float>(box.begin(), box.begin() + 640);
    box.erase(box.begin(), box.begin() + 640);
    return out;
}
void gr_demod_base_hip::set_squelch(int value)   // gr_demod_base.cpp:1186-1199
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_squelch = value;
    if (d_h && d_acap) chk(qrl_demod_set_squelch(d_h.get(), (double)value), "qrl_demod_set_squelch");
}
void gr_demod_base_hip::set_ctcss(float value)   // gr_demod_base.cpp:1212-1218 -> gr_demod_nbfm::set_ctcss on both NBFM instances (gr_demod_nbfm.cpp:97-123)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_ctcss = value;
    if (d_h && d_acap && (d_mode == QRL_MODEM_NBFM2500 || d_mode == QRL_MODEM_NBFM5000)) chk(qrl_demod_set_ctcss(d_h.get(), value), "qrl_demod_set_ctcss");
}
void gr_demod_base_hip::set_filter_width(int filter_width, int mode)   // gr_demod_base.cpp:1155-1185
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    switch (mode) {
    case QRL_MODEM_WBFM: case QRL_MODEM_AM5000: case QRL_MODEM_NBFM2500: case QRL_MODEM_NBFM5000: case QRL_MODEM_USB2500: case QRL_MODEM_LSB2500: break;
    default: return;   // the reference's default branch
    }
    if (d_h && d_acap && d_mode == mode) {
        flush();   // the chain restarts: what the running call produced belongs to the old filters (recursive lock)
        chk(qrl_demod_set_filter_width(d_h.get(), filter_width), "qrl_demod_set_filter_width");
    }
    d_width[mode] = filter_width;
}
void gr_demod_base_hip::set_gain(float value)   // gr_demod_base.cpp:1206-1210 -> gr_demod_ssb::set_gain on both SSB instances
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_if_gain = value;
    if (d_h && d_acap && (d_mode == QRL_MODEM_USB2500 || d_mode == QRL_MODEM_LSB2500)) chk(qrl_demod_set_gain(d_h.get(), value), "qrl_demod_set_gain");
}
// gr_demod_base::set_agc_attack(int) / set_agc_decay(int) (gr_demod_base.cpp:1420-1461): the GUI's integer knob becomes a rate here -- 0 -> 1, v < 0 -> 1 / -v,
// v > 0 -> 20 v (attack) or v (decay) -- and goes to the AM and both SSB receivers (_am, _usb, _lsb)
bool gr_demod_base_hip::has_agc() const { return d_mode == QRL_MODEM_AM5000 || d_mode == QRL_MODEM_USB2500 || d_mode == QRL_MODEM_LSB2500; }
void gr_demod_base_hip::set_agc_attack(int value)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_agc_attack = value == 0 ? 1.0f : value < 0 ? 1.0f / (float)-value : (float)value * 20.0f;
    if (d_h && d_acap && has_agc()) chk(qrl_demod_set_agc(d_h.get(), d_agc_attack, d_agc_decay), "qrl_demod_set_agc");
}
void gr_demod_base_hip::set_agc_decay(int value)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_agc_decay = value == 0 ? 1.0f : value < 0 ? 1.0f / (float)-value : (float)value;
    if (d_h && d_acap && has_agc()) chk(qrl_demod_set_agc(d_h.get(), d_agc_attack, d_agc_decay), "qrl_demod_set_agc");
}
std::vector<gr_complex>* gr_demod_base_hip::get_constellation_data(int stream)
{
    std::lock_guard<std::mutex> g(d_mutex);
    if (d_boxc[stream].size() < 32) return nullptr;      // gr_const_sink::get_data (src/gr/gr_const_sink.cpp:48-62)
    std::vector<gr_complex>* out = new std::vector<gr_complex>;
    out->swap(d_boxc[stream]);
    return out;
}
float gr_demod_base_hip::get_rssi(int stream)   // gr_demod_base.cpp:1234-1237
{
    std::lock_guard<std::mutex> g(d_mutex);
    return d_level[stream];
}
void gr_demod_base_hip::calibrate_rssi(float value)   // :1413-1418
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_rssi_cal = value;
    if (d_rssi.get()) chk(qrl_rssi_set_level(d_rssi.get(), value), "qrl_rssi_set_level");
}
void gr_demod_base_hip::enable_time_domain(bool value)   // gr_demod_base.cpp:1115-1147 (+ gr_sample_sink::set_enabled)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_scope_on = value;
}
void gr_demod_base_hip::reconfigure_scope(int samp_rate, double filter_width)
{
    // The engine plans the scope decimator at create time and is stricter than the reference's setters (rates above 500 ksps, widths above 500 kHz and
    // filters of more than 4096 taps -- rates below ~2.4 ksps, widths below ~590 Hz -- are rejected).  A rejected value must not cost the caller the
    // demodulator: the old settings come back, the handle is re-opened with them, and the call throws std::invalid_argument.
    const int old_rate = d_scope_rate; const double old_fw = d_scope_fw;
    if (samp_rate > 500000 || filter_width < 0.0 || filter_width > 500000.0 || (samp_rate > 0 && samp_rate / 2 - samp_rate / 8 <= 0))
        throw std::invalid_argument("gr_demod_base_hip: time-domain sample rate / filter width outside what the engine plans (rate <= 500000, width <= 500000)");
    d_scope_rate = samp_rate; d_scope_fw = filter_width;
    if (d_mode < 0) return;
    flush();
    try { open(); }
    catch (const std::exception& e) {
        d_scope_rate = old_rate; d_scope_fw = old_fw;
        open();   // the settings the handle had before: this worked when it was created
        throw std::invalid_argument(std::string("gr_demod_base_hip: time-domain settings rejected, previous ones restored: ") + e.what());
    }
    std::lock_guard<std::mutex> g(d_mutex);
    for (auto& b : d_boxs) b.clear();   // the handle keeps history for the filter it was created with
}
void gr_demod_base_hip::set_time_sink_samp_rate(int samp_rate)   // gr_demod_base.cpp:1249-1290: a new resampler (decimation 1e6 / samp_rate, its own low-pass) under lock()
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if ((unsigned)samp_rate > 1000000u) return;   // :1251-1252
    reconfigure_scope(samp_rate, 0.0);
}
void gr_demod_base_hip::set_time_domain_filter_width(double filter_width)   // :1292-1301: set_taps(low_pass(1, 1e6, width, width, HAMMING)) on the current resampler
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    reconfigure_scope(d_scope_rate, filter_width);
}
void gr_demod_base_hip::set_sample_window(unsigned int size)   // gr_sample_sink::set_sample_window (:35-41): odd sizes go up by one
{
    std::lock_guard<std::mutex> g(d_mutex);
    if (size % 2 != 0) size = size + 1;
    d_window = size;
}
void gr_demod_base_hip::get_sample_data(float* sample_data, unsigned int& size, int stream)   // :988-1013 over gr_sample_sink::get_data (:49-66)
{
    std::lock_guard<std::mutex> g(d_mutex);
    std::vector<gr_complex>& box = d_boxs[stream];
    size = 0;
    if (box.size() < 2) return;
    unsigned int n = (unsigned int)std::min<size_t>(box.size(), d_window);
    if (n % 2 != 0) n = n - 1;
    // the reference writes the reals to [0, n) and the imaginaries to [n + 1, 2 n + 1) -- one slot is skipped (i + j + 1 with i == n, :1004-1009)
    for (unsigned int i = 0; i < n; i++) sample_data[i] = box[i].real();
    for (unsigned int j = 0; j < n; j++) sample_data[n + j + 1] = box[j].imag();
    size = n * 2;
    box.erase(box.begin(), box.begin() + n);
}
void gr_demod_base_hip::enable_gui_fft(bool value)   // :1110-1113
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_fft_on = value;
    if (d_fft.get()) chk(qrl_fft_set_enabled(d_fft.get(), value ? 1 : 0), "qrl_fft_set_enabled");
}
void gr_demod_base_hip::set_fft_size(int size)   // :1227-1232
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    flush();
    d_fftsize = (unsigned)size;
    if (d_fft.get()) chk(qrl_fft_set_fft_size(d_fft.get(), d_fftsize), "qrl_fft_set_fft_size");
    d_fftout.reset();
}
void gr_demod_base_hip::get_FFT_data(float* fft_data, unsigned int& fftSize, int stream)   // :978-986 -> rx_fft_c::get_fft_data
{
    fftSize = 0;
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!d_fft) return;
    if (!d_fftout.get()) d_fftout.alloc((size_t)d_n * d_fftsize);
    unsigned got = 0;
    chk(qrl_fft_get_fft_data(d_fft.get(), d_fftout.get(), d_fftsize, &got), "qrl_fft_get_fft_data");
    if (!got) return;
    hipStream_t cs = d_copy.get();
    d_fftlast.resize((size_t)d_n * got);   // every stream's spectrum of this frame: the other rows stay readable through last_FFT_data()
    hchk(hipMemcpyAsync(d_fftlast.data(), d_fftout.get(), d_fftlast.size() * sizeof(float), hipMemcpyDeviceToHost, cs), "D2H");
    hchk(hipStreamSynchronize(cs), "hipStreamSynchronize");
    std::memcpy(fft_data, d_fftlast.data() + (size_t)stream * got, (size_t)got * sizeof(float));
    fftSize = got;
}
records gr_demod_base_hip::getDMRData(int stream) { return take_box(d_mutex, d_boxd[stream]); }
records gr_demod_base_hip::getDMRDecoded(int stream) { return take_box(d_mutex, d_boxl[stream]); }
records gr_demod_base_hip::getDMRSlotInfo(int stream) { return stream < 0 || stream >= d_n ? records() : take_box(d_mutex, d_boxi[stream]); }
records gr_demod_base_hip::getDMRCallEvents(int stream) { return take_box(d_mutex, d_boxe[stream]); }

// ================================================================================================ gr_mod_base_hip
gr_mod_base_hip::gr_mod_base_hip(qrl_runtime& rt, int streams, int device_samp_rate, double carrier_offset_hz, size_t max_bytes)
    : d_rt(rt), d_n(streams), d_rate(device_samp_rate), d_offset(carrier_offset_hz), d_max(max_bytes), d_offsets((size_t)std::max(streams, 0), carrier_offset_hz), d_queue(streams), d_aqueue(streams), d_sent(streams, 0), d_clipped((size_t)std::max(streams, 0), 0),
      d_dmr_jobs((size_t)std::max(streams, 0)), d_dmr_call((size_t)std::max(streams, 0)), d_dmr_next((size_t)std::max(streams, 0), 0),
      d_m17_call((size_t)std::max(streams, 0)), d_m17_next((size_t)std::max(streams, 0), 0)
{
    d_cw_n = std::min<size_t>(1024, d_max);   // a facade built for fewer than 1024 items per call must still key CW
}
gr_mod_base_hip::~gr_mod_base_hip() = default;
static bool tx_mode_has_back_end(int mode)   // qrl_mod_create builds the gr_mod_base back end (rotator + interpolator) for every family but these (tx.cpp)
{
    return !(mode == QRL_MODEM_M17 || mode == QRL_MODEM_BPSK8);
}
bool gr_mod_base_hip::any_offset() const
{
    if (d_offset != 0.0) return true;
    for (double f : d_offsets) if (f != 0.0) return true;
    return false;
}
static bool analog_tx_mode(int mode)
{
    return mode == QRL_MODEM_NBFM2500 || mode == QRL_MODEM_NBFM5000 || mode == QRL_MODEM_AM5000 || mode == QRL_MODEM_USB2500 || mode == QRL_MODEM_LSB2500 ||
           mode == QRL_MODEM_CW600USB;
}
void gr_mod_base_hip::open()
{
    // create first, swap in on success: a mode / offset the engine rejects leaves the running modulator intact
    const bool backend = d_rate >= 2000000 || any_offset();
    // the engine builds the back end at 1 Msps only for a non-zero configured offset: any stream's will do, open() sets each stream's below
    double cfg_offset = d_offset;
    if (d_per_stream && cfg_offset == 0.0) for (double f : d_offsets) if (f != 0.0) { cfg_offset = f; break; }
    mod_handle nh; amod_handle nah; dev_buf<uint8_t> nbytes; dev_buf<float> naudio, niq;
    size_t spblock = 0, bpb = 1;
    if (!d_clip.get()) d_clip.alloc((size_t)d_n);   // one per stream, for the life of the facade
    if (analog_tx_mode(d_mode)) {
        qrl_amod_config c{};
        c.modem_type = d_mode; c.batch = d_n; c.max_samples = d_max; c.bb_gain = d_gain;
        c.device_samp_rate = d_rate; c.carrier_offset_hz = cfg_offset;
        qrl_amod* h = nullptr;
        chk(qrl_amod_create(d_rt.ctx(), &c, &h), "qrl_amod_create");
        nah.reset(h);
        if (d_per_stream && backend) chk(qrl_amod_set_carrier_offsets(h, d_offsets.data()), "qrl_amod_set_carrier_offsets");
        // the reference's instances keep what their setters did across mode changes
        if (d_ctcss_touched && (d_mode == QRL_MODEM_NBFM2500 || d_mode == QRL_MODEM_NBFM5000)) chk(qrl_amod_set_ctcss(h, d_ctcss), "qrl_amod_set_ctcss");
        if (d_width.count(d_mode)) chk(qrl_amod_set_filter_width(h, d_width[d_mode]), "qrl_amod_set_filter_width");
        if (d_mode == QRL_MODEM_CW600USB && d_cw_key) chk(qrl_amod_set_cw_k(h, 1), "qrl_amod_set_cw_k");
        chk(qrl_amod_set_sc16_scale(h, d_sc16_scale), "qrl_amod_set_sc16_scale");
        chk(qrl_amod_set_sc16_clip_counts(h, d_clip.get()), "qrl_amod_set_sc16_clip_counts");
        chk(qrl_amod_set_sc8_scale(h, d_sc8_scale), "qrl_amod_set_sc8_scale");
        chk(qrl_amod_set_sc8_clip_counts(h, d_clip.get()), "qrl_amod_set_sc8_clip_counts");   // a pass has one format: the counters are shared
        naudio.alloc((size_t)d_n * d_max);
        niq.alloc(2 * (size_t)d_n * qrl_amod_out_cap(h, d_max));   // interleaved cf32
    } else {
        qrl_mod_config c{};
        c.modem_type = d_mode; c.use_mode_defaults = 1; c.batch = d_n; c.max_bytes = d_max; c.bb_gain = d_gain;
        c.device_samp_rate = d_rate; c.carrier_offset_hz = cfg_offset;
        qrl_mod* h = nullptr;
        chk(qrl_mod_create(d_rt.ctx(), &c, &h), "qrl_mod_create");
        nh.reset(h);
        chk(qrl_mod_set_sc16_scale(h, d_sc16_scale), "qrl_mod_set_sc16_scale");
        chk(qrl_mod_set_sc16_clip_counts(h, d_clip.get()), "qrl_mod_set_sc16_clip_counts");
        chk(qrl_mod_set_sc8_scale(h, d_sc8_scale), "qrl_mod_set_sc8_scale");
        chk(qrl_mod_set_sc8_clip_counts(h, d_clip.get()), "qrl_mod_set_sc8_clip_counts");   // a pass has one format: the counters are shared
        if (d_per_stream && backend && tx_mode_has_back_end(d_mode)) chk(qrl_mod_set_carrier_offsets(h, d_offsets.data()), "qrl_mod_set_carrier_offsets");
        nbytes.alloc((size_t)d_n * d_max);
        spblock = qrl_mod_samples_per_block(h, &bpb);     // M17: 2500 samples per 3 bytes; every other mode: samples per byte, 1
        niq.alloc(2 * (size_t)d_n * (d_max / bpb + 1) * spblock);   // interleaved cf32
    }
    // nothing threw: the new ones move in, the old ones go (the handles now, the buffers with this function's locals)
    d_h = std::move(nh); d_ah = std::move(nah); d_bytes = std::move(nbytes); d_audio = std::move(naudio); d_iq = std::move(niq); d_backend = backend;
    if (d_h) { d_spblock = spblock; d_bpb = bpb; }
    d_cw_n = std::min(d_cw_n, d_max);
    // a new handle counts its items from zero: whatever was queued for the old one (and the byte positions of its zero runs) goes with it
    std::lock_guard<std::mutex> g(d_mutex);
    for (auto& q : d_queue) q.clear();
    for (auto& q : d_aqueue) q.clear();
    for (auto& j : d_dmr_jobs) j.clear();
    for (auto& v : d_sent) v = 0;
}
void gr_mod_base_hip::set_mode(int mode)   // gr_mod_base::set_mode (src/gr/gr_mod_base.cpp:354-763): new graph, queued bytes dropped
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    const int old = d_mode;
    d_mode = mode;
    try { open(); }
    catch (...) { d_mode = old; throw; }   // the previous modulator is still open
}
int gr_mod_base_hip::setDMRData(const std::vector<std::vector<uint8_t>>& frames, int stream)   // gr_mod_base.cpp:788-791 -> gr_dmr_source.cpp:56-73
{
    // d_hmutex is held by work() across qrl_mod_process: the bytes and the zero runs that belong to them become visible to a pass together
    // (gr_dmr_source::set_data takes the source's mutex for the same reason, gr_dmr_source.cpp:56-73)
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (d_mode != QRL_MODEM_DMR || !d_h) throw std::runtime_error("gr_mod_base_hip::setDMRData outside DMR mode");
    constexpr size_t kZeroBytes = 33 + 2 * 3;            // DMR_ZERO_TX_LENGTH_BYTES = FRAME_LENGTH_BYTES + 2 CACH_LENGTH_BYTES (gr_dmr_source.cpp:24)
    std::vector<qrl_zero_run> runs;
    std::lock_guard<std::mutex> g(d_mutex);
    auto& q = d_queue[stream];
    const size_t q0 = q.size();
    for (const auto& f : frames) {
        q.insert(q.end(), f.begin(), f.end());
        const uint64_t first_zero = d_sent[stream] + q.size();   // byte index of the tag (gr_dmr_source.cpp:118-121)
        q.insert(q.end(), kZeroBytes, (uint8_t)0);
        qrl_zero_run z{};
        z.stream = stream; z.channel = 0; z.start = first_zero * 20u; z.count = kZeroBytes * 4u * 5u;   // DMR_ZERO_TX_LENGTH_SAMPLES (:25)
        runs.push_back(z);
    }
    if (!runs.empty() && qrl_mod_add_zero_runs(d_h.get(), runs.data(), runs.size()) != QRL_OK) {
        q.resize(q0);   // bytes without their idle zeros would be a different waveform: all or nothing
        throw std::runtime_error(std::string("qrl_mod_add_zero_runs: ") + qrl_last_error());
    }
    return 0;
}
void gr_mod_base_hip::setDMRCall(const uint8_t* descriptor40, int stream)   // the call of the stream's next voice bursts; DMRControl::initVoiceTX
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (d_mode != QRL_MODEM_DMR || !d_h) throw std::runtime_error("gr_mod_base_hip::setDMRCall outside DMR mode");
    std::lock_guard<std::mutex> g(d_mutex);
    d_dmr_call.at((size_t)stream).assign(descriptor40, descriptor40 + QRL_DMR_CALL_BYTES);
    d_dmr_next[(size_t)stream] = 0;
}
// one qrl_m17_call_* launch on the null stream and a blocking copy of its bytes, which then take the byte path
void gr_mod_base_hip::queue_m17(int kind, const uint8_t* payloads, size_t n, int stream)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (d_mode != QRL_MODEM_M17 || !d_h) throw std::runtime_error("gr_mod_base_hip: an M17 call outside M17 mode");
    if (d_m17_call.at((size_t)stream).empty()) throw std::runtime_error("gr_mod_base_hip: txM17Audio / endM17Call before setM17Call");
    const size_t bytes = kind == 0 ? QRL_M17_CALL_START_BYTES : kind == 2 ? QRL_M17_CALL_END_BYTES : n * 48;
    const size_t in = QRL_M17_CALL_BYTES + 4 + (kind == 1 ? n * 16 : 0);
    dev_buf<uint8_t> buf;
    buf.alloc(in + bytes);
    uint8_t* dev = buf.get();
    std::vector<uint8_t> h(in);
    std::memcpy(h.data(), d_m17_call[(size_t)stream].data(), QRL_M17_CALL_BYTES);
    std::memcpy(h.data() + QRL_M17_CALL_BYTES, &d_m17_next[(size_t)stream], 4);
    if (kind == 1) std::memcpy(h.data() + QRL_M17_CALL_BYTES + 4, payloads, n * 16);
    auto out = std::make_unique<std::vector<uint8_t>>(bytes);
    hchk(hipMemcpy(dev, h.data(), in, hipMemcpyHostToDevice), "hipMemcpy");
    const uint32_t* first = reinterpret_cast<const uint32_t*>(dev + QRL_M17_CALL_BYTES);
    uint8_t* o = dev + in;
    if (kind == 0) chk(qrl_m17_call_start(d_rt.ctx(), nullptr, dev, 1, o, bytes), "qrl_m17_call");
    else if (kind == 1) chk(qrl_m17_call_encode(d_rt.ctx(), nullptr, dev, dev + QRL_M17_CALL_BYTES + 4, first, 1, n, o, bytes, 48), "qrl_m17_call");
    else chk(qrl_m17_call_end(d_rt.ctx(), nullptr, dev, first, 1, o, bytes), "qrl_m17_call");
    hchk(hipMemcpy(out->data(), o, bytes, hipMemcpyDeviceToHost), "hipMemcpy");   // (waits for the null stream)
    if (kind == 1) d_m17_next[(size_t)stream] += (uint32_t)n;
    set_data(out.release(), stream);
}
void gr_mod_base_hip::setM17Call(const uint8_t* descriptor32, int stream)   // M17Transmitter::start: the counters to 0, preamble and LSF frame
{
    {
        std::lock_guard<std::recursive_mutex> hg(d_hmutex);
        if (d_mode != QRL_MODEM_M17 || !d_h) throw std::runtime_error("gr_mod_base_hip::setM17Call outside M17 mode");
        d_m17_call.at((size_t)stream).assign(descriptor32, descriptor32 + QRL_M17_CALL_BYTES);
        d_m17_next[(size_t)stream] = 0;
    }
    queue_m17(0, nullptr, 0, stream);
}
int gr_mod_base_hip::txM17Audio(const uint8_t* payloads, size_t n, int stream)
{
    if (!n) return 0;
    queue_m17(1, payloads, n, stream);
    return (int)n;
}
void gr_mod_base_hip::endM17Call(int stream) { queue_m17(2, nullptr, 0, stream); }
int gr_mod_base_hip::txDMRVoice(const uint8_t* voice, size_t n, int stream)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);   // as in setDMRData: slots and their zero runs become visible to a pass together
    if (d_mode != QRL_MODEM_DMR || !d_h) throw std::runtime_error("gr_mod_base_hip::txDMRVoice outside DMR mode");
    if (d_dmr_call.at((size_t)stream).empty()) throw std::runtime_error("gr_mod_base_hip::txDMRVoice before setDMRCall");
    if (!n) return 0;
    constexpr size_t kSlot = 33 + 39, kZeroBytes = 39;   // a burst and gr_dmr_source's idle bytes (setDMRData)
    std::lock_guard<std::mutex> g(d_mutex);
    auto& q = d_queue[(size_t)stream];
    dmr_tx_job job;
    job.pos = d_sent[(size_t)stream] + q.size();
    job.first = d_dmr_next[(size_t)stream];
    job.n = n;
    job.call = d_dmr_call[(size_t)stream];
    job.voice.assign(voice, voice + 27 * n);
    std::vector<qrl_zero_run> runs(n);
    for (size_t i = 0; i < n; ++i) {
        runs[i] = qrl_zero_run{};
        runs[i].stream = stream; runs[i].start = (job.pos + i * kSlot + 33) * 20u; runs[i].count = kZeroBytes * 4u * 5u;
    }
    if (qrl_mod_add_zero_runs(d_h.get(), runs.data(), runs.size()) != QRL_OK) throw std::runtime_error(std::string("qrl_mod_add_zero_runs: ") + qrl_last_error());
    q.insert(q.end(), n * kSlot, (uint8_t)0);   // the slots: zeros here, the bursts are written on the device by the pass that sends them
    d_dmr_jobs[(size_t)stream].push_back(std::move(job));
    d_dmr_next[(size_t)stream] += (uint32_t)n;
    return (int)n;
}
// The part of every queued voice job that lies in this pass's window [window0[s], window0[s] + nb) of stream s, encoded into d_bytes on the
// modulator's stream behind the upload of the queue's bytes.  Runs of whole slots go straight into the modulator's input; a slot the window
// cuts is encoded into the staging buffer and its bytes inside the window are copied over (the pass that holds the rest encodes it again).
void gr_mod_base_hip::encode_dmr_jobs(const std::vector<uint64_t>& window0, size_t nb, void* stream)
{
    constexpr size_t kSlot = 72;
    hipStream_t ms = static_cast<hipStream_t>(stream);
    struct piece { size_t call, first, voice, n, dst, slot, skip, len; bool cut; };   // offsets into the staging buffer; dst into d_bytes
    std::vector<uint8_t> stage;
    std::vector<piece> pieces;
    auto put = [&](const void* p, size_t len) {
        const size_t o = (stage.size() + 3) & ~(size_t)3;
        stage.resize(o + len, 0);
        if (p) std::memcpy(stage.data() + o, p, len);
        return o;
    };
    {
        std::lock_guard<std::mutex> g(d_mutex);
        for (int s = 0; s < d_n; ++s) {
            auto& jobs = d_dmr_jobs[(size_t)s];
            const uint64_t a = window0[(size_t)s], b = a + nb;
            for (const auto& j : jobs) {
                if (j.pos >= b) break;
                const size_t k0 = j.pos >= a ? 0 : (size_t)((a - j.pos) / kSlot), k1 = std::min<uint64_t>(j.n, (b - j.pos + kSlot - 1) / kSlot);
                if (k0 >= k1) continue;
                const size_t call = put(j.call.data(), QRL_DMR_CALL_BYTES);
                auto emit = [&](size_t ka, size_t kb, bool cut) {   // slots ka .. kb - 1
                    const uint32_t first = j.first + (uint32_t)ka;
                    const uint64_t p = j.pos + ka * kSlot, lo = std::max(a, p), hi = std::min<uint64_t>(b, p + (kb - ka) * kSlot);
                    piece pc{};
                    pc.call = call; pc.first = put(&first, sizeof first); pc.voice = put(j.voice.data() + 27 * ka, 27 * (kb - ka)); pc.n = kb - ka;
                    pc.dst = (size_t)s * d_max + (size_t)(lo - a); pc.cut = cut;
                    if (cut) { pc.slot = put(nullptr, kSlot); pc.skip = (size_t)(lo - p); pc.len = (size_t)(hi - lo); }
                    pieces.push_back(pc);
                };
                size_t run = k0;   // first slot of the current run of whole slots
                for (size_t k = k0; k < k1; ++k) {
                    const uint64_t p = j.pos + k * kSlot;
                    if (p >= a && p + kSlot <= b) continue;
                    if (k > run) emit(run, k, false);
                    if (std::min<uint64_t>(b, p + kSlot) > std::max(a, p)) emit(k, k + 1, true);
                    run = k + 1;
                }
                if (k1 > run) emit(run, k1, false);
            }
            jobs.erase(std::remove_if(jobs.begin(), jobs.end(), [&](const dmr_tx_job& j) { return j.pos + j.n * kSlot <= b; }), jobs.end());
        }
    }
    if (pieces.empty()) return;
    if (stage.size() > d_dmr_dev.size()) d_dmr_dev.alloc(2 * stage.size());   // nothing of an earlier pass is in flight: every pass ends behind qrl_mod_sync
    uint8_t* const dmr_dev = d_dmr_dev.get();
    uint8_t* const bytes_dev = d_bytes.get();
    hchk(hipMemcpyAsync(dmr_dev, stage.data(), stage.size(), hipMemcpyHostToDevice, ms), "H2D");
    for (const auto& pc : pieces) {
        uint8_t* out = pc.cut ? dmr_dev + pc.slot : bytes_dev + pc.dst;
        chk(qrl_dmr_voice_call_encode(d_rt.ctx(), ms, dmr_dev + pc.call, dmr_dev + pc.voice, reinterpret_cast<const uint32_t*>(dmr_dev + pc.first), 1,
                                      pc.n, out, pc.n * kSlot, kSlot), "qrl_dmr_voice_call_encode");
        if (pc.cut) hchk(hipMemcpyAsync(bytes_dev + pc.dst, dmr_dev + pc.slot + pc.skip, pc.len, hipMemcpyDeviceToDevice, ms), "D2D");
    }
    hchk(hipStreamSynchronize(ms), "hipStreamSynchronize");   // the staging bytes are this function's
}
int gr_mod_base_hip::set_audio(std::vector<float>* data, int stream)   // gr_mod_base.cpp:793-797 -> gr_audio_source::set_data (gr_audio_source.cpp:55-66)
{
    std::lock_guard<std::mutex> g(d_mutex);
    d_aqueue[stream].insert(d_aqueue[stream].end(), data->begin(), data->end());
    delete data;
    return 0;
}
void gr_mod_base_hip::set_cw_k(bool value)   // gr_mod_base.cpp:948-956
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_cw_key = value;
    if (d_ah && d_mode == QRL_MODEM_CW600USB) chk(qrl_amod_set_cw_k(d_ah.get(), value ? 1 : 0), "qrl_amod_set_cw_k");
}
void gr_mod_base_hip::set_ctcss(float value)   // gr_mod_base.cpp:872-877
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_ctcss = value; d_ctcss_touched = true;
    if (d_ah && (d_mode == QRL_MODEM_NBFM2500 || d_mode == QRL_MODEM_NBFM5000)) chk(qrl_amod_set_ctcss(d_ah.get(), value), "qrl_amod_set_ctcss");
}
void gr_mod_base_hip::set_filter_width(int filter_width, int mode)   // gr_mod_base.cpp:878-905
{
    if (!analog_tx_mode(mode)) return;   // the reference's default branch
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (d_ah && d_mode == mode) chk(qrl_amod_set_filter_width(d_ah.get(), filter_width), "qrl_amod_set_filter_width");
    d_width[mode] = filter_width;
}
int gr_mod_base_hip::set_data(std::vector<uint8_t>* data, int stream)   // gr_mod_base.cpp:783-786 -> gr_byte_source::set_data (:54-62)
{
    std::lock_guard<std::mutex> g(d_mutex);
    d_queue[stream].insert(d_queue[stream].end(), data->begin(), data->end());
    delete data;
    return 1;
}
void gr_mod_base_hip::set_bb_gain(float v)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    d_gain = v;
    if (d_h.get()) chk(qrl_mod_set_bb_gain(d_h.get(), v), "qrl_mod_set_bb_gain");
    if (d_ah.get()) chk(qrl_amod_set_bb_gain(d_ah.get(), v), "qrl_amod_set_bb_gain");
}
void gr_mod_base_hip::set_carrier_offset(double hz)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    // a handle opened at 1 Msps with zero offset has no back end (no rotator to retune): zero stays a no-op, the first non-zero offset re-opens the handle with one
    // (the modulator restarts and what was queued is dropped; the reference's rotator is always in the graph, gr_mod_base.cpp:38).  The new handle is created
    // BEFORE the old one goes (open()), so a mode whose back end is not built (M17, DSSS) keeps its modulator and its offset, and the call throws.
    if (!d_backend) {
        if (hz == d_offset) return;
        if (d_mode >= 0 && !tx_mode_has_back_end(d_mode))
            throw std::invalid_argument("gr_mod_base_hip::set_carrier_offset: this mode's modulator has no rotator (M17 / DSSS back end not built); offset unchanged");
        const double old = d_offset;
        const std::vector<double> old_v = d_offsets;
        d_offset = hz;
        d_offsets.assign((size_t)d_n, hz);
        if (d_mode >= 0) {
            try { open(); }
            catch (...) { d_offset = old; d_offsets = old_v; throw; }
        }
        return;
    }
    if (d_h.get()) chk(qrl_mod_set_carrier_offset(d_h.get(), hz), "qrl_mod_set_carrier_offset");
    if (d_ah.get()) chk(qrl_amod_set_carrier_offset(d_ah.get(), hz), "qrl_amod_set_carrier_offset");
    d_offset = hz;
    d_offsets.assign((size_t)d_n, hz);
}
void gr_mod_base_hip::set_carrier_offset(double hz, int stream)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (stream < 0 || stream >= d_n) throw std::out_of_range("gr_mod_base_hip::set_carrier_offset: stream out of range");
    std::vector<double> v = d_offsets;
    v[(size_t)stream] = hz;
    if (!d_backend) {
        // the rule of the one-argument setter, for any stream: the first non-zero offset re-opens a back-end-less handle with a back end
        bool any = false;
        for (double f : v) any = any || f != 0.0;
        if (!any) { d_offsets.swap(v); return; }
        if (d_mode >= 0 && !tx_mode_has_back_end(d_mode))
            throw std::invalid_argument("gr_mod_base_hip::set_carrier_offset: this mode's modulator has no rotator (M17 / DSSS back end not built); offset unchanged");
        const std::vector<double> old_v = d_offsets;
        const bool old_ps = d_per_stream;
        d_offsets.swap(v);
        d_per_stream = true;
        if (d_mode >= 0) {
            try { open(); }
            catch (...) { d_offsets = old_v; d_per_stream = old_ps; throw; }
        }
        return;
    }
    if (d_h.get()) chk(qrl_mod_set_carrier_offsets(d_h.get(), v.data()), "qrl_mod_set_carrier_offsets");
    if (d_ah.get()) chk(qrl_amod_set_carrier_offsets(d_ah.get(), v.data()), "qrl_amod_set_carrier_offsets");
    d_offsets.swap(v);
    d_per_stream = true;
}
void gr_mod_base_hip::set_samp_rate(int device_samp_rate)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (device_samp_rate == d_rate) return;
    const int old = d_rate;
    d_rate = device_samp_rate;
    if (d_mode >= 0) {
        try { open(); }
        catch (...) { d_rate = old; throw; }   // the previous modulator is still open
    }
}
void gr_mod_base_hip::flush_sources()
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    std::lock_guard<std::mutex> g(d_mutex);
    // (bytes already counted into d_sent stay counted: the positions of later zero runs are stream positions of the modulator)
    for (auto& q : d_queue) q.clear();
    for (auto& q : d_aqueue) q.clear();
    for (auto& j : d_dmr_jobs) j.clear();   // their slots went with the queue
}
size_t gr_mod_base_hip::samples_per_byte() const { return d_h ? qrl_mod_samples_per_byte(d_h.get()) : 0; }
// int16 I/Q out (out[s] = interleaved int16 I, Q pairs): replaces the SDR driver's fc32 -> sc16 converter.  The modulator's last kernel converts
// (qrl_mod_process_sc16 / qrl_amod_process_sc16: r = rintf(x * scale), saturated), the download copies 4 bytes per sample, and the per-stream counters of
// clipped components come back with the samples (clipped()).
void gr_mod_base_hip::set_sc16_scale(float scale)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!std::isfinite(scale) || scale == 0.0f) throw std::invalid_argument("gr_mod_base_hip::set_sc16_scale: finite, non-zero");
    d_sc16_scale = scale;
    if (d_h.get()) chk(qrl_mod_set_sc16_scale(d_h.get(), scale), "qrl_mod_set_sc16_scale");
    if (d_ah.get()) chk(qrl_amod_set_sc16_scale(d_ah.get(), scale), "qrl_amod_set_sc16_scale");
}
// int8 I/Q out (out[s] = interleaved int8 I, Q pairs, what a HackRF takes): qrl_mod_process_sc8 / qrl_amod_process_sc8, 2 bytes per sample downloaded
void gr_mod_base_hip::set_sc8_scale(float scale)
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);
    if (!std::isfinite(scale) || scale == 0.0f) throw std::invalid_argument("gr_mod_base_hip::set_sc8_scale: finite, non-zero");
    d_sc8_scale = scale;
    if (d_h.get()) chk(qrl_mod_set_sc8_scale(d_h.get(), scale), "qrl_mod_set_sc8_scale");
    if (d_ah.get()) chk(qrl_amod_set_sc8_scale(d_ah.get(), scale), "qrl_amod_set_sc8_scale");
}
uint64_t gr_mod_base_hip::clipped(int stream) const
{
    std::lock_guard<std::recursive_mutex> hg(d_hmutex);   // work() adds to the totals under this lock: another thread may poll
    return d_clipped.at((size_t)stream);
}
size_t gr_mod_base_hip::work(gr_complex* const* out) { return work_any(reinterpret_cast<void* const*>(out), FMT_CF32); }
size_t gr_mod_base_hip::work(int16_t* const* out) { return work_any(reinterpret_cast<void* const*>(out), FMT_SC16); }
size_t gr_mod_base_hip::work(int8_t* const* out) { return work_any(reinterpret_cast<void* const*>(out), FMT_SC8); }
size_t gr_mod_base_hip::work_any(void* const* out, int fmt)
{
    const bool sc16 = fmt == FMT_SC16, sc8 = fmt == FMT_SC8;
    const size_t sb = sc8 ? 2 * sizeof(int8_t) : sc16 ? 2 * sizeof(int16_t) : sizeof(gr_complex);   // bytes per sample; the row pitch stays `stride` samples
    // one call of the open analogue handle into d_iq, in the format asked for
    auto amod = [&](const float* audio, size_t astride, size_t n, size_t stride) {
        if (sc16) chk(qrl_amod_process_sc16(d_ah.get(), audio, astride, n, reinterpret_cast<int16_t*>(d_iq.get()), stride), "qrl_amod_process_sc16");
        else if (sc8) chk(qrl_amod_process_sc8(d_ah.get(), audio, astride, n, reinterpret_cast<int8_t*>(d_iq.get()), stride), "qrl_amod_process_sc8");
        else chk(qrl_amod_process(d_ah.get(), audio, astride, n, d_iq.get(), stride), "qrl_amod_process");
    };
    // the samples of every stream, and for int16 / int8 the clip counters of this pass
    auto download = [&](size_t ns, size_t stride) {
        for (int s = 0; s < d_n && ns; ++s)
            hchk(hipMemcpy(out[s], reinterpret_cast<const char*>(d_iq.get()) + (size_t)s * stride * sb, ns * sb, hipMemcpyDeviceToHost), "D2H");
        if (!sc16 && !sc8) return;
        std::vector<uint32_t> c((size_t)d_n);
        hchk(hipMemcpy(c.data(), d_clip.get(), c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H");
        for (int s = 0; s < d_n; ++s) d_clipped[(size_t)s] += c[(size_t)s];
    };
    auto zero_clip = [&](hipStream_t ms) { if (sc16 || sc8) hchk(hipMemsetAsync(d_clip.get(), 0, (size_t)d_n * sizeof(uint32_t), ms), "hipMemsetAsync"); };

    std::lock_guard<std::recursive_mutex> hg(d_hmutex);   // the handle and its zero-run list for the whole pass; the byte / audio queues stay under d_mutex
    if (d_ah && d_mode == QRL_MODEM_CW600USB) {   // the tone source lives on the device: nothing to upload
        const size_t stride = qrl_amod_out_cap(d_ah.get(), d_max);
        zero_clip(static_cast<hipStream_t>(qrl_amod_stream(d_ah.get())));
        amod(nullptr, 0, d_cw_n, stride);
        chk(qrl_amod_sync(d_ah.get()), "qrl_amod_sync");
        const size_t ns = qrl_amod_last_count(d_ah.get());
        download(ns, stride);
        return ns;
    }
    if (d_ah.get()) {
        size_t na = 0;
        std::vector<float> host((size_t)d_n * d_max, 0.0f);
        {
            std::lock_guard<std::mutex> g(d_mutex);
            for (auto& q : d_aqueue) na = std::max(na, std::min(q.size(), d_max));
            if (d_mode == QRL_MODEM_NBFM2500 || d_mode == QRL_MODEM_NBFM5000) na -= na % 4;   // the 25:4 resampler; the rest waits for the next call
            if (na == 0) return 0;
            for (int s = 0; s < d_n; ++s) {   // a stream with fewer samples queued sends silence
                const size_t k = std::min(d_aqueue[s].size(), na);
                std::memcpy(host.data() + (size_t)s * d_max, d_aqueue[s].data(), k * sizeof(float));
                d_aqueue[s].erase(d_aqueue[s].begin(), d_aqueue[s].begin() + k);
            }
        }
        hipStream_t ms = static_cast<hipStream_t>(qrl_amod_stream(d_ah.get()));
        hchk(hipMemcpyAsync(d_audio.get(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ms), "H2D");
        const size_t stride = qrl_amod_out_cap(d_ah.get(), d_max);
        zero_clip(ms);
        amod(d_audio.get(), d_max, na, stride);
        chk(qrl_amod_sync(d_ah.get()), "qrl_amod_sync");
        const size_t ns = qrl_amod_last_count(d_ah.get());
        download(ns, stride);
        return ns;
    }
    if (!d_h) throw std::runtime_error("gr_mod_base_hip::work before set_mode");
    size_t nb = 0;
    std::vector<uint8_t> host((size_t)d_n * d_max, 0);
    std::vector<uint64_t> window0(d_sent);   // the stream position of this pass's first byte
    {
        std::lock_guard<std::mutex> g(d_mutex);
        for (auto& q : d_queue) nb = std::max(nb, std::min(q.size(), d_max));
        nb -= nb % d_bpb;                 // whole blocks only (M17: 3 bytes); the rest waits for the next call
        if (nb == 0) return 0;
        for (int s = 0; s < d_n; ++s) {   // a stream with fewer bytes queued sends zero bytes, like an idle gr_byte_source feeding zeros
            const size_t k = std::min(d_queue[s].size(), nb);
            std::memcpy(host.data() + (size_t)s * d_max, d_queue[s].data(), k);
            d_queue[s].erase(d_queue[s].begin(), d_queue[s].begin() + k);
            d_sent[s] += nb;
        }
    }
    hipStream_t ms = static_cast<hipStream_t>(qrl_mod_stream(d_h.get()));
    hchk(hipMemcpyAsync(d_bytes.get(), host.data(), host.size(), hipMemcpyHostToDevice, ms), "H2D");
    if (d_mode == QRL_MODEM_DMR) encode_dmr_jobs(window0, nb, ms);
    const size_t ns = nb / d_bpb * d_spblock, stride = (d_max / d_bpb + 1) * d_spblock;
    zero_clip(ms);
    if (sc16) chk(qrl_mod_process_sc16(d_h.get(), d_bytes.get(), d_max, nb, reinterpret_cast<int16_t*>(d_iq.get()), stride), "qrl_mod_process_sc16");
    else if (sc8) chk(qrl_mod_process_sc8(d_h.get(), d_bytes.get(), d_max, nb, reinterpret_cast<int8_t*>(d_iq.get()), stride), "qrl_mod_process_sc8");
    else chk(qrl_mod_process(d_h.get(), d_bytes.get(), d_max, nb, d_iq.get(), stride), "qrl_mod_process");
    chk(qrl_mod_sync(d_h.get()), "qrl_mod_sync");
    download(ns, stride);
    return ns;
}

// ================================================================================================ gr_modem_hip
gr_modem_hip::gr_modem_hip(gr_demod_base_hip* demod, gr_mod_base_hip* mod, gr_modem_events events)
    : _gr_demod_base(demod), _gr_mod_base(mod), _ev(std::move(events)), _rx(2 * (size_t)(demod ? demod->streams() : (mod ? mod->streams() : 1)))
{
}
void gr_modem_hip::toggleRxMode(int modem_type)   // gr_modem.cpp:203-322
{
    _modem_type_rx = modem_type;
    if (!_gr_demod_base) return;
    _gr_demod_base->enable_device_framing(_device_framing);
    _gr_demod_base->set_mode(modem_type);
    _rx_frame_length = modem_rx_frame_length(modem_type, &_bit_buf_len);
    for (auto& r : _rx) { r = rx_state(); r.bit_buf.assign((size_t)std::max(_bit_buf_len, 8), 0); }
}
void gr_modem_hip::toggleTxMode(int modem_type)   // gr_modem.cpp:105-199
{
    _modem_type_tx = modem_type;
    if (!_gr_mod_base) return;
    _gr_mod_base->set_mode(modem_type);
    _tx_frame_length = modem_tx_frame_length(modem_type);
}

bool gr_modem_hip::demodulateAnalog(int stream)
{
    if (!_gr_demod_base) return false;
    std::vector<float>* audio_data = _gr_demod_base->getAudio(stream);
    if (audio_data == nullptr) return false;
    if (audio_data->size() > 0) {
        if (_ev.pcmAudio) _ev.pcmAudio(stream, audio_data); else delete audio_data;
        return true;
    }
    delete audio_data;
    return false;
}
bool gr_modem_hip::demodulate(int stream)   // gr_modem.cpp:1019-1117
{
    if (!_gr_demod_base) return false;
    if (_modem_type_rx == QRL_MODEM_DMR) {   // :1025-1038 (getDMRData -> DMRControl::addFrames)
        auto frames = _gr_demod_base->getDMRData(stream);
        if (frames.empty()) return false;
        if (_ev.dmrFrames) _ev.dmrFrames(stream, frames);
        auto decoded = _gr_demod_base->getDMRDecoded(stream);   // set_dmr_l2: the same bursts validated and FEC'd on the device (DMRFrame::validate / runAudioFEC)
        if (!decoded.empty() && _ev.dmrFramesDecoded) _ev.dmrFramesDecoded(stream, decoded);
        auto events = _gr_demod_base->getDMRCallEvents(stream);   // set_dmr_call: what DMRControl::addFrames makes of each of them, per-stream state on the device
        if (!events.empty() && _ev.dmrCallEvents) _ev.dmrCallEvents(stream, events);
        auto info = _gr_demod_base->getDMRSlotInfo(stream);       // set_dmr_repeater: the slot record of each of them (CACH, timeslot, end_bit)
        if (!info.empty() && _ev.dmrSlotInfo) _ev.dmrSlotInfo(stream, info);
        return true;
    }
    const bool two = modem_two_branches(_modem_type_rx);
    if (device_framing()) {
        // the synchroniser ran on the device (qrl_framesync_process behind the demodulator): what arrives here are the frames
        // gr_modem::synchronize would have cut out of the bit stream, with _modem_sync as it stood when each frame completed.
        // Same dispatch as the host loop (processReceivedData, :1285-1441); two-branch modes: branch A's frames, then branch B's
        // (BranchRuleReference: branch A only -- the `>=` rule of :1080-1090 with equal counts).
        // Return value = the reference's: getData() hands out nothing below 32 bits -- then demodulate() returns false and consumes
        // nothing (:1057-1071; two-branch modes need both vectors) -- else synchronize()'s data_to_process: true iff a bit of this batch was collected
        // while a sync was held (:1121-1175), which k_framesync counts per call (qrl_framesync_set_activity_output).
        if (_gr_demod_base->peekFrameBits(1, stream) < 32 || (two && _gr_demod_base->peekFrameBits(2, stream) < 32)) return false;
        bool data_to_process = false;
        for (int k = 0; k < (two ? 2 : 1); ++k) {
            std::vector<gr_demod_base_hip::frame_record> recs;
            size_t bits = 0, collected = 0;
            if (!_gr_demod_base->takeFrames(k + 1, stream, recs, bits, collected)) continue;
            if (k == 1 && _branch_rule != BranchRuleBoth) continue;   // BranchRuleReference: branch B's vector is fetched and dropped
            rx_state& r = _rx[2 * (size_t)stream + (size_t)k];
            data_to_process = data_to_process || collected > 0;
            for (auto& f : recs) {
                r.modem_sync = (int)f.modem_sync;
                r.current_frame_type = f.type;
                processReceivedData(f.payload.data(), f.type, r, stream);
            }
            if (k == 0 && _ev.m17LinkEvents) {   // set_m17_link: the same frames through the link layer on the device
                std::vector<std::vector<unsigned char>> events;
                for (auto& f : recs) if (!f.m17_event.empty()) events.push_back(std::move(f.m17_event));
                if (!events.empty()) _ev.m17LinkEvents(stream, events);
            }
        }
        return data_to_process;
    }
    std::vector<unsigned char>*demod_data = nullptr, *demod_data2 = nullptr;
    if (two) {
        demod_data = _gr_demod_base->getData(1, stream);
        demod_data2 = _gr_demod_base->getData(2, stream);
        if (demod_data == nullptr || demod_data2 == nullptr) {
            // (the reference leaks whichever branch did come back, :1062-1063; here it is freed)
            delete demod_data; delete demod_data2;
            return false;
        }
    } else {
        demod_data = _gr_demod_base->getData(stream);
        if (demod_data == nullptr) return false;
    }
    bool data_to_process;
    if (two && _branch_rule == BranchRuleReference) {
        // :1080-1090: the longer vector wins, `>=` favours branch 1.  In the reference the two sinks are filled by scheduler
        // threads, so the comparison is an accident of timing; the device fills both mailboxes with the same count every call,
        // which turns the rule into "always branch 1" (kept selectable for like-for-like comparisons with the reference).
        std::vector<unsigned char>* data = demod_data->size() >= demod_data2->size() ? demod_data : demod_data2;
        data_to_process = synchronize((int)data->size(), data, _rx[2 * (size_t)stream], stream);
    } else if (two) {
        // default: both Viterbi alignments keep their own frame synchroniser; only the branch whose decoder is aligned with
        // the transmitter's code words ever finds a sync word, so frames are delivered once
        const bool a = synchronize((int)demod_data->size(), demod_data, _rx[2 * (size_t)stream], stream);
        const bool b = synchronize((int)demod_data2->size(), demod_data2, _rx[2 * (size_t)stream + 1], stream);
        data_to_process = a || b;
    } else {
        data_to_process = synchronize((int)demod_data->size(), demod_data, _rx[2 * (size_t)stream], stream);
    }
    delete demod_data;
    delete demod_data2;
    return data_to_process;
}

bool gr_modem_hip::synchronize(int v_size, std::vector<unsigned char>* data, rx_state& r, int stream)   // gr_modem.cpp:1119-1181
{
    bool data_to_process = false;
    const int m = _modem_type_rx;
    for (int i = 0; i < v_size; i++) {
        if (!r.sync_found) {
            r.current_frame_type = findSync((*data)[i], r);
            if (r.sync_found) {
                r.bit_buf_index = 0;
                if (r.modem_sync < 32) r.modem_sync += 8;
                continue;
            } else if (r.modem_sync > 0) {
                r.modem_sync -= 1;
            }
        }
        if (r.sync_found) {
            data_to_process = true;
            r.bit_buf[r.bit_buf_index] = (*data)[i] & 0x1;
            r.bit_buf_index++;
            int frame_length = _rx_frame_length, bit_buf_len = _bit_buf_len;
            if (!is_1k(m) && m != ModemTypeM17 && r.current_frame_type == FrameTypeVoice) frame_length++;   // reserved data
            else if (!is_1k(m) && m != ModemTypeM17 && r.current_frame_type != FrameTypeVoice) bit_buf_len = _bit_buf_len - 8;
            if (r.bit_buf_index >= bit_buf_len) {
                std::vector<unsigned char> frame_data((size_t)frame_length + 1, 0);
                for (int k = 0; k + 8 <= bit_buf_len; k += 8) {   // packBytes, :980-994
                    int t = 0;
                    for (int b = 0; b < 8; ++b) t = (t << 1) | (r.bit_buf[k + b] & 0x1);
                    if (k / 8 < (int)frame_data.size()) frame_data[k / 8] = (unsigned char)t;
                }
                processReceivedData(frame_data.data(), r.current_frame_type, r, stream);
                r.sync_found = false;
                r.shift_reg = 0;
                r.bit_buf_index = 0;
            }
        }
    }
    return data_to_process;
}

uint64_t gr_modem_hip::findSync(unsigned char bit, rx_state& r)   // gr_modem.cpp:1183-1282
{
    r.shift_reg = (r.shift_reg << 1) | (bit & 0x1);
    uint64_t temp;
    const int m = _modem_type_rx;
    if (m == ModemTypeM17) {   // :1187-1210
        temp = r.shift_reg & 0xFFFF;
        if (temp == FrameTypeM17LSF) { r.sync_found = true; return FrameTypeM17LSF; }
        if (temp == FrameTypeM17Stream) { r.sync_found = true; return FrameTypeM17Stream; }
        temp = r.shift_reg & 0xFFFFFFFF;
        if (temp == FrameTypeM17EOT) { r.sync_found = true; return FrameTypeM17EOT; }
        return FrameTypeNone;
    }
    if (is_1k(m)) {
        temp = r.shift_reg & 0xFF;
        if (temp == FrameTypeVoice1) { r.sync_found = true; return FrameTypeVoice1; }
        return FrameTypeNone;
    }
    if (m != QRL_MODEM_QPSK250K && m != QRL_MODEM_QPSKVIDEO && m != QRL_MODEM_4FSK100K) {
        temp = r.shift_reg & 0xFFFF;
        if (temp == FrameTypeVoice2) { r.sync_found = true; return FrameTypeVoice; }
        temp = r.shift_reg & 0xFFFFFF;
        if (temp == FrameTypeText) { r.sync_found = true; return FrameTypeText; }
        if (temp == FrameTypeProto) { r.sync_found = true; return FrameTypeProto; }
        if (temp == FrameTypeVideo) { r.sync_found = true; return FrameTypeVideo; }
        if (temp == FrameTypeCallsign) { r.sync_found = true; return FrameTypeCallsign; }
        if (temp == FrameTypeEnd) { r.sync_found = true; return FrameTypeEnd; }
        return FrameTypeNone;
    }
    temp = r.shift_reg & 0xFFFFFF;
    if (temp == FrameTypeIP) { r.sync_found = true; return FrameTypeIP; }
    if (temp == FrameTypeVideo) { r.sync_found = true; return FrameTypeVideo; }
    if (temp == FrameTypeEnd) { r.sync_found = true; return FrameTypeEnd; }
    return FrameTypeNone;
}

void gr_modem_hip::processReceivedData(unsigned char* received_data, uint64_t current_frame_type, rx_state& r, int stream)   // gr_modem.cpp:1285-1441
{
    const int L = _rx_frame_length;
    if (current_frame_type == FrameTypeEnd) {
        handleStreamEnd(r, stream);
    } else if (current_frame_type == FrameTypeText) {
        if (_ev.dataFrameReceived) _ev.dataFrameReceived(stream);
        r.last_frame_type = FrameTypeText;
        int string_length = L;
        for (int ii = L - 1; ii >= 0; ii--) { if (received_data[ii] == 0) string_length--; else break; }   // trailing NULs off
        if (_ev.textReceived) _ev.textReceived(stream, std::string(reinterpret_cast<const char*>(received_data), (size_t)string_length), false);
    } else if (current_frame_type == FrameTypeProto) {
        if (_ev.dataFrameReceived) _ev.dataFrameReceived(stream);
        r.last_frame_type = FrameTypeProto;
        if (_ev.protoReceived) _ev.protoReceived(stream, std::vector<unsigned char>(received_data, received_data + L));
    } else if (current_frame_type == FrameTypeCallsign) {
        r.last_frame_type = FrameTypeCallsign;
        std::string callsign;
        for (int i = 0; i < 7 && received_data[i]; ++i) {   // QRegExp("[^a-zA-Z/\\d\\s]") removed, first 7 characters kept
            const unsigned char c = received_data[i];
            if ((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '/' || c == ' ' || (c >= 9 && c <= 13)) callsign.push_back((char)c);
        }
        if (_ev.callsignReceived) _ev.callsignReceived(stream, callsign);
    } else if (current_frame_type == FrameTypeVoice1) {
        r.last_frame_type = FrameTypeVoice1;
        if (r.modem_sync >= 16 && _ev.digitalAudio) _ev.digitalAudio(stream, received_data, L);   // the voice gate of the 1k modes
    } else if (current_frame_type == FrameTypeVoice2) {
        r.last_frame_type = FrameTypeVoice2;
        if (_ev.digitalAudio) _ev.digitalAudio(stream, received_data + 1, L);   // one reserved byte in front
    } else if (current_frame_type == FrameTypeVideo) {
        if (_ev.dataFrameReceived) _ev.dataFrameReceived(stream);
        r.last_frame_type = FrameTypeVideo;
        if (_ev.videoData) _ev.videoData(stream, received_data, L);
    } else if (current_frame_type == FrameTypeIP) {
        r.last_frame_type = FrameTypeIP;
        if (_ev.netData) _ev.netData(stream, received_data, L);
    } else if (current_frame_type == FrameTypeM17Stream || current_frame_type == FrameTypeM17LSF || current_frame_type == FrameTypeM17EOT) {
        if (_ev.m17Frame) _ev.m17Frame(stream, current_frame_type, received_data, L);   // raw; the link layer's records of the same frames: m17LinkEvents (set_m17_link)
    }
}
void gr_modem_hip::handleStreamEnd(rx_state& r, int stream)   // gr_modem.cpp:1443-1451
{
    if (r.last_frame_type == FrameTypeText && _ev.textReceived) _ev.textReceived(stream, "\n", false);
    if (_ev.endAudioTransmission) _ev.endAudioTransmission(stream);
    if (_ev.receiveEnd) _ev.receiveEnd(stream);
}

// ---- TX
std::vector<unsigned char>* gr_modem_hip::frame(unsigned char* encoded_audio, int data_size, int frame_type)   // gr_modem.cpp:904-961
{
    std::vector<unsigned char>* data = new std::vector<unsigned char>;
    if ((uint64_t)frame_type == FrameTypeIP && _burst_ip_modem) for (int i = 0; i < 10; i++) data->push_back(0xAA);
    auto push3 = [&](uint64_t t) { data->push_back((unsigned char)((t >> 16) & 0xFF)); data->push_back((unsigned char)((t >> 8) & 0xFF)); data->push_back((unsigned char)(t & 0xFF)); };
    if ((uint64_t)frame_type == FrameTypeVoice) {
        if (is_1k(_modem_type_tx)) data->push_back((unsigned char)(FrameTypeVoice1 & 0xFF));
        else { data->push_back((unsigned char)((FrameTypeVoice2 >> 8) & 0xFF)); data->push_back((unsigned char)(FrameTypeVoice2 & 0xFF)); data->push_back(0xAA); }
    } else if ((uint64_t)frame_type == FrameTypeText) push3(FrameTypeText);
    else if ((uint64_t)frame_type == FrameTypeVideo) push3(FrameTypeVideo);
    else if ((uint64_t)frame_type == FrameTypeIP) push3(FrameTypeIP);
    else if ((uint64_t)frame_type == FrameTypeProto) push3(FrameTypeProto);
    for (int i = 0; i < data_size; i++) data->push_back(encoded_audio[i]);
    return data;
}
void gr_modem_hip::transmit(std::vector<std::vector<unsigned char>*> frames, int stream)   // gr_modem.cpp:963-978
{
    if (!_gr_mod_base) { for (auto* f : frames) delete f; return; }
    std::vector<unsigned char>* all_frames = new std::vector<unsigned char>;
    for (auto* f : frames) { all_frames->insert(all_frames->end(), f->begin(), f->end()); delete f; }
    _gr_mod_base->set_data(all_frames, stream);
}
void gr_modem_hip::sendCallsign(const std::string& callsign, int stream)   // gr_modem.cpp:654-676
{
    std::vector<unsigned char>* f = new std::vector<unsigned char>;
    f->push_back((unsigned char)((FrameTypeCallsign >> 16) & 0xFF));
    f->push_back((unsigned char)((FrameTypeCallsign >> 8) & 0xFF));
    f->push_back((unsigned char)(FrameTypeCallsign & 0xFF));
    for (char c : callsign) f->push_back((unsigned char)c);
    for (int i = 0; i < _tx_frame_length - (int)callsign.size(); i++) f->push_back(0x00);
    transmit({f}, stream);
}
void gr_modem_hip::startTransmission(const std::string& callsign, int stream)   // gr_modem.cpp:678-707 (digital modes)
{
    if (!_gr_mod_base) return;
    std::vector<unsigned char>* tx_start = new std::vector<unsigned char>;
    for (int i = 0; i < 8; i++) tx_start->push_back(0xAA);   // preamble of 48 bits incl. ramp-up
    transmit({tx_start}, stream);
    sendCallsign(callsign, stream);
}
void gr_modem_hip::endTransmission(const std::string& callsign, int stream)   // gr_modem.cpp:710-744 (digital modes)
{
    std::vector<unsigned char>* tx_end = new std::vector<unsigned char>;
    _frame_counter = 0;
    sendCallsign(callsign, stream);
    tx_end->push_back((unsigned char)((FrameTypeEnd >> 16) & 0xFF));
    tx_end->push_back((unsigned char)((FrameTypeEnd >> 8) & 0xFF));
    tx_end->push_back((unsigned char)(FrameTypeEnd & 0xFF));
    for (int i = 0; i < _tx_frame_length * 10; i++) tx_end->push_back(0xAA);
    transmit({tx_end}, stream);
}
void gr_modem_hip::transmitDigitalAudio(unsigned char* data, int size, int stream) { transmit({frame(data, size, (int)FrameTypeVoice)}, stream); delete[] data; }   // :857-864
void gr_modem_hip::transmitVideoData(unsigned char* data, int size, int stream) { transmit({frame(data, size, (int)FrameTypeVideo)}, stream); delete[] data; }      // :892-899
void gr_modem_hip::transmitNetData(unsigned char* data, int size, int stream) { transmit({frame(data, size, (int)FrameTypeIP)}, stream); delete[] data; }           // :901-908
void gr_modem_hip::transmitTextData(const std::string& text, int frame_type, int stream)   // gr_modem.cpp:812-832
{
    std::vector<std::vector<unsigned char>*> frames;
    for (size_t k = 0; k < text.size(); k += (size_t)_tx_frame_length) {
        const std::string chunk = text.substr(k, (size_t)_tx_frame_length);
        std::vector<unsigned char> d((size_t)_tx_frame_length, 0);
        std::memcpy(d.data(), chunk.data(), chunk.size());
        frames.push_back(frame(d.data(), _tx_frame_length, frame_type));
    }
    transmit(frames, stream);
}
void gr_modem_hip::transmitBinData(const std::vector<unsigned char>& bin, int frame_type, int stream)   // gr_modem.cpp:834-855
{
    std::vector<std::vector<unsigned char>*> frames;
    for (size_t k = 0; k < bin.size(); k += (size_t)_tx_frame_length) {
        std::vector<unsigned char> d((size_t)_tx_frame_length, 0);
        std::memcpy(d.data(), bin.data() + k, std::min((size_t)_tx_frame_length, bin.size() - k));
        frames.push_back(frame(d.data(), _tx_frame_length, frame_type));
    }
    transmit(frames, stream);
}

}  // namespace qrl_host
