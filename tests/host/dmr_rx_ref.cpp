// dmr_rx_ref.cpp — the reference's own DMR receive call layer behind a C interface, for tests/test_dmr_rx.py and tools/make_dmr_rx_golden.py.
// Includes the reference's headers from where they lie, links oracle/_ref/libqrl_ref.so and is compiled together with the reference's
// src/DMR/dmrcontrol.cpp, unmodified, against the stand-ins of tests/host/dmr_rx_stub (a logger that counts, a QString) and, behind them, tests/host/dmr_ctl_stub;
// nothing of the reference is copied.
//   ref_dmr_rx_step      one 40-byte slicer record -> DMRFrame as tests/host/dmr_l2_ref.cpp builds it -> DMRControl::addFrames with that one
//                        frame -> the 128-byte record of qrl_dmr_rx_process (include/qrl_hip.h) from the signals fired and the private state
//   ref_embedded_decode  four 32-bit fragments through CDMREmbeddedData::addData
// The signals are DMRControl's own member functions, which moc would write; here they record.  talkerAlias fires before the class clears
// its buffer, so the alias bytes, format and length are read there.  What addFrames keeps to itself, the result of the process* call, comes
// from a second DMRControl that is fed the same frames through the private process* functions directly, by addFrames' dispatch; after
// every burst the two must agree in every field, or the step fails.  DMRControl never initialises _ta_df and _ta_dl: both objects are
// built in zeroed memory.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <string>
#include <vector>
// everything that is not the reference's own goes in first, so that only its classes are opened up
#include <QObject>
#include <gnuradio/gr_complex.h>
#include "src/settings.h"
#include "src/logger.h"
#include "src/DMR/dmrutils.h"
#define private public
#include "src/DMR/dmrcontrol.h"
#undef private
#include "src/DMR/dmrframe.h"

namespace {
struct Events {
    unsigned header = 0, terminator = 0, end_beep = 0, audio = 0, alias = 0, gps = 0;
    unsigned ta_df = 0, ta_dl = 0;
    std::vector<uint8_t> ta;
};
Events* g_events = nullptr;

struct Handle {
    Settings settings;
    Logger logger_a, logger_b;
    void *mem_a, *mem_b;
    DMRControl *a, *b;
};

DMRControl* make_control(Settings* s, Logger* l, void** mem)
{
    *mem = calloc(1, sizeof(DMRControl));
    DMRControl* c = new (*mem) DMRControl(s, l);
    memset(c->_embedded_data_RX.m_raw, 0, 128 * sizeof(bool));   // new bool[]: not initialised either, and never read before it is written
    memset(c->_embedded_data_RX.m_data, 0, 72 * sizeof(bool));
    return c;
}

bool same(const DMRControl* x, const DMRControl* y)
{
    return x->_receiver_state == y->_receiver_state && x->_color_code_RX == y->_color_code_RX && x->_srcId_RX == y->_srcId_RX &&
           x->_dstId_RX == y->_dstId_RX && x->_FLCO_RX == y->_FLCO_RX && x->_talker_alias_received == y->_talker_alias_received &&
           x->_ta_df == y->_ta_df && x->_ta_dl == y->_ta_dl && x->_ta_data.size() == y->_ta_data.size() &&
           (x->_ta_data.size() == 0 || !memcmp(x->_ta_data.constData(), y->_ta_data.constData(), (size_t)x->_ta_data.size())) &&
           x->_embedded_data_RX.m_state == y->_embedded_data_RX.m_state && x->_embedded_data_RX.m_valid == y->_embedded_data_RX.m_valid &&
           x->_embedded_data_RX.m_FLCO == y->_embedded_data_RX.m_FLCO && !memcmp(x->_embedded_data_RX.m_raw, y->_embedded_data_RX.m_raw, 128 * sizeof(bool));
}

DMRFrame make_frame(const uint8_t* in)
{
    uint8_t burst[33];
    memcpy(burst, in + 4, 33);
    DMRFrame frame(burst, in[0]);
    frame.setFN(in[1]);
    return frame;
}
}  // namespace

void DMRControl::digitalAudio(unsigned char* audiodata, int) { delete[] audiodata; if (g_events) ++g_events->audio; }
void DMRControl::talkerAlias(QString, bool)
{
    if (!g_events) return;
    ++g_events->alias;
    g_events->ta_df = _ta_df; g_events->ta_dl = _ta_dl;
    g_events->ta.assign((const uint8_t*)_ta_data.constData(), (const uint8_t*)_ta_data.constData() + _ta_data.size());
}
void DMRControl::gpsInfo(QString, bool) { if (g_events) ++g_events->gps; }
void DMRControl::headerReceived(QString, bool) { if (g_events) ++g_events->header; }
void DMRControl::terminatorReceived(QString, bool) { if (g_events) ++g_events->terminator; }
void DMRControl::endBeep() { if (g_events) ++g_events->end_beep; }

extern "C" {

void* ref_dmr_rx_new(int color_code, int promiscuous, int audio_fec)
{
    Handle* h = new Handle;
    h->settings.dmr_mode = DMR_MODE::DMR_MODE_DMO;
    h->settings.dmr_color_code = color_code;
    h->settings.dmr_promiscuous_mode = promiscuous != 0;
    h->settings.dmr_vocoder = audio_fec ? 1 : 0;
    h->a = make_control(&h->settings, &h->logger_a, &h->mem_a);
    h->b = make_control(&h->settings, &h->logger_b, &h->mem_b);
    return h;
}
void ref_dmr_rx_set_config(void* p, int color_code, int promiscuous)
{
    Handle* h = static_cast<Handle*>(p);
    h->settings.dmr_color_code = color_code;
    h->settings.dmr_promiscuous_mode = promiscuous != 0;
}
void ref_dmr_rx_free(void* p)
{
    Handle* h = static_cast<Handle*>(p);
    h->a->~DMRControl(); h->b->~DMRControl();
    free(h->mem_a); free(h->mem_b);
    delete h;
}

// in: 40 bytes; out: 128 bytes.  0, or -1 when the second object's state differs from the first's, -2 when a signal fired an unexpected
// number of times
int ref_dmr_rx_step(void* p, const uint8_t* in, uint8_t* out)
{
    Handle* h = static_cast<Handle*>(p);
    memset(out, 0, 128);
    Events ev;
    const unsigned warned = h->logger_a.count[Logger::LogLevelWarning], unknown = h->logger_a.count[Logger::LogLevelDebug];
    const bool emb_valid_before = h->a->_embedded_data_RX.m_valid;
    g_events = &ev;
    std::vector<DMRFrame> frames;
    frames.push_back(make_frame(in));
    h->a->addFrames(frames);
    g_events = nullptr;
    // the second object: the same frame through the same private function, for its result
    bool valid = false, result = true;
    {
        DMRFrame frame = make_frame(in);
        valid = frame.validate();
        if (valid) {
            const uint8_t dt = frame.getDataType();
            if (dt == DT_CSBK || dt == DT_MBC_HEADER || dt == DT_MBC_CONTINUATION) result = h->b->processCSBK(frame);
            else if (dt == DT_DATA_HEADER) result = h->b->processDataHeader(frame);
            else if (dt == DT_VOICE_LC_HEADER) result = h->b->processVoiceHeader(frame);
            else if (dt == DT_TERMINATOR_WITH_LC) result = h->b->processTerminator(frame);
            else if (dt == DT_VOICE_SYNC || dt == DT_VOICE) { frame.setColorCode(h->b->_color_code_RX); result = h->b->processAudio(frame); }
        }
    }
    if (!same(h->a, h->b)) return -1;
    if (valid != (h->logger_a.count[Logger::LogLevelWarning] == warned)) return -1;   // addFrames logs the burst it refuses
    if (ev.header > 1 || ev.terminator > 1 || ev.end_beep > 1 || ev.audio > 1 || ev.alias > 1 || ev.gps > 1) return -2;
    const DMRControl* c = h->a;
    const bool embedded = !emb_valid_before && c->_embedded_data_RX.m_valid;   // only a fourth fragment that decodes sets it
    unsigned flags = 0;
    if (valid) flags |= 0x0001;
    if (valid && result) flags |= 0x0002;
    if (ev.header && c->_receiver_state == RECEIVER_STATE::STATE_AUDIO) flags |= 0x0004;
    if (ev.header && c->_receiver_state == RECEIVER_STATE::STATE_DATA) flags |= 0x0008;
    if (ev.terminator) flags |= 0x0010;
    if (ev.end_beep) flags |= 0x0020;
    if (ev.audio) flags |= 0x0040;
    if (embedded) flags |= 0x0080;
    if (ev.alias) flags |= 0x0100;
    if (ev.gps) flags |= 0x0200;
    if (h->logger_a.count[Logger::LogLevelDebug] != unknown) flags |= 0x0400;
    out[0] = (uint8_t)flags; out[1] = (uint8_t)(flags >> 8);
    out[2] = (uint8_t)c->_receiver_state; out[3] = c->_color_code_RX; out[4] = c->_FLCO_RX;
    for (int i = 0; i < 4; ++i) { out[8 + i] = (uint8_t)(c->_srcId_RX >> (8 * i)); out[12 + i] = (uint8_t)(c->_dstId_RX >> (8 * i)); }
    if (embedded) {
        out[16] = (uint8_t)c->_embedded_data_RX.getFLCO();
        c->_embedded_data_RX.getRawData(out + 17);
    }
    if (ev.alias) {
        if (ev.ta.size() > 68) return -2;
        out[26] = (uint8_t)ev.ta_df; out[27] = (uint8_t)ev.ta_dl; out[28] = (uint8_t)ev.ta.size();
        memcpy(out + 32, ev.ta.data(), ev.ta.size());
    }
    return 0;
}

// the bytes the alias buffer holds now (at most cap are copied); returns its size
int ref_dmr_rx_alias_pending(void* p, uint8_t* out, int cap)
{
    const DMRControl* c = static_cast<Handle*>(p)->a;
    const int n = c->_ta_data.size();
    if (n > 0) memcpy(out, c->_ta_data.constData(), (size_t)(n < cap ? n : cap));
    return n;
}

// frag: four fragments, the first embedded bit of each highest.  data9: m_data packed, whatever the outcome (zero before anything was written).
// Returns isValid(); *flco = getFLCO().
int ref_embedded_decode(const uint32_t* frag, uint8_t* data9, int* flco)
{
    static const unsigned char lcss[4] = {1, 3, 3, 2};
    CDMREmbeddedData emb;
    memset(emb.m_data, 0, 72 * sizeof(bool));
    for (int k = 0; k < 4; ++k) {
        unsigned char d[33] = {};
        d[14] = (unsigned char)(frag[k] >> 28);
        d[15] = (unsigned char)(frag[k] >> 20); d[16] = (unsigned char)(frag[k] >> 12); d[17] = (unsigned char)(frag[k] >> 4);
        d[18] = (unsigned char)(frag[k] << 4);
        emb.addData(d, lcss[k]);
    }
    for (int i = 0; i < 9; ++i) { unsigned v = 0; for (int j = 0; j < 8; ++j) v = (v << 1) | (emb.m_data[8 * i + j] ? 1u : 0u); data9[i] = (uint8_t)v; }
    *flco = (int)emb.getFLCO();
    return emb.isValid() ? 1 : 0;
}

}
