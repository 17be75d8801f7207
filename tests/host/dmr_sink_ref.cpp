// dmr_sink_ref.cpp — the reference's own repeater-mode burst sink behind a C interface, for tests/test_dmr_sink.py and
// tools/make_dmr_sink_golden.py.  Includes the reference's headers from where they lie, links oracle/_ref/libqrl_ref.so and is compiled
// together with the reference's src/gr/gr_dmr_sink.cpp, src/DMR/dmrframe.cpp, src/DMR/dmrtiming.cpp and src/DMR/dmrcontrol.cpp, unmodified, against oracle/gr_stub
// (the GNU Radio base classes), tests/host/dmr_sink_stub (a Settings with the one more field DMRTiming reads), tests/host/dmr_rx_stub and
// tests/host/dmr_ctl_stub; nothing of the reference is copied.
//   ref_dmr_sink_work   one work() call on n bits with its rx_time tags -> the frames get_data() returns afterwards, as the 40-byte frame
//                       records and 16-byte slot records of qrl_dmr_sink_process (include/qrl_hip.h), and the (slot, value) pairs of every
//                       DMRTiming::timing_ready the call fired (the value set_slot_times stored: get_sample_counter() at that burst)
// The reference has no end_bit: a second gr_dmr_sink is fed the same bits one work() call per bit, and the bit after which its get_data()
// returns a frame is that frame's end_bit.  The two sinks must return the same frames, byte for byte, or the call fails: the second one
// enters work() at every bit, so its buffers are trimmed at other moments than the first one's.
// DMRTiming::timing_ready is the class's own signal, which moc would write; here it records.
//   ref_dmr_rxs_step    the call layer in either mode: one 40-byte frame record and its 16-byte slot record -> DMRFrame as
//                       tests/host/dmr_rx_ref.cpp builds it, with cachDecoded() and getSlotNo() as the sink's frame had them ->
//                       DMRControl::addFrames with that one frame -> the 128-byte record of qrl_dmr_rx_process_slots.  As in dmr_rx_ref.cpp a
//                       second DMRControl is fed the same frames through addFrames' own filters and the private process* functions, for the
//                       result of the call; which check refused a burst is asked of the reference's own processColorCode / processTimeslot
//                       on that second object, its locks put back afterwards.  src/DMR/dmrcontrol.cpp is compiled in unmodified as well.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <QObject>
#include <gnuradio/gr_complex.h>
#include "src/settings.h"
#include "src/logger.h"
#define private public
#include "src/DMR/dmrframe.h"
#include "src/DMR/dmrtiming.h"
#include "src/gr/gr_dmr_sink.h"
#undef private

namespace {
struct TimingEvent { uint64_t slot, value; };
std::vector<TimingEvent>* g_timing = nullptr;

struct Pair {
    Settings settings;
    DMRTiming *timing_a, *timing_b;
    gr_dmr_sink *a, *b;
    uint64_t total = 0;
    Pair()
    {
        settings.dmr_mode = DMR_MODE::DMR_MODE_REPEATER;
        timing_a = new DMRTiming(&settings); timing_b = new DMRTiming(&settings);
        a = new gr_dmr_sink(timing_a); b = new gr_dmr_sink(timing_b);
    }
    ~Pair() { delete a; delete b; delete timing_a; delete timing_b; }
};
struct Handle { Pair* p; };

void records(const DMRFrame& f, uint64_t end_bit, uint8_t* frame, uint8_t* info)
{
    memset(frame, 0, 40); memset(info, 0, 16);
    frame[0] = f._frame_type; frame[1] = f._FN;
    memcpy(frame + 4, f._frame_data, 33);
    info[0] = f._downlink ? 1 : 0; info[1] = f.cachDecoded() ? 1 : 0; info[2] = f.getSlotNo(); info[3] = f._lcss; info[4] = f._at;
    f.getCACH(info + 5);
    for (int i = 0; i < 8; ++i) info[8 + i] = (uint8_t)(end_bit >> (8 * i));
}

void run_work(gr_dmr_sink* s, const uint8_t* bits, int n, uint64_t read, const uint64_t* tag_off, const uint64_t* tag_secs, const double* tag_fracs, int ntags)
{
    s->stub_read = read;
    s->stub_in_tags.clear();
    for (int k = 0; k < ntags; ++k)
        s->stub_in_tags.push_back(gr::tag_t{tag_off[k], pmt::string_to_symbol("rx_time"),
                                            pmt::make_tuple(pmt::from_uint64(tag_secs[k]), pmt::from_double(tag_fracs[k])), 0});
    gr_vector_const_void_star in(1, bits);
    gr_vector_void_star out;
    s->work(n, in, out);
}
}  // namespace

void DMRTiming::timing_ready(unsigned int sn)
{
    if (g_timing) g_timing->push_back(TimingEvent{sn, _slot_times[sn - 1]});
}

extern "C" {

void* ref_dmr_sink_new() { Handle* h = new Handle; h->p = new Pair; return h; }
void ref_dmr_sink_free(void* p) { Handle* h = static_cast<Handle*>(p); delete h->p; delete h; }
void ref_dmr_sink_reset(void* p) { Handle* h = static_cast<Handle*>(p); delete h->p; h->p = new Pair; }
void ref_dmr_sink_flush(void* p) { Handle* h = static_cast<Handle*>(p); h->p->a->flush(); h->p->b->flush(); }

// the tags carry absolute bit offsets (counted from creation or reset).  frames [cap][40], info [cap][16], timing [cap][2].  Returns the
// number of frames the call found (at most cap are written; more is an error, -3), *ntiming the number of timing_ready events; -1 when the
// sink fed bit by bit disagrees with the one fed the whole call.
int ref_dmr_sink_work(void* p, const uint8_t* bits, int n, const uint64_t* tag_off, const uint64_t* tag_secs, const double* tag_fracs, int ntags,
                      uint8_t* frames, uint8_t* info, int cap, uint64_t* timing, int* ntiming)
{
    Pair* q = static_cast<Handle*>(p)->p;
    std::vector<TimingEvent> events, ignored;
    g_timing = &events;
    run_work(q->a, bits, n, q->total, tag_off, tag_secs, tag_fracs, ntags);
    g_timing = &ignored;
    std::vector<DMRFrame> fa = q->a->get_data();
    std::vector<DMRFrame> fb;
    std::vector<uint64_t> ends;
    for (int i = 0; i < n; ++i) {
        run_work(q->b, bits + i, 1, q->total + (uint64_t)i, tag_off, tag_secs, tag_fracs, ntags);
        for (const DMRFrame& f : q->b->get_data()) { fb.push_back(f); ends.push_back(q->total + (uint64_t)i + 1); }
    }
    g_timing = nullptr;
    q->total += (uint64_t)(n > 0 ? n : 0);
    *ntiming = (int)events.size();
    if (fa.size() != fb.size() || events.size() != ignored.size()) return -1;
    if ((int)fa.size() > cap || (int)events.size() > cap) return -3;
    for (size_t k = 0; k < fa.size(); ++k) {
        uint8_t f2[40], i2[16];
        records(fa[k], ends[k], frames + 40 * k, info + 16 * k);
        records(fb[k], ends[k], f2, i2);
        if (memcmp(f2, frames + 40 * k, 40) || memcmp(i2, info + 16 * k, 16)) return -1;
    }
    for (size_t k = 0; k < events.size(); ++k) {
        if (events[k].slot != ignored[k].slot || events[k].value != ignored[k].value) return -1;
        timing[2 * k] = events[k].slot; timing[2 * k + 1] = events[k].value;
    }
    return (int)fa.size();
}

// the first sink's private state: per context _state, _bits_to_receive, _frames_to_receive, _downlink, _bit_buffer.size(); then _next_slot
void ref_dmr_sink_state(void* p, uint32_t* out)
{
    const gr_dmr_sink* s = static_cast<Handle*>(p)->p->a;
    for (int c = 0; c < 2; ++c) {
        out[5 * c] = s->_state[c]; out[5 * c + 1] = s->_bits_to_receive[c]; out[5 * c + 2] = s->_frames_to_receive[c];
        out[5 * c + 3] = s->_downlink[c] ? 1 : 0; out[5 * c + 4] = (uint32_t)s->_bit_buffer[c].size();
    }
    out[10] = s->_next_slot;
}

}

// ---------------------------------------------------------------------------------------------------------------- the call layer, either mode
namespace {
struct Events { unsigned header = 0, terminator = 0, end_beep = 0, audio = 0, alias = 0, gps = 0, ta_df = 0, ta_dl = 0; std::vector<uint8_t> ta; };
Events* g_events = nullptr;

struct Rx {
    Settings settings;
    Logger logger_a, logger_b;
    void *mem_a, *mem_b;
    DMRControl *a, *b;
};
DMRControl* make_control(Settings* s, Logger* l, void** mem)
{
    *mem = calloc(1, sizeof(DMRControl));   // _ta_df and _ta_dl are never initialised by the class
    DMRControl* c = new (*mem) DMRControl(s, l);
    memset(c->_embedded_data_RX.m_raw, 0, 128 * sizeof(bool));
    memset(c->_embedded_data_RX.m_data, 0, 72 * sizeof(bool));
    return c;
}
bool same(const DMRControl* x, const DMRControl* y)
{
    return x->_receiver_state == y->_receiver_state && x->_color_code_RX == y->_color_code_RX && x->_timeslot_RX == y->_timeslot_RX &&
           x->_srcId_RX == y->_srcId_RX && x->_dstId_RX == y->_dstId_RX && x->_FLCO_RX == y->_FLCO_RX &&
           x->_talker_alias_received == y->_talker_alias_received && x->_ta_data.size() == y->_ta_data.size() &&
           x->_embedded_data_RX.m_state == y->_embedded_data_RX.m_state && x->_embedded_data_RX.m_valid == y->_embedded_data_RX.m_valid;
}
DMRFrame make_frame(const uint8_t* in, const uint8_t* slot)
{
    uint8_t burst[33];
    memcpy(burst, in + 4, 33);
    DMRFrame frame(burst, in[0]);
    frame.setFN(in[1]);
    frame._downlink = slot[0] != 0; frame._cach_decoded = slot[1] != 0; frame._slot_no = slot[2]; frame._lcss = slot[3]; frame._at = slot[4];
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

void ref_dmr_rxs_set(void* p, int color_code, int promiscuous, int mode, int timeslot)
{
    Rx* h = static_cast<Rx*>(p);
    h->settings.dmr_color_code = color_code; h->settings.dmr_promiscuous_mode = promiscuous != 0;
    h->settings.dmr_mode = mode; h->settings.dmr_timeslot = timeslot;
}
void* ref_dmr_rxs_new(int color_code, int promiscuous, int audio_fec, int mode, int timeslot)
{
    Rx* h = new Rx;
    h->settings.dmr_vocoder = audio_fec ? 1 : 0;
    ref_dmr_rxs_set(h, color_code, promiscuous, mode, timeslot);
    h->a = make_control(&h->settings, &h->logger_a, &h->mem_a);
    h->b = make_control(&h->settings, &h->logger_b, &h->mem_b);
    return h;
}
void ref_dmr_rxs_free(void* p)
{
    Rx* h = static_cast<Rx*>(p);
    h->a->~DMRControl(); h->b->~DMRControl();
    free(h->mem_a); free(h->mem_b);
    delete h;
}

// in: 40 bytes, slot: 16 bytes; out: 128 bytes.  0, or -1 when the second object's state differs from the first's, -2 when a signal fired an
// unexpected number of times
int ref_dmr_rxs_step(void* p, const uint8_t* in, const uint8_t* slot, uint8_t* out)
{
    Rx* h = static_cast<Rx*>(p);
    memset(out, 0, 128);
    Events ev;
    const unsigned unknown = h->logger_a.count[Logger::LogLevelDebug];
    const bool emb_valid_before = h->a->_embedded_data_RX.m_valid;
    g_events = &ev;
    std::vector<DMRFrame> frames;
    frames.push_back(make_frame(in, slot));
    h->a->addFrames(frames);
    g_events = nullptr;
    bool valid = false, result = false, slot_refused = false;
    {
        DMRFrame frame = make_frame(in, slot);
        DMRControl* b = h->b;
        const Settings& st = h->settings;
        valid = frame.validate();
        const bool repeater = st.dmr_mode != DMR_MODE::DMR_MODE_DMO;
        if (valid && repeater && (!frame.cachDecoded() || (frame.getSlotNo() != st.dmr_timeslot && !st.dmr_promiscuous_mode))) {
            slot_refused = true;   // addFrames' two filters (:636-644)
        } else if (valid) {
            const uint8_t dt = frame.getDataType();
            const bool audio = dt == DT_VOICE_SYNC || dt == DT_VOICE;
            if (audio) frame.setColorCode(b->_color_code_RX);
            // which check says no, asked of the class itself with the locks put back
            const bool passed_over = dt == DT_TERMINATOR_WITH_LC && frame.getDstId() == 0 && frame.getSrcId() == 0;
            const bool known = audio || dt == DT_CSBK || dt == DT_MBC_HEADER || dt == DT_MBC_CONTINUATION || dt == DT_DATA_HEADER ||
                               dt == DT_VOICE_LC_HEADER || dt == DT_TERMINATOR_WITH_LC;
            if (known && !passed_over) {
                const uint8_t cc0 = b->_color_code_RX, ts0 = b->_timeslot_RX;
                if (audio) slot_refused = !b->processTimeslot(frame);
                else slot_refused = b->processColorCode(frame) && !b->processTimeslot(frame);
                b->_color_code_RX = cc0; b->_timeslot_RX = ts0;
            }
            result = true;
            if (dt == DT_CSBK || dt == DT_MBC_HEADER || dt == DT_MBC_CONTINUATION) result = b->processCSBK(frame);
            else if (dt == DT_DATA_HEADER) result = b->processDataHeader(frame);
            else if (dt == DT_VOICE_LC_HEADER) result = b->processVoiceHeader(frame);
            else if (dt == DT_TERMINATOR_WITH_LC) result = b->processTerminator(frame);
            else if (audio) result = b->processAudio(frame);
        }
    }
    if (!same(h->a, h->b)) return -1;
    if (ev.header > 1 || ev.terminator > 1 || ev.end_beep > 1 || ev.audio > 1 || ev.alias > 1 || ev.gps > 1) return -2;
    const DMRControl* c = h->a;
    const bool embedded = !emb_valid_before && c->_embedded_data_RX.m_valid;
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
    if (slot_refused) flags |= 0x0800;
    out[0] = (uint8_t)flags; out[1] = (uint8_t)(flags >> 8);
    out[2] = (uint8_t)c->_receiver_state; out[3] = c->_color_code_RX; out[4] = c->_FLCO_RX; out[5] = c->_timeslot_RX;
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

}
