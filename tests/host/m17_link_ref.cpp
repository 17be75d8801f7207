// m17_link_ref.cpp — the reference's own M17 link layer behind a C interface, for tests/test_m17_link.py and tools/make_m17_link_golden.py.
// Compiled together with the reference's gr_modem.cpp, M17Transmitter.cpp, M17FrameDecoder.cpp, M17LinkSetupFrame.cpp, M17Callsign.cpp and
// M17Golay.cpp, unmodified, where they lie, against the stand-in headers of oracle/qt_stub and oracle/gr_stub; nothing of the reference is copied.
//   ref_m17_step     one 56-byte record of the frame synchroniser -> gr_modem::processReceivedData -> the 64-byte record of qrl_m17_rx_process
//                    (include/qrl_hip.h) from the signals fired, their arguments and the decoder's private state; and that state itself
//   ref_m17_tx_*     Settings::m17_src / m17_dest / m17_can_tx / m17_destination_type, startTransmission, transmitM17Audio, endTransmission -> the
//                    bytes the class hands to the modulator
// The signals are gr_modem's own member functions, which moc would write; here they record.  What the class keeps to itself is read through
// its own accessors where there are any: the callsign texts of a frame that fires no signal come from getSource() / getDestination() of the
// decoder's LSF, and where m17FrameInfoReceived fires its arguments must be those, or the step fails.  Whether the LICH of a stream frame
// decoded is asked of the decoder's own decodeLich on the frame's own bytes (the reference's decorrelate / deinterleave in front).
// Two flags have no accessor and no signal and are worked out here beside the reference: _LICH_OK from that decodeLich call, _LSF_FROM_LICH by
// laying the segment into a copy of the decoder's image and asking the reference's valid() of it when the map completes.  That repeats the rule
// of decodeStream for these two bits only; what they lead to -- lsf, lsfFromLich, lsfSegmentMap and the lock after the frame -- is read from the
// reference's own members (ref_m17_state) and pins the core independently of them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include <array>
#include <bitset>
#include <complex>
#include <chrono>
#include <mutex>
#include <map>
#include <deque>
#include <algorithm>
#include <memory>
#include <experimental/array>

#define private public
#include "src/gr_modem.h"
#undef private
#include <M17/M17Decorrelator.hpp>
#include <M17/M17Interleaver.hpp>

namespace {
struct Events {
    unsigned info = 0, audio = 0, end_audio = 0, receive_end = 0, other = 0;
    std::string src, dst;
    unsigned can = 0;
    uint8_t payload[16] = {};
};
Events* g_ev = nullptr;

struct Handle {
    Settings settings; Logger logger; DMRControl dmr;
    gr_modem* m = nullptr;
};

void put_text(uint8_t* at, const std::string& s)
{
    at[0] = (uint8_t)s.size();
    memcpy(at + 1, s.data(), s.size() < 10 ? s.size() : 10);
}
}  // namespace

void gr_modem::pcmAudio(std::vector<float>* pcm) { if (g_ev) ++g_ev->other; delete pcm; }
void gr_modem::digitalAudio(unsigned char* d, int size)
{
    if (g_ev) { ++g_ev->audio; if (size == 16) memcpy(g_ev->payload, d, 16); else ++g_ev->other; }
    delete[] d;
}
void gr_modem::videoData(unsigned char* d, int) { if (g_ev) ++g_ev->other; delete[] d; }
void gr_modem::netData(unsigned char* d, int) { if (g_ev) ++g_ev->other; delete[] d; }
void gr_modem::demodulated_audio(short*, short) {}
void gr_modem::textReceived(QString, bool) { if (g_ev) ++g_ev->other; }
void gr_modem::protoReceived(QByteArray) { if (g_ev) ++g_ev->other; }
void gr_modem::callsignReceived(QString) { if (g_ev) ++g_ev->other; }
void gr_modem::m17FrameInfoReceived(QString src, QString dest, uint16_t CAN)
{
    if (!g_ev) return;
    ++g_ev->info; g_ev->src = src.toStdString(); g_ev->dst = dest.toStdString(); g_ev->can = CAN;
}
void gr_modem::audioFrameReceived() { if (g_ev) ++g_ev->other; }
void gr_modem::dataFrameReceived() { if (g_ev) ++g_ev->other; }
void gr_modem::syncIssues() { if (g_ev) ++g_ev->other; }
void gr_modem::receiveEnd() { if (g_ev) ++g_ev->receive_end; }
void gr_modem::endAudioTransmission() { if (g_ev) ++g_ev->end_audio; }
void gr_modem::endBeep() { if (g_ev) ++g_ev->other; }

extern "C" int qrl_stub_nanosleep(const struct timespec*, struct timespec*) { return 0; }

extern "C" {

void* ref_m17_new(int can_rx, int decode_all_can)
{
    Handle* h = new Handle;
    h->settings.m17_can_rx = can_rx;
    h->settings.m17_decode_all_can = decode_all_can;
    h->m = new gr_modem(&h->settings, &h->logger, &h->dmr);
    h->m->initRX(gr_modem_types::ModemTypeM17, "", "", 0);
    h->m->initTX(gr_modem_types::ModemTypeM17, 433500000, "", "", 0);
    h->m->_m17_decoder.reset();          // lsfSegmentMap is not initialised before the first reset()
    return h;
}
void ref_m17_free(void* p) { Handle* h = static_cast<Handle*>(p); delete h->m; delete h; }
void ref_m17_set_rx(void* p, int can_rx, int decode_all_can)
{
    Handle* h = static_cast<Handle*>(p);
    h->settings.m17_can_rx = can_rx; h->settings.m17_decode_all_can = decode_all_can;
}
int ref_m17_rx_frame_length(void* p) { return static_cast<Handle*>(p)->m->_rx_frame_length; }
int ref_m17_tx_frame_length(void* p) { return static_cast<Handle*>(p)->m->_tx_frame_length; }

// the decoder's lsf (30), lsfFromLich (30), lsfSegmentMap, _m17_decoder_locked
void ref_m17_state(void* p, uint8_t* out62)
{
    Handle* h = static_cast<Handle*>(p);
    static_assert(sizeof(h->m->_m17_decoder.lsf.data) == 30, "the LSF is 30 bytes");
    memcpy(out62, &h->m->_m17_decoder.lsf.data, 30);
    memcpy(out62 + 30, &h->m->_m17_decoder.lsfFromLich.data, 30);
    out62[60] = h->m->_m17_decoder.lsfSegmentMap;
    out62[61] = h->m->_m17_decoder_locked ? 1 : 0;
}

// in: 56 bytes; out: 64 bytes.  0, or -1 when m17FrameInfoReceived's arguments are not what the LSF's accessors give, -2 when a signal fired an
// unexpected number of times
int ref_m17_step(void* p, const uint8_t* in, uint8_t* out)
{
    Handle* h = static_cast<Handle*>(p);
    gr_modem* m = h->m;
    memset(out, 0, 64);
    uint32_t ftype, word1;
    memcpy(&ftype, in, 4); memcpy(&word1, in + 4, 4);
    if ((word1 & 0xFFFFu) != 46u || m->_rx_frame_length != 46) return 0;
    if (ftype != FrameTypeM17LSF && ftype != FrameTypeM17Stream && ftype != FrameTypeM17EOT) return 0;
    M17::M17FrameDecoder& dec = m->_m17_decoder;
    M17::M17LinkSetupFrame before = dec.getLsf();
    M17::M17LinkSetupFrame image = dec.lsfFromLich;
    const unsigned map_before = dec.lsfSegmentMap;
    // the LICH of a stream frame through the decoder's own decodeLich
    bool lich_ok = false, from_lich = false;
    unsigned segment = 0;
    if (ftype == FrameTypeM17Stream) {
        std::array<uint8_t, 46> data;
        memcpy(data.data(), in + 8, 46);
        M17::decorrelate(data);
        M17::deinterleave(data);
        M17::lich_t lich;
        std::copy_n(data.begin(), lich.size(), lich.begin());
        std::array<uint8_t, 6> seg;
        lich_ok = dec.decodeLich(seg, lich);
        if (lich_ok) {
            segment = seg[5];
            if (segment <= 5) memcpy(reinterpret_cast<uint8_t*>(&image.data) + 5 * segment, seg.data(), 5);
            from_lich = (map_before | (1u << segment)) == 0x3Fu && image.valid();
        }
    }
    Events ev;
    g_ev = &ev;
    unsigned char* received = new unsigned char[46];
    memcpy(received, in + 8, 46);
    m->processReceivedData(received, ftype);
    g_ev = nullptr;
    if (ev.info > 1 || ev.audio > 1 || ev.end_audio > 1 || ev.end_audio != ev.receive_end || ev.other) return -2;
    M17::M17LinkSetupFrame after = dec.getLsf();
    // the LSF the reference read its fields from: the decoder's after an LSF or stream frame, the one before an EOT's reset()
    M17::M17LinkSetupFrame read = ftype == FrameTypeM17EOT ? before : after;
    unsigned flags = 0x0001;
    if (after.valid()) flags |= 0x0002;
    if (ev.info) flags |= 0x0004;
    if (ev.audio) flags |= 0x0008;
    if (ev.end_audio) flags |= 0x0010;
    if (lich_ok) flags |= 0x0020;
    if (from_lich) flags |= 0x0040;
    if (m->_m17_decoder_locked) flags |= 0x0080;
    out[0] = (uint8_t)flags; out[1] = (uint8_t)(flags >> 8);
    out[2] = ftype == FrameTypeM17LSF ? 1 : ftype == FrameTypeM17Stream ? 2 : 0xFF;
    if (ftype == FrameTypeM17Stream) {
        M17::M17StreamFrame sf = dec.getStreamFrame();
        const uint16_t fn = sf.getFrameNumber();
        out[4] = (uint8_t)fn; out[5] = (uint8_t)(fn >> 8);
        out[6] = (uint8_t)segment;
    }
    out[7] = dec.lsfSegmentMap;
    if (read.valid()) {
        const std::string src = read.getSource(), dst = read.getDestination();
        const unsigned can = read.getType().fields.CAN;
        if (ev.info && (ev.src != src || ev.dst != dst || ev.can != can)) return -1;
        if (src.size() > 10 || dst.size() > 10) return -2;
        out[3] = (uint8_t)can;
        memcpy(out + 8, read.data.src.data(), 6);
        memcpy(out + 14, read.data.dst.data(), 6);
        put_text(out + 20, src);
        put_text(out + 31, dst);
    } else if (ev.info || ev.audio || ev.end_audio) return -1;
    if (ev.audio) memcpy(out + 48, ev.payload, 16);
    return 0;
}

// ---- transmit
void ref_m17_set_tx(void* p, const char* src, const char* dest, int can_tx, int destination_type)
{
    Handle* h = static_cast<Handle*>(p);
    h->settings.m17_src = QString(src); h->settings.m17_dest = QString(dest);
    h->settings.m17_can_tx = can_tx; h->settings.m17_destination_type = destination_type;
}
void ref_m17_tx_start(void* p) { static_cast<Handle*>(p)->m->startTransmission(QString("")); }
void ref_m17_tx_audio(void* p, const uint8_t* d)
{
    unsigned char* c = new unsigned char[16];
    memcpy(c, d, 16);
    static_cast<Handle*>(p)->m->transmitM17Audio(c, 16);
}
void ref_m17_tx_end(void* p) { static_cast<Handle*>(p)->m->endTransmission(QString("")); }
// the bytes gr_mod_base::set_data received since the last call
size_t ref_m17_tx_take(void* p, uint8_t* buf, size_t cap)
{
    std::vector<unsigned char>& s = static_cast<Handle*>(p)->m->_gr_mod_base->sent;
    const size_t n = s.size() < cap ? s.size() : cap;
    memcpy(buf, s.data(), n);
    s.clear();
    return n;
}

}
