// The M17 link layer through the C++ facade (qradiolink_amd/host/gr_modem_hip.*, host/m17_link_hip.h), both directions in one run:
//   test_m17_link_facade <calls.txt> <out_prefix> <link: 0 | 1> <can_rx> <decode_all_can>
//     calls.txt: one line per stream: source destination CAN destination_type frames ("-" = an empty callsign); payload byte j of frame k of stream s
//     is (31 (s + 1) + 7 k + 3 j + 1) & 255.
//     Transmit: a gr_mod_base_hip in M17 mode under a gr_modem_hip; per stream 144 idle bytes, then setM17Call, txM17Audio in two cuts, endM17Call, then idle bytes.  The
//     bytes that reach set_data are tapped into <out_prefix>.tx.<s>.bin; work() turns them into samples.
//     Receive: those samples, scaled, through a gr_demod_base_hip in M17 mode with the device frame synchroniser under a second gr_modem_hip, with
//     set_m17_link(link, can_rx, decode_all_can).  With link = 1 every frame of the m17Frame callback must arrive in the m17LinkEvents callback of
//     the same demodulate(); <out_prefix>.ev.<s>.bin holds the 64-byte records of stream s, .get.<s>.txt one line of m17_link_event_hip getters per
//     record.  With link = 0 the events callback must never fire.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

#include "gr_modem_hip.h"
#include "m17_link_hip.h"

using namespace qrl_host;

static std::string hex(const unsigned char* p, size_t n)
{
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s.empty() ? "-" : s;
}

struct tapped_mod : gr_mod_base_hip {
    using gr_mod_base_hip::gr_mod_base_hip;
    std::vector<std::vector<uint8_t>> seen;
    int set_data(std::vector<uint8_t>* data, int stream) override
    {
        if (seen.size() <= (size_t)stream) seen.resize((size_t)stream + 1);
        seen[(size_t)stream].insert(seen[(size_t)stream].end(), data->begin(), data->end());
        return gr_mod_base_hip::set_data(data, stream);
    }
};

struct call { std::string src, dst; unsigned can, type; size_t n; };

int main(int argc, char** argv)
{
    if (argc != 6) { std::cerr << "usage: test_m17_link_facade <calls.txt> <out_prefix> <link> <can_rx> <decode_all_can>\n"; return 2; }
    try {
        std::vector<call> calls;
        {
            std::ifstream f(argv[1]);
            std::string line;
            while (std::getline(f, line)) {
                std::istringstream is(line);
                call c;
                if (!(is >> c.src >> c.dst >> c.can >> c.type >> c.n)) continue;
                if (c.src == "-") c.src.clear();
                if (c.dst == "-") c.dst.clear();
                calls.push_back(c);
            }
        }
        const int S = (int)calls.size();
        if (S < 1) { std::cerr << "no calls\n"; return 2; }
        const std::string pre = argv[2];
        const bool link = atoi(argv[3]) != 0;
        qrl_runtime rt(0);
        // ---- transmit
        const size_t maxb = 96;
        tapped_mod mod(rt, S, 1000000, 0.0, maxb);
        gr_modem_hip txm(nullptr, &mod, gr_modem_events());
        bool refused = false;
        try { txm.txM17Audio(nullptr, 1, 0); } catch (const std::exception&) { refused = true; }
        if (!refused) throw std::runtime_error("txM17Audio outside M17 mode was taken");
        txm.toggleTxMode(QRL_MODEM_M17);
        refused = false;
        try { uint8_t z[16] = {}; txm.txM17Audio(z, 1, 0); } catch (const std::exception&) { refused = true; }
        if (!refused) throw std::runtime_error("txM17Audio before setM17Call was taken");
        size_t longest = 0;
        const size_t lead = 144;
        for (int s = 0; s < S; ++s) {
            const call& c = calls[(size_t)s];
            const auto desc = m17_call_descriptor(c.src, c.dst, c.can, c.type);
            mod.set_data(new std::vector<uint8_t>(lead, 0), s);   // an idle carrier in front of the call: the receiver's loops settle on it
            txm.setM17Call(desc.data(), s);
            std::vector<uint8_t> pay(c.n * 16);
            for (size_t k = 0; k < c.n; ++k) for (size_t j = 0; j < 16; ++j) pay[16 * k + j] = (uint8_t)(31 * (s + 1) + 7 * k + 3 * j + 1);
            const size_t cut = c.n / 3;
            if (txm.txM17Audio(pay.data(), cut, s) != (int)cut) throw std::runtime_error("txM17Audio: another count");
            if (txm.txM17Audio(pay.data() + 16 * cut, c.n - cut, s) != (int)(c.n - cut)) throw std::runtime_error("txM17Audio: another count");
            txm.endM17Call(s);
            if (mod.seen[(size_t)s].size() != lead + 96 + 48 * c.n + 64) throw std::runtime_error("a call of another length");
            std::ofstream(pre + ".tx." + std::to_string(s) + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(mod.seen[(size_t)s].data() + lead), (std::streamsize)(mod.seen[(size_t)s].size() - lead));
            longest = std::max(longest, mod.seen[(size_t)s].size());
        }
        // idle bytes behind every call: the EOT word opens a 46-byte frame, and every stream is as long as the longest
        for (int s = 0; s < S; ++s) {
            const size_t have = mod.seen[(size_t)s].size(), want = (longest + 96 + 2) / 3 * 3;
            mod.set_data(new std::vector<uint8_t>(want - have, 0), s);
        }
        const size_t total = (longest + 96 + 2) / 3 * 3, spb3 = 2500;   // 2500 samples per 3 bytes
        std::vector<std::vector<gr_complex>> iq((size_t)S);
        std::vector<gr_complex> buf((size_t)S * (maxb / 3 * spb3 + spb3));
        std::vector<gr_complex*> op((size_t)S);
        for (int s = 0; s < S; ++s) op[(size_t)s] = buf.data() + (size_t)s * (maxb / 3 * spb3 + spb3);
        for (size_t sent = 0, guard = 0; sent < total && guard < 1000; ++guard) {
            const size_t n = mod.work(op.data());
            if (!n) break;
            for (int s = 0; s < S; ++s) iq[(size_t)s].insert(iq[(size_t)s].end(), op[(size_t)s], op[(size_t)s] + n);
            sent += n / spb3 * 3;
        }
        if (iq[0].size() < total / 3 * spb3) throw std::runtime_error("the modulator made fewer samples than the bytes ask for");
        for (auto& v : iq) for (auto& x : v) x *= 0.05f;
        // ---- receive
        const size_t chunk = 250000;
        gr_demod_base_hip dem(rt, S, 1000000, 0.0, chunk);
        std::vector<std::vector<unsigned char>> evt((size_t)S);
        std::vector<size_t> nraw((size_t)S, 0), nevt((size_t)S, 0);
        gr_modem_events ev;
        ev.m17Frame = [&](int s, uint64_t, const unsigned char*, int size) { if (size != 46) throw std::runtime_error("an M17 frame of another size"); ++nraw[(size_t)s]; };
        ev.m17LinkEvents = [&](int s, const std::vector<std::vector<unsigned char>>& r) {
            for (auto& x : r) {
                if (x.size() != QRL_M17_RX_RECORD_BYTES) throw std::runtime_error("a link record of another size");
                evt[(size_t)s].insert(evt[(size_t)s].end(), x.begin(), x.end()); ++nevt[(size_t)s];
            }
        };
        gr_modem_hip rxm(&dem, nullptr, ev);
        if (link) {
            refused = false;
            try { rxm.set_m17_link(true, 16, true); } catch (const std::exception&) { refused = true; }
            if (!refused) throw std::runtime_error("CAN 16 was taken");
            rxm.set_m17_link(true, atoi(argv[4]), atoi(argv[5]) != 0);
        }
        rxm.toggleRxMode(QRL_MODEM_M17);
        if (!dem.device_framing()) throw std::runtime_error("the frame synchroniser is not on the device");
        auto poll = [&]() {
            for (int s = 0; s < S; ++s) {
                rxm.demodulate(s);
                if (link && nraw[(size_t)s] != nevt[(size_t)s]) throw std::runtime_error("a frame without its link record");
            }
        };
        const size_t n = iq[0].size();
        std::vector<const gr_complex*> p((size_t)S);
        for (size_t pos = 0; pos < n; pos += chunk) {
            const size_t c = std::min(chunk, n - pos) & ~(size_t)1;
            if (!c) break;
            for (int s = 0; s < S; ++s) p[(size_t)s] = iq[(size_t)s].data() + pos;
            dem.work(p.data(), c);
            poll();
        }
        dem.flush();
        poll();
        for (int s = 0; s < S; ++s) {
            if (!link && nevt[(size_t)s]) throw std::runtime_error("link records although the link layer is off");
            std::ofstream(pre + ".ev." + std::to_string(s) + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(evt[(size_t)s].data()), (std::streamsize)evt[(size_t)s].size());
            std::ofstream g(pre + ".get." + std::to_string(s) + ".txt");
            for (size_t i = 0; i < nevt[(size_t)s]; ++i) {
                m17_link_event_hip e(evt[(size_t)s].data() + i * QRL_M17_RX_RECORD_BYTES);
                const auto es = e.encodedSource(), ed = e.encodedDestination();
                g << (int)e.frame() << " " << (int)e.lsfValid() << " " << (int)e.frameInfoReceived() << " " << (int)e.digitalAudio() << " " << (int)e.endAudioTransmission() << " "
                  << (int)e.lichDecoded() << " " << (int)e.lsfFromLich() << " " << (int)e.locked() << " " << e.frameType() << " " << e.CAN() << " " << e.frameNumber() << " "
                  << (int)e.isLastFrame() << " " << e.lichSegment() << " " << e.segmentMap() << " " << hex(es.data(), 6) << " " << hex(ed.data(), 6) << " "
                  << (e.source().empty() ? "-" : e.source()) << " " << (e.destination().empty() ? "-" : e.destination()) << " " << hex(e.payload(), 16) << "\n";
            }
        }
        std::printf("ok %d streams, frames", S);
        for (int s = 0; s < S; ++s) std::printf(" %zu", nraw[(size_t)s]);
        std::printf("\n");
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
}
