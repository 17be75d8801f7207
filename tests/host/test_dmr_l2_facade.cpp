// DMR layer 2 through the C++ facade (qradiolink_amd/host/gr_modem_hip.*, host/dmr_frame_hip.h):
//   test_dmr_l2_facade <streams> <n> <iq.bin> <out_prefix> <l2: 0 | 1>
//     iq.bin = streams x n complex64 samples at 1 Msps (stream-major).  A gr_demod_base_hip in DMR mode under a gr_modem_hip, fed in calls of 250 000
//     samples, demodulate() after each.  With l2 = 1 set_dmr_l2(true, true) is called first: every burst of the dmrFrames callback must then arrive in the
//     dmrFramesDecoded callback of the same demodulate() as well.  <out_prefix>.raw.<s>.bin holds the 40-byte records of stream s,
//     <out_prefix>.l2.<s>.bin the 80-byte ones, <out_prefix>.get.<s>.bin one line of dmr_frame_hip getters per record.  With l2 = 0 the decoded
//     callback must never fire.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "dmr_frame_hip.h"
#include "gr_modem_hip.h"

using namespace qrl_host;

int main(int argc, char** argv)
{
    if (argc != 6) { std::cerr << "usage: test_dmr_l2_facade <streams> <n> <iq.bin> <out_prefix> <l2>\n"; return 2; }
    try {
        const int S = atoi(argv[1]);
        const size_t n = (size_t)atoll(argv[2]);
        const bool l2 = atoi(argv[5]) != 0;
        std::vector<gr_complex> iq((size_t)S * n);
        {
            std::ifstream f(argv[3], std::ios::binary);
            f.read(reinterpret_cast<char*>(iq.data()), (std::streamsize)(iq.size() * sizeof(gr_complex)));
            if (!f) { std::cerr << "short input\n"; return 2; }
        }
        qrl_runtime rt(0);
        const size_t chunk = 250000;
        gr_demod_base_hip dem(rt, S, 1000000, 0.0, chunk);
        std::vector<std::vector<unsigned char>> raw((size_t)S), dec((size_t)S);
        std::vector<size_t> nraw((size_t)S, 0), ndec((size_t)S, 0);
        gr_modem_events ev;
        ev.dmrFrames = [&](int s, const std::vector<std::vector<unsigned char>>& r) {
            for (auto& x : r) { raw[(size_t)s].insert(raw[(size_t)s].end(), x.begin(), x.end()); ++nraw[(size_t)s]; }
        };
        ev.dmrFramesDecoded = [&](int s, const std::vector<std::vector<unsigned char>>& r) {
            for (auto& x : r) { dec[(size_t)s].insert(dec[(size_t)s].end(), x.begin(), x.end()); ++ndec[(size_t)s]; }
        };
        gr_modem_hip modem(&dem, nullptr, ev);
        if (l2) modem.set_dmr_l2(true, true);
        modem.toggleRxMode(QRL_MODEM_DMR);
        std::vector<const gr_complex*> p((size_t)S);
        auto poll = [&]() {
            for (int s = 0; s < S; ++s) {
                modem.demodulate(s);
                if (l2 && nraw[(size_t)s] != ndec[(size_t)s]) throw std::runtime_error("a burst without its decoded record");
            }
        };
        for (size_t pos = 0; pos < n; pos += chunk) {
            const size_t c = std::min(chunk, n - pos) & ~(size_t)1;
            if (!c) break;
            for (int s = 0; s < S; ++s) p[(size_t)s] = iq.data() + (size_t)s * n + pos;
            dem.work(p.data(), c);
            poll();
        }
        dem.flush();
        poll();
        for (int s = 0; s < S; ++s) {
            if (!l2 && ndec[(size_t)s]) throw std::runtime_error("decoded records although layer 2 is off");
            const std::string pre = std::string(argv[4]);
            std::ofstream(pre + ".raw." + std::to_string(s) + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(raw[(size_t)s].data()), (std::streamsize)raw[(size_t)s].size());
            std::ofstream(pre + ".l2." + std::to_string(s) + ".bin", std::ios::binary).write(reinterpret_cast<const char*>(dec[(size_t)s].data()), (std::streamsize)dec[(size_t)s].size());
            std::ofstream g(pre + ".get." + std::to_string(s) + ".txt");
            for (size_t i = 0; i < ndec[(size_t)s]; ++i) {
                dmr_frame_hip f(dec[(size_t)s].data() + i * QRL_DMR_L2_RECORD_BYTES);
                unsigned char pay[33]; uint8_t len = 0; unsigned char data[33], voice[27] = {};
                f.getDataPayload(pay, len); f.getData(data);
                const bool v = f.getVoice(voice);
                g << (int)f.validate() << " " << (int)f.getDataType() << " " << (int)f.getColorCode() << " " << f.getSrcId() << " " << f.getDstId() << " "
                  << (int)f.getFLCO() << " " << (int)f.getFID() << " " << (int)len << " " << (int)v << " " << (int)data[0] << " " << (int)pay[0] << " " << (int)voice[26] << "\n";
            }
        }
        std::printf("ok %d streams\n", S);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
}
