// DMR layer 2 transmit through the C++ facade (qradiolink_amd/host/gr_modem_hip.*, host/dmr_frame_hip.h):
//   test_dmr_tx_facade <calls.bin> <out_prefix> <max_bytes>
//     calls.bin = uint32 S | uint32 nv | per stream: 40-byte descriptor, nv x 27 codec bytes, (2 + nv + 1) x 33 bursts (the call's LC header
//     twice, its nv voice bursts, its terminator: the reference's recorded frames).  Two gr_mod_base_hip in DMR mode of S streams each, passes
//     of max_bytes bytes:
//       call   setDMRData(the two headers), setDMRCall, txDMRVoice in two cuts (5 bursts, the rest), setDMRData(the terminator)
//       data   setDMRData(every recorded burst)
//     <out_prefix>.call.<s>.bin / .data.<s>.bin hold the complex64 samples of stream s.  The descriptor and the LC header are also written
//     with the writers of host/dmr_frame_hip.h: the descriptor must equal the file's, the header record, through qrl_dmr_l2_encode, the
//     recorded header burst.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime.h>

#include "dmr_frame_hip.h"
#include "gr_modem_hip.h"

using namespace qrl_host;

struct call_in { std::vector<uint8_t> desc, voice; std::vector<std::vector<uint8_t>> frames; };

static void run(gr_mod_base_hip& mod, int S, size_t max_bytes, const std::string& pre, const char* name)
{
    const size_t cap = (max_bytes / 3 + 1) * 2500;
    std::vector<std::vector<gr_complex>> buf((size_t)S, std::vector<gr_complex>(cap)), all((size_t)S);
    std::vector<gr_complex*> p((size_t)S);
    for (int s = 0; s < S; ++s) p[(size_t)s] = buf[(size_t)s].data();
    for (;;) {
        const size_t n = mod.work(p.data());
        if (!n) break;
        for (int s = 0; s < S; ++s) all[(size_t)s].insert(all[(size_t)s].end(), buf[(size_t)s].begin(), buf[(size_t)s].begin() + (std::ptrdiff_t)n);
    }
    for (int s = 0; s < S; ++s)
        std::ofstream(pre + "." + name + "." + std::to_string(s) + ".bin", std::ios::binary)
            .write(reinterpret_cast<const char*>(all[(size_t)s].data()), (std::streamsize)(all[(size_t)s].size() * sizeof(gr_complex)));
}

int main(int argc, char** argv)
{
    if (argc != 4) { std::cerr << "usage: test_dmr_tx_facade <calls.bin> <out_prefix> <max_bytes>\n"; return 2; }
    try {
        std::ifstream f(argv[1], std::ios::binary);
        uint32_t S = 0, nv = 0;
        f.read(reinterpret_cast<char*>(&S), 4); f.read(reinterpret_cast<char*>(&nv), 4);
        if (!f || S == 0 || S > 64 || nv < 6 || nv > 4096) { std::cerr << "bad header\n"; return 2; }
        std::vector<call_in> calls(S);
        for (auto& c : calls) {
            c.desc.resize(QRL_DMR_CALL_BYTES); c.voice.resize(27 * (size_t)nv);
            f.read(reinterpret_cast<char*>(c.desc.data()), (std::streamsize)c.desc.size());
            f.read(reinterpret_cast<char*>(c.voice.data()), (std::streamsize)c.voice.size());
            c.frames.assign(2 + (size_t)nv + 1, std::vector<uint8_t>(33));
            for (auto& fr : c.frames) f.read(reinterpret_cast<char*>(fr.data()), 33);
        }
        if (!f) { std::cerr << "short input\n"; return 2; }
        const size_t max_bytes = (size_t)atoll(argv[3]);
        const std::string pre = argv[2];
        qrl_runtime rt(0);
        {   // the writers of host/dmr_frame_hip.h
            uint8_t *d_rec = nullptr, *d_out = nullptr;
            if (hipMalloc(reinterpret_cast<void**>(&d_rec), QRL_DMR_TX_RECORD_BYTES) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&d_out), 36) != hipSuccess)
                throw std::runtime_error("hipMalloc");
            for (const auto& c : calls) {
                const uint8_t* d = c.desc.data();
                const uint32_t src = (uint32_t)d[0] << 16 | (uint32_t)d[1] << 8 | d[2], dst = (uint32_t)d[3] << 16 | (uint32_t)d[4] << 8 | d[5];
                dmr_call_descriptor mine(src, dst, d[6] == 0, d[7] == 0xC2, d[8], std::vector<unsigned char>(d + 9, d + 36));
                if (std::memcmp(mine.data(), d, QRL_DMR_CALL_BYTES)) throw std::runtime_error("dmr_call_descriptor differs from the recorded descriptor");
                dmr_tx_record rec;
                rec.setColorCode(d[8]).setLC(d[6], d[7], 0, src, dst).lcFrame(1);
                uint8_t burst[33];
                if (hipMemcpy(d_rec, rec.data(), QRL_DMR_TX_RECORD_BYTES, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
                if (qrl_dmr_l2_encode(rt.ctx(), nullptr, d_rec, nullptr, 1, 1, d_out, 36, 36) != QRL_OK) throw std::runtime_error(qrl_last_error());
                if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(burst, d_out, 33, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy");
                if (std::memcmp(burst, c.frames[0].data(), 33)) throw std::runtime_error("dmr_tx_record's LC header differs from the recorded burst");
            }
            (void)hipFree(d_rec); (void)hipFree(d_out);
        }
        {
            gr_mod_base_hip mod(rt, (int)S, 1000000, 0.0, max_bytes);
            mod.set_mode(QRL_MODEM_DMR);
            for (uint32_t s = 0; s < S; ++s) {
                const auto& c = calls[s];
                mod.setDMRData({c.frames[0], c.frames[1]}, (int)s);
                mod.setDMRCall(c.desc.data(), (int)s);
                if (mod.txDMRVoice(c.voice.data(), 5, (int)s) != 5) throw std::runtime_error("txDMRVoice");
                if (mod.txDMRVoice(c.voice.data() + 27 * 5, nv - 5, (int)s) != (int)nv - 5) throw std::runtime_error("txDMRVoice");
                mod.setDMRData({c.frames[2 + nv]}, (int)s);
            }
            run(mod, (int)S, max_bytes, pre, "call");
        }
        {
            gr_mod_base_hip mod(rt, (int)S, 1000000, 0.0, max_bytes);
            mod.set_mode(QRL_MODEM_DMR);
            for (uint32_t s = 0; s < S; ++s) mod.setDMRData(calls[s].frames, (int)s);
            run(mod, (int)S, max_bytes, pre, "data");
        }
        std::printf("ok %u streams\n", S);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
}
