// work(int16) of the C++ facade at 1 Msps (qradiolink_amd/host/gr_modem_hip.*: gr_demod_base_hip::set_sc16_baseband):
//   test_sc16_baseband_work demod <modem_type> <streams> <n> <offset_hz> <iq.bin> <out_prefix>
//     iq.bin = streams x n interleaved int16 I, Q pairs (stream-major).  Two gr_demod_base_hip objects at 1 Msps: one has
//     set_sc16_baseband(true) and is fed the int16 samples through work(const int16_t* const*, n), the other is fed the floats
//     (float)v * (1 / 32768) through the cf32 work(); both in calls of 65536 samples, with a set_mode() round trip in front of the
//     first one (the setting is forwarded to the re-created handle).  Bits A of every stream go to <out_prefix>.sc16.<s>.bin and
//     <out_prefix>.cf32.<s>.bin.
//   test_sc16_baseband_work switch
//     a 1 Msps object refuses work(int16) by default (std::invalid_argument), takes it after set_sc16_baseband(true), also through the
//     gr_modem_hip setter and across set_mode, and refuses again after set_sc16_baseband(false).  Prints key=value lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "gr_modem_hip.h"

using namespace qrl_host;

static void drain(gr_demod_base_hip& dem, int S, std::vector<std::vector<unsigned char>>& bits)
{
    for (int s = 0; s < S; ++s)
        if (std::vector<unsigned char>* v = dem.getData(1, s)) { bits[(size_t)s].insert(bits[(size_t)s].end(), v->begin(), v->end()); delete v; }
}
static void dump(const std::string& name, const std::vector<unsigned char>& v)
{
    std::ofstream o(name, std::ios::binary);
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)v.size());
}

static int demod(char** argv)
{
    const int mode = atoi(argv[2]), S = atoi(argv[3]);
    const size_t n = (size_t)atoll(argv[4]);
    const int rate = 1000000;
    const double offset = atof(argv[5]);
    std::vector<int16_t> raw((size_t)S * n * 2);
    {
        std::ifstream f(argv[6], std::ios::binary);
        f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)(raw.size() * sizeof(int16_t)));
        if (!f) { std::cerr << "short input\n"; return 2; }
    }
    const float scale = 1.0f / 32768.0f;
    std::vector<gr_complex> conv((size_t)S * n);
    for (size_t i = 0; i < conv.size(); ++i) conv[i] = gr_complex((float)raw[2 * i] * scale, (float)raw[2 * i + 1] * scale);
    qrl_runtime rt(0);
    const size_t chunk = 65536;
    for (int fmt = 0; fmt < 2; ++fmt) {   // 0: int16 overload, 1: cf32
        gr_demod_base_hip dem(rt, S, rate, offset, chunk);
        if (fmt == 0) dem.set_sc16_baseband(true);          // before the first handle exists: open() forwards it
        dem.set_mode(QRL_MODEM_GMSK10K);
        dem.set_mode(mode);                                  // ... and to every re-created one
        std::vector<std::vector<unsigned char>> bits((size_t)S);
        std::vector<const int16_t*> p16((size_t)S);
        std::vector<const gr_complex*> p32((size_t)S);
        for (size_t pos = 0; pos < n; pos += chunk) {
            const size_t c = std::min(chunk, n - pos) & ~(size_t)1;
            if (!c) break;
            for (int s = 0; s < S; ++s) { p16[(size_t)s] = raw.data() + 2 * ((size_t)s * n + pos); p32[(size_t)s] = conv.data() + (size_t)s * n + pos; }
            if (fmt == 0) dem.work(p16.data(), c); else dem.work(p32.data(), c);
            drain(dem, S, bits);
        }
        dem.flush();
        drain(dem, S, bits);
        for (int s = 0; s < S; ++s) dump(std::string(argv[7]) + (fmt == 0 ? ".sc16." : ".cf32.") + std::to_string(s) + ".bin", bits[(size_t)s]);
    }
    return 0;
}

static int refused(gr_demod_base_hip& dem, const int16_t* p16)
{
    try { dem.work(&p16, 1024); } catch (const std::invalid_argument&) { return 1; }
    return 0;
}
static int switch_()
{
    qrl_runtime rt(0);
    gr_demod_base_hip dem(rt, 1, 1000000, 0.0, 4096);
    dem.set_mode(QRL_MODEM_GMSK10K);
    std::vector<int16_t> raw(2 * 1024, 100);
    std::vector<gr_complex> x(1024, gr_complex(0.01f, 0.0f));
    const gr_complex* p32 = x.data();
    std::cout << "refused_by_default=" << refused(dem, raw.data()) << "\n";
    dem.set_sc16_baseband(true);
    std::cout << "refused_when_on=" << refused(dem, raw.data()) << "\n";
    dem.set_mode(QRL_MODEM_2FSK1K);
    std::cout << "refused_after_set_mode=" << refused(dem, raw.data()) << "\n";
    dem.work(&p32, 1024);
    dem.set_sc16_baseband(false);
    std::cout << "refused_when_off_again=" << refused(dem, raw.data()) << "\n";
    dem.work(&p32, 1024);
    dem.flush();
    gr_modem_hip modem(&dem, nullptr, gr_modem_events{});
    modem.set_sc16_baseband(true);
    std::cout << "refused_after_modem_setter=" << refused(dem, raw.data()) << "\n";
    dem.flush();
    std::cout << "done=1\n";
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 8 && !strcmp(argv[1], "demod")) return demod(argv);
        if (argc == 2 && !strcmp(argv[1], "switch")) return switch_();
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    std::cerr << "usage: test_sc16_baseband_work demod <modem> <streams> <n> <offset_hz> <iq.bin> <out_prefix> | switch\n";
    return 2;
}
