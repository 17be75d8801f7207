// work(int8) / work(uint8) of the C++ facade at 1 Msps (qradiolink_amd/host/gr_modem_hip.*: gr_demod_base_hip::set_iq8_baseband):
//   test_iq8_baseband_work demod <modem_type> <streams> <n> <offset_hz> <scale> <bias> <sc8.bin> <cu8.bin> <out_prefix>
//     sc8.bin / cu8.bin = streams x n interleaved 8-bit I, Q pairs (stream-major), signed and unsigned.  Two gr_demod_base_hip objects at
//     1 Msps with set_iq8_baseband(true), set_sc8_scale(scale) and set_cu8_scale(scale, bias): one is fed sc8.bin through
//     work(const int8_t* const*, n), the other cu8.bin through work(const uint8_t* const*, n), both in calls of 65536 samples with a
//     set_mode() round trip in front of the first one (the setting is forwarded to the re-created handle) and with the spectrum tap on
//     (enable_gui_fft: it reads the uploaded 8-bit slot).  Bits A of every stream go to <out_prefix>.sc8.<s>.bin and <out_prefix>.cu8.<s>.bin;
//     prints "fft_sc8=<frames> fft_cu8=<frames>", the spectrum frames fetched.
//   test_iq8_baseband_work switch
//     a 1 Msps object refuses both 8-bit overloads by default (std::invalid_argument), also under set_sc16_baseband(true); takes them after
//     set_iq8_baseband(true), also across set_mode and through the gr_modem_hip setter, refuses again after set_iq8_baseband(false); and
//     set_iq8_baseband alone does not admit work(int16).  Prints key=value lines.
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
static bool slurp(const char* name, std::vector<unsigned char>& raw)
{
    std::ifstream f(name, std::ios::binary);
    f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)raw.size());
    return static_cast<bool>(f);
}

static int demod(char** argv)
{
    const int mode = atoi(argv[2]), S = atoi(argv[3]);
    const size_t n = (size_t)atoll(argv[4]);
    const int rate = 1000000;
    const double offset = atof(argv[5]);
    const float scale = (float)atof(argv[6]), bias = (float)atof(argv[7]);
    std::vector<unsigned char> raw[2] = {std::vector<unsigned char>((size_t)S * n * 2), std::vector<unsigned char>((size_t)S * n * 2)};
    if (!slurp(argv[8], raw[0]) || !slurp(argv[9], raw[1])) { std::cerr << "short input\n"; return 2; }
    qrl_runtime rt(0);
    const size_t chunk = 65536;
    int frames[2] = {0, 0};
    for (int fmt = 0; fmt < 2; ++fmt) {   // 0: int8 overload, 1: uint8 overload
        gr_demod_base_hip dem(rt, S, rate, offset, chunk);
        dem.set_iq8_baseband(true);                          // before the first handle exists: open() forwards it
        dem.set_sc8_scale(scale);
        dem.set_cu8_scale(scale, bias);
        dem.set_mode(QRL_MODEM_GMSK10K);
        dem.set_mode(mode);                                  // ... and to every re-created one
        dem.set_fft_size(1024);
        dem.enable_gui_fft(true);                            // the spectrum tap beside the demodulator, on the same 8-bit slot
        std::vector<std::vector<unsigned char>> bits((size_t)S);
        std::vector<const int8_t*> ps((size_t)S);
        std::vector<const uint8_t*> pu((size_t)S);
        for (size_t pos = 0; pos < n; pos += chunk) {
            const size_t c = std::min(chunk, n - pos) & ~(size_t)1;
            if (!c) break;
            for (int s = 0; s < S; ++s) {
                pu[(size_t)s] = raw[fmt].data() + 2 * ((size_t)s * n + pos);
                ps[(size_t)s] = reinterpret_cast<const int8_t*>(pu[(size_t)s]);
            }
            if (fmt == 0) dem.work(ps.data(), c); else dem.work(pu.data(), c);
            drain(dem, S, bits);
            std::vector<float> pts(1024);
            unsigned size = 0;
            dem.get_FFT_data(pts.data(), size, 0);
            if (size == 1024) ++frames[fmt];
        }
        dem.flush();
        drain(dem, S, bits);
        {
            std::vector<float> pts(1024);
            unsigned size = 0;
            dem.get_FFT_data(pts.data(), size, 0);
            if (size == 1024) ++frames[fmt];
        }
        for (int s = 0; s < S; ++s) dump(std::string(argv[10]) + (fmt == 0 ? ".sc8." : ".cu8.") + std::to_string(s) + ".bin", bits[(size_t)s]);
    }
    std::cout << "fft_sc8=" << frames[0] << " fft_cu8=" << frames[1] << "\n";
    return 0;
}

template <class T> static int refused(gr_demod_base_hip& dem, const T* p)
{
    try { dem.work(&p, 1024); } catch (const std::invalid_argument&) { return 1; }
    return 0;
}
static int switch_()
{
    qrl_runtime rt(0);
    gr_demod_base_hip dem(rt, 1, 1000000, 0.0, 4096);
    dem.set_mode(QRL_MODEM_GMSK10K);
    std::vector<int8_t> s8(2 * 1024, 40);
    std::vector<uint8_t> u8(2 * 1024, 170);
    std::vector<int16_t> s16(2 * 1024, 100);
    std::vector<gr_complex> x(1024, gr_complex(0.01f, 0.0f));
    const gr_complex* p32 = x.data();
    std::cout << "sc8_refused_by_default=" << refused(dem, s8.data()) << "\n";
    std::cout << "cu8_refused_by_default=" << refused(dem, u8.data()) << "\n";
    dem.set_sc16_baseband(true);
    std::cout << "sc8_refused_under_sc16_baseband=" << refused(dem, s8.data()) << "\n";
    std::cout << "cu8_refused_under_sc16_baseband=" << refused(dem, u8.data()) << "\n";
    dem.set_sc16_baseband(false);
    dem.set_iq8_baseband(true);
    std::cout << "sc8_refused_when_on=" << refused(dem, s8.data()) << "\n";
    std::cout << "cu8_refused_when_on=" << refused(dem, u8.data()) << "\n";
    std::cout << "int16_refused_under_iq8_baseband=" << refused(dem, s16.data()) << "\n";
    dem.set_mode(QRL_MODEM_2FSK1K);
    std::cout << "cu8_refused_after_set_mode=" << refused(dem, u8.data()) << "\n";
    dem.work(&p32, 1024);
    dem.set_iq8_baseband(false);
    std::cout << "sc8_refused_when_off_again=" << refused(dem, s8.data()) << "\n";
    std::cout << "cu8_refused_when_off_again=" << refused(dem, u8.data()) << "\n";
    dem.work(&p32, 1024);
    dem.flush();
    gr_modem_hip modem(&dem, nullptr, gr_modem_events{});
    modem.set_iq8_baseband(true);
    std::cout << "cu8_refused_after_modem_setter=" << refused(dem, u8.data()) << "\n";
    dem.flush();
    std::cout << "done=1\n";
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 11 && !strcmp(argv[1], "demod")) return demod(argv);
        if (argc == 2 && !strcmp(argv[1], "switch")) return switch_();
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    std::cerr << "usage: test_iq8_baseband_work demod <modem> <streams> <n> <offset_hz> <scale> <bias> <sc8.bin> <cu8.bin> <out_prefix> | switch\n";
    return 2;
}
