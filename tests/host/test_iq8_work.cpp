// The 8-bit work() overloads of the C++ facade (qradiolink_amd/host/gr_modem_hip.*) with the spectrum tap on:
//   test_iq8_work demod <modem_type> <streams> <n> <rate> <offset_hz> <iq.bin> <out_prefix>
//     iq.bin = streams x n interleaved int8 I, Q pairs (stream-major).  Three gr_demod_base_hip objects at <rate>, FFT size 1024,
//     enable_gui_fft(true): one is fed the int8 samples through work(const int8_t* const*, n), one the codes u = v + 128 through
//     work(const uint8_t* const*, n) after set_cu8_scale(1 / 128, 128) -- the same samples --, one the floats (float)v * (1 / 128) through the
//     cf32 work(); all in calls of 65536 and 1000 samples.  After every call each is asked for a spectrum (get_FFT_data); sizes and values of
//     every stream must agree bit for bit with the cf32 object's.  Bits A of every stream go to <out_prefix>.sc8.<s>.bin, .cu8.<s>.bin and
//     .cf32.<s>.bin; prints frames=, equal_sc8=, equal_cu8=.
//   test_iq8_work refuse
//     a 1 Msps object refuses both overloads (std::invalid_argument), also under set_sc16_baseband(true), and still takes cf32 samples.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
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
    const int rate = atoi(argv[5]);
    const double offset = atof(argv[6]);
    std::vector<int8_t> raw((size_t)S * n * 2);
    {
        std::ifstream f(argv[7], std::ios::binary);
        f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)raw.size());
        if (!f) { std::cerr << "short input\n"; return 2; }
    }
    const float scale = 1.0f / 128.0f;
    std::vector<uint8_t> rawu(raw.size());
    for (size_t i = 0; i < raw.size(); ++i) rawu[i] = (uint8_t)((int)raw[i] + 128);
    std::vector<gr_complex> conv((size_t)S * n);
    for (size_t i = 0; i < conv.size(); ++i) conv[i] = gr_complex((float)raw[2 * i] * scale, (float)raw[2 * i + 1] * scale);
    qrl_runtime rt(0);
    const size_t chunk = 65536;
    const char* tag[3] = {".sc8.", ".cu8.", ".cf32."};
    std::unique_ptr<gr_demod_base_hip> dem[3];
    std::vector<std::vector<unsigned char>> bits[3];
    for (int k = 0; k < 3; ++k) {
        dem[k].reset(new gr_demod_base_hip(rt, S, rate, offset, chunk));
        if (k == 1) dem[k]->set_cu8_scale(scale, 128.0f);      // before set_mode: open() re-applies it
        dem[k]->set_mode(mode);
        dem[k]->set_fft_size(1024);
        dem[k]->enable_gui_fft(true);
        bits[k].resize((size_t)S);
    }
    std::vector<const int8_t*> p8((size_t)S);
    std::vector<const uint8_t*> pu((size_t)S);
    std::vector<const gr_complex*> p32((size_t)S);
    std::vector<float> buf(1024);
    int frames = 0, equal[2] = {1, 1};
    size_t pos = 0;
    for (int call = 0; pos < n; ++call) {
        const size_t c = std::min((call & 1) ? (size_t)1000 : chunk, n - pos) & ~(size_t)1;
        if (!c) break;
        for (int s = 0; s < S; ++s) {
            p8[(size_t)s] = raw.data() + 2 * ((size_t)s * n + pos); pu[(size_t)s] = rawu.data() + 2 * ((size_t)s * n + pos);
            p32[(size_t)s] = conv.data() + (size_t)s * n + pos;
        }
        dem[0]->work(p8.data(), c);
        dem[1]->work(pu.data(), c);
        dem[2]->work(p32.data(), c);
        pos += c;
        unsigned got[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) { dem[k]->get_FFT_data(buf.data(), got[k], 0); drain(*dem[k], S, bits[k]); }
        for (int k = 0; k < 2; ++k) {
            if (got[k] != got[2]) { equal[k] = 0; continue; }
            for (int s = 0; got[2] && s < S; ++s) {
                const float* x = dem[k]->last_FFT_data(s);
                const float* y = dem[2]->last_FFT_data(s);
                if (!x || !y || std::memcmp(x, y, (size_t)got[2] * sizeof(float))) equal[k] = 0;
            }
        }
        if (got[2]) ++frames;
    }
    for (int k = 0; k < 3; ++k) {
        dem[k]->flush();
        drain(*dem[k], S, bits[k]);
        for (int s = 0; s < S; ++s) dump(std::string(argv[8]) + tag[k] + std::to_string(s) + ".bin", bits[k][(size_t)s]);
    }
    std::cout << "frames=" << frames << "\nequal_sc8=" << equal[0] << "\nequal_cu8=" << equal[1] << "\n";
    return 0;
}

static int refuse()
{
    qrl_runtime rt(0);
    gr_demod_base_hip dem(rt, 1, 1000000, 0.0, 4096);
    dem.set_mode(QRL_MODEM_GMSK10K);
    std::vector<int8_t> raw(2 * 1024, 10);
    std::vector<uint8_t> rawu(2 * 1024, 138);
    std::vector<gr_complex> x(1024, gr_complex(0.01f, 0.0f));
    const int8_t* p8 = raw.data();
    const uint8_t* pu = rawu.data();
    const gr_complex* p32 = x.data();
    int refused = 0;
    for (int baseband = 0; baseband < 2; ++baseband) {
        dem.set_sc16_baseband(baseband != 0);
        try { dem.work(&p8, 1024); } catch (const std::invalid_argument&) { ++refused; }
        try { dem.work(&pu, 1024); } catch (const std::invalid_argument&) { ++refused; }
    }
    std::cout << "refused=" << refused << "\n";
    dem.work(&p32, 1024);
    dem.flush();
    std::cout << "cf32_after=1\n";
    return 0;
}

int main(int argc, char** argv)
{
    try {
        if (argc == 9 && !strcmp(argv[1], "demod")) return demod(argv);
        if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    std::cerr << "usage: test_iq8_work demod <modem> <streams> <n> <rate> <offset_hz> <iq.bin> <out_prefix> | refuse\n";
    return 2;
}
