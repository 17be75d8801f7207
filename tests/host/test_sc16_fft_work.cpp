// The spectrum tap under the int16 work() overload of the C++ facade (qradiolink_amd/host/gr_modem_hip.*):
//   test_sc16_fft_work
//     Two gr_demod_base_hip objects at 2 Msps (GMSK-10k, 2 streams, FFT size 1024) with enable_gui_fft(true): one is fed int16 samples through
//     work(const int16_t* const*, n), the other the floats (float)v * (1 / 32768) through the cf32 work(), in calls of 4096 and 1000 samples (a
//     frame boundary falls inside a call).  After every call both are asked for a spectrum (get_FFT_data); sizes and values of every stream must
//     agree bit for bit.  First with the demodulator valve open, then (new objects) closed.  Prints key=value lines.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>

#include "gr_modem_hip.h"

using namespace qrl_host;

struct result { int threw = 0, frames = 0, equal = 1; };

static result run(qrl_runtime& rt, bool valve_open, const std::vector<int16_t>& raw, const std::vector<gr_complex>& conv, int S, size_t n)
{
    result r;
    const size_t chunk = 4096;
    gr_demod_base_hip d16(rt, S, 2000000, 0.0, chunk), d32(rt, S, 2000000, 0.0, chunk);
    for (gr_demod_base_hip* d : {&d16, &d32}) {
        d->set_mode(QRL_MODEM_GMSK10K);
        d->set_fft_size(1024);
        d->enable_gui_fft(true);
        d->enable_demodulator(valve_open);
    }
    std::vector<const int16_t*> p16((size_t)S);
    std::vector<const gr_complex*> p32((size_t)S);
    std::vector<float> a(1024), b(1024);
    size_t pos = 0;
    for (int call = 0; pos < n; ++call) {
        const size_t c = std::min((call & 1) ? (size_t)1000 : chunk, n - pos) & ~(size_t)1;
        if (!c) break;
        for (int s = 0; s < S; ++s) { p16[(size_t)s] = raw.data() + 2 * ((size_t)s * n + pos); p32[(size_t)s] = conv.data() + (size_t)s * n + pos; }
        try { d16.work(p16.data(), c); } catch (const std::invalid_argument&) { r.threw = 1; return r; }
        d32.work(p32.data(), c);
        pos += c;
        unsigned na = 0, nb = 0;
        d16.get_FFT_data(a.data(), na, 0);
        d32.get_FFT_data(b.data(), nb, 0);
        if (na != nb) { r.equal = 0; continue; }
        if (!na) continue;
        ++r.frames;
        for (int s = 0; s < S; ++s) {
            const float* x = d16.last_FFT_data(s);
            const float* y = d32.last_FFT_data(s);
            if (!x || !y || std::memcmp(x, y, (size_t)na * sizeof(float))) r.equal = 0;
        }
    }
    d16.flush(); d32.flush();
    return r;
}

int main()
{
    try {
        const int S = 2;
        const size_t n = 6 * 4096;
        std::vector<int16_t> raw((size_t)S * n * 2);
        uint32_t lcg = 12345u;
        for (size_t i = 0; i < raw.size(); ++i) { lcg = lcg * 1664525u + 1013904223u; raw[i] = (int16_t)((int32_t)(lcg >> 16) - 32768); }   // the whole int16 range
        raw[0] = -32768; raw[1] = 32767; raw[2] = 0; raw[3] = 1; raw[4] = -1;
        const float scale = 1.0f / 32768.0f;
        std::vector<gr_complex> conv((size_t)S * n);
        for (size_t i = 0; i < conv.size(); ++i) conv[i] = gr_complex((float)raw[2 * i] * scale, (float)raw[2 * i + 1] * scale);
        qrl_runtime rt(0);
        for (int open = 1; open >= 0; --open) {
            const result r = run(rt, open != 0, raw, conv, S, n);
            const char* tag = open ? "open" : "closed";
            std::cout << "threw_" << tag << "=" << r.threw << "\n" << "frames_" << tag << "=" << r.frames << "\n" << "equal_" << tag << "=" << r.equal << "\n";
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
