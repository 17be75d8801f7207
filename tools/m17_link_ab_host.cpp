// m17_link_ab_host.cpp — the host path the M17 link layer replaces, timed for tools/m17_link_ab.py: m17_frame_decoder_hip::decodeFrames
// (host/m17_frame_decoder_hip.cpp: a copy up, qrl_m17_decode_frames, a blocking copy down, the scalar LICH reassembly per record) over a
// file of frames.  Usage: m17_link_ab_host FRAMES STREAMS SLOTS WARMUP STEPS -- FRAMES holds [STREAMS][SLOTS][48] bytes; prints the
// wall-clock milliseconds of every timed decodeFrames call over all of them, one line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "m17_frame_decoder_hip.h"

int main(int argc, char** argv)
{
    if (argc != 6) { std::fprintf(stderr, "usage: %s frames streams slots warmup steps\n", argv[0]); return 2; }
    const size_t streams = (size_t)std::atol(argv[2]), slots = (size_t)std::atol(argv[3]);
    const int warmup = std::atoi(argv[4]), steps = std::atoi(argv[5]);
    const size_t n = streams * slots;
    std::vector<uint8_t> frames(n * 48);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(frames.data(), 1, frames.size(), f) != frames.size()) { std::fprintf(stderr, "cannot read %zu bytes of %s\n", frames.size(), argv[1]); return 2; }
    std::fclose(f);
    std::vector<int> stream_of(n);
    for (size_t i = 0; i < n; ++i) stream_of[i] = (int)(i / slots);
    qrl_runtime rt(0);
    qrl_host::m17_frame_decoder_hip dec(rt, (int)streams, n);
    for (int k = 0; k < warmup + steps; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        const auto types = dec.decodeFrames(frames.data(), stream_of.data(), n);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (types.size() != n) return 1;
        if (k >= warmup) std::printf("%.4f%c", ms, k + 1 == warmup + steps ? '\n' : ' ');
    }
    return 0;
}
