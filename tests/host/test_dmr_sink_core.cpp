// test_dmr_sink_core.cpp — qradiolink_amd/csrc/dmr_sink_core.hpp on the CPU, for a build with -fsanitize=address,undefined
// (tests/test_dmr_sink.py): every scenario of a flat file made from tests/golden/ref/dmr_sink.npz, call by call with its flushes and
// resets, must give the recorded frame and slot records and burst counts.
// File: u32 scenarios; per scenario u32 nbits, u32 ncalls, u32 cap, u32 nrecords, then ncalls x {u32 size, u32 op, u32 found}, the bits
// (one per byte), nrecords x 40 frame bytes, nrecords x 16 slot bytes (the records a mailbox of cap holds, in order).
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../qradiolink_amd/csrc/dmr_sink_core.hpp"

using namespace qrl::dmr_sink;

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s golden.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t scenarios = 0;
    if (!rd(f, &scenarios, 4)) return 2;
    size_t bursts = 0;
    for (uint32_t s = 0; s < scenarios; ++s) {
        uint32_t head[4];
        if (!rd(f, head, 16)) return 2;
        const uint32_t nbits = head[0], ncalls = head[1], cap = head[2], nrec = head[3];
        std::vector<uint32_t> calls(3 * (size_t)ncalls);
        std::vector<uint8_t> bits(nbits), want_f((size_t)nrec * FRAME_REC), want_i((size_t)nrec * INFO_REC);
        if (!rd(f, calls.data(), 12 * (size_t)ncalls) || !rd(f, bits.data(), nbits) || !rd(f, want_f.data(), want_f.size()) || !rd(f, want_i.data(), want_i.size())) return 2;
        dmr_sink_state st;
        memset(&st, 0, sizeof st);
        // exactly cap records per call, so that a write past the mailbox is a heap overflow
        size_t at = 0, rec = 0;
        for (uint32_t c = 0; c < ncalls; ++c) {
            const uint32_t size = calls[3 * c], op = calls[3 * c + 1], found = calls[3 * c + 2];
            if (op == 1) { ctx_flush(st.c[0]); ctx_flush(st.c[1]); }
            if (op == 2) memset(&st, 0, sizeof st);
            std::vector<uint8_t> frames((size_t)cap * FRAME_REC), info((size_t)cap * INFO_REC);
            std::vector<uint8_t> in(bits.begin() + (long)at, bits.begin() + (long)(at + size));
            dmr_sink_run run;
            run_load(run, st);
            uint32_t nout = 0;
            auto emit = [&](const uint32_t* fr, const uint32_t* sl) {
                if (nout < cap) {
                    for (int k = 0; k < FRAME_REC; ++k) frames[(size_t)nout * FRAME_REC + k] = (uint8_t)(fr[k / 4] >> (8 * (k % 4)));
                    for (int k = 0; k < INFO_REC; ++k) info[(size_t)nout * INFO_REC + k] = (uint8_t)(sl[k / 4] >> (8 * (k % 4)));
                }
                ++nout;
            };
            for (size_t p = 0; p < size; p += 32) {
                const unsigned nb = size - p < 32 ? (unsigned)(size - p) : 32u;
                uint32_t w = 0;
                for (unsigned i = 0; i < nb; ++i) w |= (uint32_t)(in[p + i] & 1u) << (31u - i);
                sink_bits(run, w, nb, emit);
            }
            run_store(run, st);
            at += size;
            if (nout != found) { printf("scenario %u call %u: %u bursts, the reference %u\n", s, c, nout, found); return 1; }
            const uint32_t w = nout < cap ? nout : cap;
            if (rec + w > nrec || memcmp(frames.data(), want_f.data() + rec * FRAME_REC, (size_t)w * FRAME_REC) ||
                memcmp(info.data(), want_i.data() + rec * INFO_REC, (size_t)w * INFO_REC)) { printf("scenario %u call %u: records differ\n", s, c); return 1; }
            rec += w; bursts += w;
        }
        if (rec != nrec) { printf("scenario %u: %zu records, the reference %u\n", s, rec, nrec); return 1; }
    }
    fclose(f);
    printf("ok %u scenarios, %zu bursts\n", scenarios, bursts);
    return 0;
}
