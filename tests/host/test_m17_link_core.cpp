// test_m17_link_core.cpp — qradiolink_amd/csrc/m17_link_core.hpp on the CPU, a program of its own for the address and undefined-behaviour
// sanitizers (tests/test_m17_link.py builds and runs it).  Input: a flat file of the golden's scenarios that keep one configuration
//   u32 scenarios; per scenario: u32 frames, i32 can_rx, i32 decode_all_can, frames x 56 synchroniser records, frames x 40 decode records,
//   frames x 64 expected records
// then u32 calls; per call: 32 descriptor bytes, u32 k, 16 payload bytes, i32 kind, 40 expected record bytes.
// Every scenario runs whole and in calls of one frame with the state carried through its 64 bytes.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../qradiolink_amd/csrc/m17_link_core.hpp"

using namespace qrl::m17;

static bool rd(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t scenarios = 0, total = 0;
    if (!rd(f, &scenarios, 4)) return 2;
    for (uint32_t s = 0; s < scenarios; ++s) {
        uint32_t n; int32_t cfg2[2];
        if (!rd(f, &n, 4) || !rd(f, cfg2, 8)) return 2;
        std::vector<uint8_t> fs((size_t)n * M17_FS_REC), dec((size_t)n * M17_DEC_REC), want((size_t)n * M17_RX_REC);
        if (!rd(f, fs.data(), fs.size()) || !rd(f, dec.data(), dec.size()) || !rd(f, want.data(), want.size())) return 2;
        const m17_rx_config cfg = {cfg2[0], cfg2[1]};
        uint8_t carried[M17_RX_STATE_SIZE];
        const m17_rx_state fresh = m17_rx_fresh();
        std::memcpy(carried, &fresh, sizeof fresh);
        m17_rx_state whole = m17_rx_fresh();
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t head[2], d[M17_DEC_REC / 4], r[M17_RX_REC / 4], r2[M17_RX_REC / 4];
            std::memcpy(head, fs.data() + (size_t)i * M17_FS_REC, 8);
            std::memcpy(d, dec.data() + (size_t)i * M17_DEC_REC, M17_DEC_REC);
            m17_rx_step(cfg, whole, head[0], head[1], d, r);
            m17_rx_state st;
            std::memcpy(&st, carried, sizeof st);
            m17_rx_step(cfg, st, head[0], head[1], d, r2);
            std::memcpy(carried, &st, sizeof st);
            if (std::memcmp(r, want.data() + (size_t)i * M17_RX_REC, M17_RX_REC) || std::memcmp(r, r2, M17_RX_REC) || std::memcmp(&whole, carried, sizeof whole)) {
                std::printf("scenario %u frame %u differs\n", s, i);
                return 1;
            }
            uint32_t pub[4];
            m17_rx_public(whole, pub);
        }
        total += n;
    }
    uint32_t calls = 0;
    if (!rd(f, &calls, 4)) return 2;
    for (uint32_t c = 0; c < calls; ++c) {
        uint8_t desc[M17_CALL_BYTES], pay8[16], want[M17_DEC_REC];
        uint32_t k; int32_t kind;
        if (!rd(f, desc, sizeof desc) || !rd(f, &k, 4) || !rd(f, pay8, 16) || !rd(f, &kind, 4) || !rd(f, want, sizeof want)) return 2;
        uint32_t lsf[8], rec[M17_DEC_REC / 4], pay[4];
        std::memcpy(pay, pay8, 16);
        call_lsf(desc, lsf);
        if (kind == 0) lsf_record(lsf, rec); else stream_record(lsf, k, pay, kind == 2, rec);
        if (std::memcmp(rec, want, M17_DEC_REC)) { std::printf("call record %u differs\n", c); return 1; }
    }
    std::fclose(f);
    std::printf("ok %u scenarios, %u frames, %u call records\n", scenarios, total, calls);
    return 0;
}
