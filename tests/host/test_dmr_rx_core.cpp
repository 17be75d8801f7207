// test_dmr_rx_core.cpp — qradiolink_amd/csrc/dmr_rx_core.hpp on the CPU (tests/test_dmr_rx.py builds this with the address and
// undefined-behaviour sanitizers): every scenario of a flat binary file (what the test writes from tests/golden/ref/dmr_rx.npz) through
// decode_record and dmr_rx_step, byte for byte against the reference's records; once in one piece and once with the state carried through a
// copy after every burst, as a call boundary does.  The alias buffer must never hold more than TA_MAX bytes.
//   file: uint32 s | s x { uint32 n | int32 colour code | int32 promiscuous | n x 40 slicer records | n x 128 expected records }
//   test_dmr_rx_core FILE     compare, print "ok <s> scenarios, <bursts> bursts"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../qradiolink_amd/csrc/dmr_rx_core.hpp"

using namespace qrl::dmr;

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t s = 0;
    if (fread(&s, 4, 1, f) != 1 || s > (1u << 16)) { fprintf(stderr, "bad header\n"); return 2; }
    unsigned bad = 0, total = 0;
    for (uint32_t k = 0; k < s; ++k) {
        uint32_t n = 0;
        int32_t cc = 0, prom = 0;
        if (fread(&n, 4, 1, f) != 1 || fread(&cc, 4, 1, f) != 1 || fread(&prom, 4, 1, f) != 1 || n > (1u << 20)) { fprintf(stderr, "short file\n"); return 2; }
        std::vector<uint8_t> in((size_t)n * REC_IN), want((size_t)n * DMR_RX_REC);
        if ((n && fread(in.data(), 1, in.size(), f) != in.size()) || (n && fread(want.data(), 1, want.size(), f) != want.size())) {
            fprintf(stderr, "short file\n");
            return 2;
        }
        const dmr_rx_config cfg = {cc, prom};
        for (int pass = 0; pass < 2; ++pass) {
            dmr_rx_state* st = static_cast<dmr_rx_state*>(calloc(1, sizeof(dmr_rx_state)));
            for (uint32_t i = 0; i < n; ++i) {
                uint8_t l2[REC_OUT], out[DMR_RX_REC];
                decode_record(&in[(size_t)i * REC_IN], 1, l2, true);
                dmr_rx_step_bytes(cfg, *st, l2, out);
                if (st->ta_size > TA_MAX) { fprintf(stderr, "scenario %u burst %u: %u alias bytes\n", k, i, st->ta_size); ++bad; }
                if (memcmp(out, &want[(size_t)i * DMR_RX_REC], DMR_RX_REC)) {
                    if (bad++ < 8) {
                        int j = 0;
                        while (out[j] == want[(size_t)i * DMR_RX_REC + j]) ++j;
                        fprintf(stderr, "scenario %u burst %u pass %d: byte %d is %u, the reference has %u\n", k, i, pass, j, out[j], want[(size_t)i * DMR_RX_REC + j]);
                    }
                }
                if (pass) {   // a call boundary: the state goes through memory of its own size and back
                    dmr_rx_state* next = static_cast<dmr_rx_state*>(malloc(sizeof(dmr_rx_state)));
                    memcpy(next, st, sizeof(dmr_rx_state));
                    free(st);
                    st = next;
                }
            }
            free(st);
        }
        total += n;
    }
    fclose(f);
    if (bad) { fprintf(stderr, "%u differences\n", bad); return 1; }
    printf("ok %u scenarios, %u bursts\n", s, total);
    return 0;
}
