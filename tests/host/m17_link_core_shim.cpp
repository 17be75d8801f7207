// m17_link_core_shim.cpp — qradiolink_amd/csrc/m17_link_core.hpp behind a C interface for tests/test_m17_link.py and tools/m17_link_ab.py
// (ctypes): the scalar code the kernels call, on the CPU.
#include <cstring>
#include "../../qradiolink_amd/csrc/m17_link_core.hpp"

using namespace qrl::m17;

extern "C" {

int core_m17_sizes(int which)
{
    return which == 0 ? M17_RX_REC : which == 1 ? M17_RX_STATE_SIZE : which == 2 ? M17_RX_STATE_PUBLIC : which == 3 ? M17_FS_REC : which == 4 ? M17_DEC_REC
         : which == 5 ? M17_CALL_BYTES : which == 6 ? M17_START_BYTES : M17_END_BYTES;
}

void core_m17_fresh(uint8_t* state)
{
    const m17_rx_state st = m17_rx_fresh();
    memcpy(state, &st, sizeof st);
}

// n synchroniser records fs [n][56] of one stream with their decode records dec [n][40] -> out [n][64], `reps` times from the given state (the
// single-core figure of docs/MEASUREMENT.md); the state of the last pass is kept
void core_m17_rx_run(int can_rx, int decode_all_can, uint8_t* state, const uint8_t* fs, const uint8_t* dec, size_t n, uint8_t* out, int reps)
{
    const m17_rx_config cfg = {can_rx, decode_all_can};
    m17_rx_state st;
    for (int rep = 0; rep < (reps > 0 ? reps : 1); ++rep) {
        memcpy(&st, state, sizeof st);
        for (size_t i = 0; i < n; ++i) {
            uint32_t head[2], d[M17_DEC_REC / 4], r[M17_RX_REC / 4];
            memcpy(head, fs + i * M17_FS_REC, 8);
            memcpy(d, dec + i * M17_DEC_REC, M17_DEC_REC);
            m17_rx_step(cfg, st, head[0], head[1], d, r);
            memcpy(out + i * M17_RX_REC, r, M17_RX_REC);
        }
    }
    memcpy(state, &st, sizeof st);
}

void core_m17_public(const uint8_t* state, uint8_t* out16)
{
    m17_rx_state st;
    uint32_t w[4];
    memcpy(&st, state, sizeof st);
    m17_rx_public(st, w);
    memcpy(out16, w, 16);
}

// kind 0: the record of the call's LSF frame; 1: of stream frame k with pay16; 2: of the last frame, index k
void core_m17_call_record(int kind, const uint8_t* desc, uint32_t k, const uint8_t* pay16, uint8_t* rec40)
{
    uint32_t lsf[8], rec[M17_DEC_REC / 4], pay[4] = {0, 0, 0, 0};
    call_lsf(desc, lsf);
    if (kind == 0) lsf_record(lsf, rec);
    else {
        if (kind == 1) memcpy(pay, pay16, 16);
        stream_record(lsf, k, pay, kind == 2, rec);
    }
    memcpy(rec40, rec, M17_DEC_REC);
}

}
