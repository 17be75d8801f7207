// dmr_rx_core_shim.cpp — qradiolink_amd/csrc/dmr_rx_core.hpp behind a C interface for tests/test_dmr_rx.py and tools/dmr_rx_ab.py (ctypes):
// the scalar code the kernel calls, on the CPU.
#include <cstring>
#include "../../qradiolink_amd/csrc/dmr_rx_core.hpp"

using namespace qrl::dmr;

extern "C" {

int core_dmr_rx_sizes(int which) { return which == 0 ? DMR_RX_REC : which == 1 ? DMR_RX_STATE_SIZE : which == 2 ? DMR_RX_STATE_PUBLIC : TA_MAX; }

// n slicer records [n][40] of one stream -> layer-2 records l2 [n][80] (decode_record, the rate 3/4 search included) -> out [n][128].
// state: DMR_RX_STATE_SIZE bytes, carried.  Returns the largest number of alias bytes the state held after any step.
int core_dmr_rx_run(int color_code, int promiscuous, int audio_fec, uint8_t* state, const uint8_t* in, size_t n, uint8_t* l2, uint8_t* out)
{
    const dmr_rx_config cfg = {color_code, promiscuous};
    dmr_rx_state st;
    memcpy(&st, state, sizeof st);
    int most = st.ta_size;
    for (size_t i = 0; i < n; ++i) {
        decode_record(in + i * REC_IN, audio_fec, l2 + i * REC_OUT, true);
        dmr_rx_step_bytes(cfg, st, l2 + i * REC_OUT, out + i * DMR_RX_REC);
        if (st.ta_size > most) most = st.ta_size;
    }
    memcpy(state, &st, sizeof st);
    return most;
}

// the same from layer-2 records, `reps` times from the given state (the single-core figure of docs/MEASUREMENT.md); the state of the last pass is kept
void core_dmr_rx_run_l2(int color_code, int promiscuous, uint8_t* state, const uint8_t* l2, size_t n, uint8_t* out, int reps)
{
    const dmr_rx_config cfg = {color_code, promiscuous};
    dmr_rx_state st;
    for (int r = 0; r < (reps > 0 ? reps : 1); ++r) {
        memcpy(&st, state, sizeof st);
        for (size_t i = 0; i < n; ++i) dmr_rx_step_bytes(cfg, st, l2 + i * REC_OUT, out + i * DMR_RX_REC);
    }
    memcpy(state, &st, sizeof st);
}

// frag: four fragments, the first embedded bit of each highest; data9: zero unless the decode got as far as the checksum.  Returns embedded_lc_decode's code.
int core_embedded_decode(const uint32_t* frag, uint8_t* data9)
{
    uint32_t d[3] = {0, 0, 0};
    const int code = embedded_lc_decode(frag, d);
    for (unsigned i = 0; i < 9; ++i) data9[i] = (uint8_t)word_byte(d, i);
    return code;
}

}
