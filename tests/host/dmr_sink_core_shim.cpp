// dmr_sink_core_shim.cpp — qradiolink_amd/csrc/dmr_sink_core.hpp and the slot-time helper of qradiolink_amd/host/dmr_frame_hip.h behind a C
// interface for tests/test_dmr_sink.py and tools/dmr_sink_ab.py (ctypes): the scalar code the kernel calls, on the CPU.
#include <cstring>
#include "../../qradiolink_amd/csrc/dmr_sink_core.hpp"
#include "../../qradiolink_amd/csrc/dmr_rx_core.hpp"
#include "../../qradiolink_amd/host/dmr_frame_hip.h"

using namespace qrl::dmr_sink;

extern "C" {

int core_dmr_sink_sizes(int which) { return which == 0 ? FRAME_REC : which == 1 ? INFO_REC : STATE_BYTES; }

// n unpacked bits of one stream through the sink; state: STATE_BYTES bytes, carried.  At most cap records are written; returns the bursts found.
unsigned core_dmr_sink_run(uint8_t* state, const uint8_t* bits, size_t n, uint8_t* frames, uint8_t* info, unsigned cap)
{
    dmr_sink_state st;
    memcpy(&st, state, sizeof st);
    dmr_sink_run run;
    run_load(run, st);
    unsigned nout = 0;
    auto emit = [&](const uint32_t* f, const uint32_t* s) {
        if (nout < cap) {
            for (int k = 0; k < FRAME_REC / 4; ++k) for (int m = 0; m < 4; ++m) frames[(size_t)nout * FRAME_REC + 4 * k + m] = (uint8_t)(f[k] >> (8 * m));
            for (int k = 0; k < INFO_REC / 4; ++k) for (int m = 0; m < 4; ++m) info[(size_t)nout * INFO_REC + 4 * k + m] = (uint8_t)(s[k] >> (8 * m));
        }
        ++nout;
    };
    for (size_t at = 0; at < n; at += 32) {
        const unsigned nbits = n - at < 32 ? (unsigned)(n - at) : 32u;
        uint32_t w = 0;
        for (unsigned i = 0; i < nbits; ++i) w |= (uint32_t)(bits[at + i] & 1u) << (31u - i);
        sink_bits(run, w, nbits, emit);
    }
    run_store(run, st);
    memcpy(state, &st, sizeof st);
    return nout;
}

void core_dmr_sink_flush(uint8_t* state)
{
    dmr_sink_state st;
    memcpy(&st, state, sizeof st);
    ctx_flush(st.c[0]); ctx_flush(st.c[1]);
    memcpy(state, &st, sizeof st);
}

// dmr_slot_time of host/dmr_frame_hip.h; tags as (bit, whole seconds, fraction)
uint64_t core_dmr_slot_time(uint64_t end_bit, const uint64_t* tag_bit, const uint64_t* tag_secs, const double* tag_fracs, size_t ntags)
{
    qrl_host::dmr_time_tag tags[64];
    if (ntags > 64) ntags = 64;
    for (size_t k = 0; k < ntags; ++k) tags[k] = qrl_host::dmr_time_tag{tag_bit[k], qrl_host::dmr_tag_ns(tag_secs[k], tag_fracs[k])};
    return qrl_host::dmr_slot_time(end_bit, tags, ntags);
}
// the call layer in either mode: n frame records [n][40] of one stream and their slot records [n][16] (null: none) -> layer-2 records l2 [n][80]
// -> out [n][128].  state: DMR_RX_STATE_SIZE bytes, carried.
void core_dmr_rxs_run(int color_code, int promiscuous, int repeater, int timeslot, int audio_fec, uint8_t* state, const uint8_t* in,
                      const uint8_t* slots, size_t n, uint8_t* l2, uint8_t* out)
{
    using namespace qrl::dmr;
    const dmr_rx_config cfg = {color_code, promiscuous, repeater, timeslot};
    dmr_rx_state st;
    memcpy(&st, state, sizeof st);
    for (size_t i = 0; i < n; ++i) {
        decode_record(in + i * REC_IN, audio_fec, l2 + i * REC_OUT, true);
        dmr_rx_step_slots_bytes(cfg, st, l2 + i * REC_OUT, slots ? slots + i * SLOT_REC : nullptr, out + i * DMR_RX_REC);
    }
    memcpy(state, &st, sizeof st);
}

// the slot getters of qrl_host::dmr_frame_hip on a layer-2 record and a slot record: downlink, cachDecoded, getSlotNo, getCachLCSS, getAT, the
// three CACH bytes, then endBit as eight bytes, little endian (the slot record's own layout, read back through the class)
void core_dmr_frame_hip_slot(const uint8_t* record80, const uint8_t* slot_info16, uint8_t* out16)
{
    const qrl_host::dmr_frame_hip f(record80, slot_info16);
    out16[0] = f.getDownlink(); out16[1] = f.cachDecoded(); out16[2] = f.getSlotNo(); out16[3] = f.getCachLCSS(); out16[4] = f.getAT();
    f.getCACH(out16 + 5);
    for (int i = 0; i < 8; ++i) out16[8 + i] = (uint8_t)(f.endBit() >> (8 * i));
}

int core_dmr_slot_time_set(const uint8_t* slot_info16) { return qrl_host::dmr_slot_time_set(slot_info16) ? 1 : 0; }

}
