// Stand-in for src/settings.h in front of tests/host/dmr_ctl_stub's on the include path of tests/host/dmr_sink_ref.cpp: the dmr_* fields
// DMRControl reads, and the one more DMRTiming reads
#pragma once
#include <cstdint>
#include <QString>
class Settings {
public:
    int dmr_call_type = 0;            // DMR_CALL_TYPE: 0 group, 1 private
    uint32_t dmr_source_id = 0, dmr_destination_id = 0;
    int dmr_vocoder = 1;              // 0: Codec2 voice, FID 0xC2
    QString dmr_talker_alias;
    int dmr_color_code = 1, dmr_timeslot = 1, dmr_mode = 0;   // DMR_MODE: 0 repeater, 1 DMO
    bool dmr_promiscuous_mode = false;
    int dmr_timing_correction = 0;    // samples; DMRTiming::get_slot_times
};
