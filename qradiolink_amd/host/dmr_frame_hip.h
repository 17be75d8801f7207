// dmr_frame_hip.h — an 80-byte record of qrl_dmr_l2_decode (include/qrl_hip.h) behind the getters of the reference's DMRFrame
// (src/DMR/dmrframe.h:50-88) as they read after DMRFrame(bytes, type), validate() and runAudioFEC(): what DMRControl::addFrames /
// processAudio (src/DMR/dmrcontrol.cpp:225-260, :625-700) look at.  The work is done on the device; this class only reads bytes.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "qrl_hip.h"

namespace qrl_host {

class dmr_frame_hip {
public:
    explicit dmr_frame_hip(const unsigned char* record80) { std::memcpy(_r, record80, QRL_DMR_L2_RECORD_BYTES); }
    explicit dmr_frame_hip(const std::vector<unsigned char>& record80) { std::memcpy(_r, record80.data(), QRL_DMR_L2_RECORD_BYTES); }
    bool validate() const { return _r[4] != 0; }
    uint8_t getFrameType() const { return _r[0]; }
    uint8_t getFN() const { return _r[1]; }
    uint8_t getColorCode() const { return _r[2]; }
    uint8_t getDataType() const { return _r[3]; }               // 0..15, QRL_DMR_DT_VOICE_SYNC, QRL_DMR_DT_VOICE
    int audioErrors() const { return _r[5]; }                   // what runAudioFEC() returned
    bool getPI() const { return _r[6] != 0; }                   // CDMREMB of voice frames B..F
    uint8_t getLCSS() const { return _r[7]; }
    uint8_t getFLCO() const { return _r[9]; }
    uint8_t getFID() const { return _r[10]; }
    uint32_t getSrcId() const { return le32(12); }
    uint32_t getDstId() const { return le32(16); }
    void getData(unsigned char* data) const { std::memcpy(data, _r + 20, 33); }
    bool getVoice(unsigned char* data) const
    {
        if (_r[0] != 1 && _r[0] != 2) return false;
        std::memcpy(data, _r + 53, 27);
        return true;
    }
    // the decoded payload: 12 bytes of a BPTC burst, 18 of a rate 3/4 burst, 27 of a voice burst; length 0 for a refused or rate 1 burst
    void getDataPayload(unsigned char* data, uint8_t& length) const { length = _r[8]; std::memcpy(data, _r + 53, length); }

private:
    uint32_t le32(int o) const { return (uint32_t)_r[o] | ((uint32_t)_r[o + 1] << 8) | ((uint32_t)_r[o + 2] << 16) | ((uint32_t)_r[o + 3] << 24); }
    unsigned char _r[QRL_DMR_L2_RECORD_BYTES];
};

}  // namespace qrl_host
