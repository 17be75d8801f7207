// dmr_frame_hip.h — an 80-byte record of qrl_dmr_l2_decode (include/qrl_hip.h) behind the getters of the reference's DMRFrame
// (src/DMR/dmrframe.h:50-88) as they read after DMRFrame(bytes, type), validate() and runAudioFEC(): what DMRControl::addFrames /
// processAudio (src/DMR/dmrcontrol.cpp:225-260, :625-700) look at.  The work is done on the device; this class only reads bytes.
// Below it the transmit side: dmr_tx_record and dmr_call_descriptor write the two records of qrl_dmr_l2_encode / qrl_dmr_voice_call_encode.
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

// ---- the transmit side: writers of the two records of qrl_dmr_l2_encode / qrl_dmr_voice_call_encode (include/qrl_hip.h) ----
// A 48-byte TX record: what DMRFrame(type) and its setters / constructLCFrame / constructCSBKFrame take in the reference (src/DMR/dmrframe.h).
class dmr_tx_record {
public:
    enum kind : uint8_t { Empty = 0, LC = 1, CSBK = 2, DataHeader = 3, Rate12 = 4, Rate34 = 5, VoiceSync = 7, Voice = 8 };
    dmr_tx_record() { std::memset(_r, 0, sizeof _r); }
    const unsigned char* data() const { return _r; }
    dmr_tx_record& setColorCode(uint8_t cc) { _r[2] = cc; return *this; }
    dmr_tx_record& setFN(uint8_t fn) { _r[1] = fn; return *this; }
    // the nine LC bytes: flco with the PF / R bits, FID, options, destination, source (CDMRLC::getData)
    dmr_tx_record& setLC(uint8_t flco, uint8_t fid, uint8_t options, uint32_t src, uint32_t dst)
    {
        _r[4] = flco; _r[5] = fid; _r[6] = options;
        _r[7] = (uint8_t)(dst >> 16); _r[8] = (uint8_t)(dst >> 8); _r[9] = (uint8_t)dst;
        _r[10] = (uint8_t)(src >> 16); _r[11] = (uint8_t)(src >> 8); _r[12] = (uint8_t)src;
        return *this;
    }
    dmr_tx_record& lcFrame(uint8_t data_type) { _r[0] = LC; _r[3] = data_type; return *this; }            // 1 voice LC header, 2 terminator with LC
    dmr_tx_record& block(kind k, uint8_t data_type, const unsigned char* payload, size_t len)            // CSBK / data header 10, rate 1/2 12, rate 3/4 18
    {
        _r[0] = k; _r[3] = data_type;
        std::memset(_r + 16, 0, 27);
        std::memcpy(_r + 16, payload, len < 27 ? len : 27);
        return *this;
    }
    dmr_tx_record& voice(const unsigned char* codec27, uint8_t fn) { _r[0] = fn ? Voice : VoiceSync; _r[1] = fn; std::memcpy(_r + 16, codec27, 27); return *this; }

private:
    unsigned char _r[QRL_DMR_TX_RECORD_BYTES];
};
// The 40-byte call descriptor: what DMRControl reads from Settings (dmr_source_id, dmr_destination_id, dmr_call_type, dmr_vocoder,
// dmr_color_code, dmr_talker_alias; src/DMR/dmrcontrol.cpp:19-53).
class dmr_call_descriptor {
public:
    dmr_call_descriptor(uint32_t src, uint32_t dst, bool group, bool codec2, uint8_t color_code, const std::vector<unsigned char>& alias = {})
    {
        std::memset(_d, 0, sizeof _d);
        _d[0] = (uint8_t)(src >> 16); _d[1] = (uint8_t)(src >> 8); _d[2] = (uint8_t)src;
        _d[3] = (uint8_t)(dst >> 16); _d[4] = (uint8_t)(dst >> 8); _d[5] = (uint8_t)dst;
        _d[6] = group ? 0 : 3; _d[7] = codec2 ? 0xC2 : 0; _d[8] = color_code;
        std::memcpy(_d + 9, alias.data(), alias.size() < 27 ? alias.size() : 27);
    }
    const unsigned char* data() const { return _d; }

private:
    unsigned char _d[QRL_DMR_CALL_BYTES];
};

}  // namespace qrl_host
