// m17_link_hip.h — readers and a writer for the records of the M17 link layer on the device (include/qrl_hip.h, csrc/m17_link_core.hpp), for a
// host that gets them through gr_modem_hip (m17LinkEvents, setM17Call):
//   m17_link_event_hip    the 64-byte record of qrl_m17_rx_process: which signals gr_modem::processReceivedData fires for the frame (reference
//                         src/gr_modem.cpp:1370-1439) and their arguments -- the CAN, the texts of M17LinkSetupFrame::getSource() / getDestination()
//                         (src/M17/M17/M17LinkSetupFrame.cpp:49-52, 83-97), the 16 payload bytes of digitalAudio
//   m17_call_descriptor   the 32-byte call descriptor of qrl_m17_call_* from what M17Transmitter::start is given (src/M17/M17/M17Transmitter.cpp:46-72)
// Header only; no device code.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <string>

#include "qrl_hip.h"

namespace qrl_host {

class m17_link_event_hip {
public:
    explicit m17_link_event_hip(const uint8_t* record64) { std::memcpy(d, record64, QRL_M17_RX_RECORD_BYTES); }
    unsigned flags() const { return d[0] | (unsigned)d[1] << 8; }
    bool frame() const { return flags() & QRL_M17_RX_FRAME; }                    // false: the record was passed over (another size or frame type)
    bool lsfValid() const { return flags() & QRL_M17_RX_LSF_VALID; }             // lsf.valid() after the frame
    bool frameInfoReceived() const { return flags() & QRL_M17_RX_INFO; }         // emit m17FrameInfoReceived(source(), destination(), CAN())
    bool digitalAudio() const { return flags() & QRL_M17_RX_AUDIO; }             // emit digitalAudio(payload(), 16)
    bool endAudioTransmission() const { return flags() & QRL_M17_RX_END; }       // emit endAudioTransmission(), receiveEnd()
    bool lichDecoded() const { return flags() & QRL_M17_RX_LICH_OK; }
    bool lsfFromLich() const { return flags() & QRL_M17_RX_LSF_FROM_LICH; }
    bool locked() const { return flags() & QRL_M17_RX_LOCKED; }                  // _m17_decoder_locked after the frame
    unsigned frameType() const { return d[2]; }                                  // M17FrameType: 1 link setup, 2 stream; 0xFF: EOT
    unsigned CAN() const { return d[3]; }
    unsigned frameNumber() const { return (d[4] | (unsigned)d[5] << 8) & 0x7FFFu; }
    bool isLastFrame() const { return d[5] & 0x80; }                             // the EOS bit
    unsigned lichSegment() const { return d[6]; }
    unsigned segmentMap() const { return d[7]; }
    std::array<uint8_t, 6> encodedSource() const { std::array<uint8_t, 6> a; std::memcpy(a.data(), d + 8, 6); return a; }
    std::array<uint8_t, 6> encodedDestination() const { std::array<uint8_t, 6> a; std::memcpy(a.data(), d + 14, 6); return a; }
    std::string source() const { return std::string(reinterpret_cast<const char*>(d + 21), d[20] <= 10 ? d[20] : 10); }
    std::string destination() const { return std::string(reinterpret_cast<const char*>(d + 32), d[31] <= 10 ? d[31] : 10); }
    const uint8_t* payload() const { return d + 48; }                            // 16 bytes, zero without digitalAudio()
private:
    uint8_t d[QRL_M17_RX_RECORD_BYTES];
};

// source, destination: the callsigns as typed (nine characters are kept; more than nine read as the reference's zero address);
// destination_type: Settings::m17_destination_type 0..4
inline std::array<uint8_t, QRL_M17_CALL_BYTES> m17_call_descriptor(const std::string& source, const std::string& destination, unsigned can, unsigned destination_type)
{
    std::array<uint8_t, QRL_M17_CALL_BYTES> a{};
    std::memcpy(a.data(), source.data(), source.size() < 9 ? source.size() : 9);
    a[9] = (uint8_t)(source.size() < 10 ? source.size() : 10);
    std::memcpy(a.data() + 10, destination.data(), destination.size() < 9 ? destination.size() : 9);
    a[19] = (uint8_t)(destination.size() < 10 ? destination.size() : 10);
    a[20] = (uint8_t)(can & 15u); a[21] = (uint8_t)destination_type;
    return a;
}

}  // namespace qrl_host
