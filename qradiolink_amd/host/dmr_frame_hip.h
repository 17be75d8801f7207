// dmr_frame_hip.h — an 80-byte record of qrl_dmr_l2_decode (include/qrl_hip.h) behind the getters of the reference's DMRFrame
// (src/DMR/dmrframe.h:50-88) as they read after DMRFrame(bytes, type), validate() and runAudioFEC(): what DMRControl::addFrames /
// processAudio (src/DMR/dmrcontrol.cpp:225-260, :625-700) look at.  The work is done on the device; this class only reads bytes.
// Below it dmr_call_event_hip reads a 128-byte record of qrl_dmr_rx_process and dmr_alias_text turns collected alias bytes into text; then the transmit side: dmr_tx_record and dmr_call_descriptor write the two records of qrl_dmr_l2_encode / qrl_dmr_voice_call_encode.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "qrl_hip.h"

namespace qrl_host {

class dmr_frame_hip {
public:
    explicit dmr_frame_hip(const unsigned char* record80) { std::memcpy(_r, record80, QRL_DMR_L2_RECORD_BYTES); }
    explicit dmr_frame_hip(const std::vector<unsigned char>& record80) { std::memcpy(_r, record80.data(), QRL_DMR_L2_RECORD_BYTES); }
    // a burst of the repeater-mode sink: the layer-2 record and the 16-byte slot record of qrl_dmr_sink_process for the same slot
    dmr_frame_hip(const unsigned char* record80, const unsigned char* slot_info16)
    {
        std::memcpy(_r, record80, QRL_DMR_L2_RECORD_BYTES);
        std::memcpy(_s, slot_info16, QRL_DMR_SINK_INFO_BYTES);
    }
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
    // what DMRFrame(bits, type) + setDownlink() left (src/DMR/dmrframe.cpp:255-298); all zero for a burst of the DMO sink
    bool getDownlink() const { return _s[0] != 0; }
    bool cachDecoded() const { return _s[1] != 0; }
    uint8_t getSlotNo() const { return _s[2]; }
    uint8_t getCachLCSS() const { return _s[3]; }               // the TACT's LCSS; getLCSS() above is the EMB's
    uint8_t getAT() const { return _s[4]; }
    void getCACH(unsigned char* cach_data) const { std::memcpy(cach_data, _s + 5, 3); }
    uint64_t endBit() const { uint64_t v = 0; for (int i = 7; i >= 0; --i) v = (v << 8) | _s[8 + i]; return v; }

private:
    uint32_t le32(int o) const { return (uint32_t)_r[o] | ((uint32_t)_r[o + 1] << 8) | ((uint32_t)_r[o + 2] << 16) | ((uint32_t)_r[o + 3] << 24); }
    unsigned char _r[QRL_DMR_L2_RECORD_BYTES];
    unsigned char _s[QRL_DMR_SINK_INFO_BYTES] = {};
};

// ---- slot timing of the repeater-mode sink (src/gr/gr_dmr_sink.cpp:171-197, src/DMR/dmrtiming.cpp:54-82).  While it walks the bits the reference
// keeps DMRTiming's sample counter: every second bit of the stream (_symbol_bits back at 0) adds SYMBOL_LENGTH_SAMPLES = 5 samples, and a bit
// that carries an rx_time tag zeroes the counter, sets the time base to the tag's time and adds nothing.  For a burst with downlink, a decoded
// CACH and slot 1 or 2 it then calls set_slot_times(slot), which stores get_sample_counter() = time base + counter * time per sample.  From
// a slot record's end_bit and the tags the host gets that value without seeing the bit stream.
struct dmr_time_tag { uint64_t bit; uint64_t ns; };      // the tag's absolute bit offset (counted like end_bit, from 0) and its time in nanoseconds
constexpr uint64_t DMR_TIME_PER_SAMPLE_NS = 41667;         // TIME_PER_SAMPLE, src/bursttimer.h:31
// rx_time's (whole seconds, fraction) as work() turns it into nanoseconds (:182-185)
inline uint64_t dmr_tag_ns(uint64_t secs, double fracs) { return (uint64_t)llround((double)(secs * 1000000000ull) + fracs * 1000000000.0); }
// whether set_slot_times is called for the burst (:105, :121)
inline bool dmr_slot_time_set(const unsigned char* slot_info16) { return slot_info16[0] && slot_info16[1] && slot_info16[2] >= 1 && slot_info16[2] <= 2; }
// the value it stores; tags in any order, the last one at or before the burst's last bit counts
inline uint64_t dmr_slot_time(uint64_t end_bit, const dmr_time_tag* tags, size_t ntags, uint64_t time_per_sample = DMR_TIME_PER_SAMPLE_NS)
{
    uint64_t base = 0, first = 0;   // the counter adds at odd bit indices first <= j < end_bit
    bool have = false;
    uint64_t at = 0;
    for (size_t k = 0; k < ntags; ++k)
        if (tags[k].bit < end_bit && (!have || tags[k].bit >= at)) { have = true; at = tags[k].bit; base = tags[k].ns; }
    if (have) first = at + 1;
    const uint64_t adds = end_bit / 2 - first / 2;   // odd j in [first, end_bit): floor(end_bit / 2) - floor(first / 2)
    return base + adds * 5u * time_per_sample;
}

// ---- the receive call layer: a 128-byte record of qrl_dmr_rx_process (include/qrl_hip.h), what DMRControl::addFrames did with one burst
// (which of its signals fired) and the stream's call state afterwards (src/DMR/dmrcontrol.cpp:225-665).  The state lives on the device.
class dmr_call_event_hip {
public:
    enum receiver_state : uint8_t { Idle = 0, LateEntry = 1, Audio = 2, Data = 3 };   // RECEIVER_STATE
    explicit dmr_call_event_hip(const unsigned char* record128) { std::memcpy(_r, record128, QRL_DMR_RX_RECORD_BYTES); }
    explicit dmr_call_event_hip(const std::vector<unsigned char>& record128) { std::memcpy(_r, record128.data(), QRL_DMR_RX_RECORD_BYTES); }
    unsigned flags() const { return (unsigned)_r[0] | ((unsigned)_r[1] << 8); }
    bool validated() const { return flags() & QRL_DMR_RX_VALID; }
    bool processed() const { return flags() & QRL_DMR_RX_PROCESSED; }                 // its process* call returned true
    bool voiceHeaderReceived() const { return flags() & QRL_DMR_RX_HEADER_VOICE; }    // headerReceived, from processVoiceHeader
    bool dataHeaderReceived() const { return flags() & QRL_DMR_RX_HEADER_DATA; }      // headerReceived, from processDataHeader
    bool terminatorReceived() const { return flags() & QRL_DMR_RX_TERMINATOR; }
    bool endBeep() const { return flags() & QRL_DMR_RX_END_BEEP; }
    bool digitalAudio() const { return flags() & QRL_DMR_RX_AUDIO; }                  // the codec bytes: dmr_frame_hip::getVoice of the same slot
    bool embeddedData() const { return flags() & QRL_DMR_RX_EMBEDDED; }               // an embedded LC completed: processEmbeddedData ran
    bool talkerAlias() const { return flags() & QRL_DMR_RX_TALKER_ALIAS; }
    bool gpsInfo() const { return flags() & QRL_DMR_RX_GPS; }
    bool unknownEmbeddedFLCO() const { return flags() & QRL_DMR_RX_UNKNOWN_FLCO; }
    uint8_t receiverState() const { return _r[2]; }
    uint8_t colorCodeRX() const { return _r[3]; }
    uint8_t FLCO_RX() const { return _r[4]; }
    uint32_t srcIdRX() const { return le32(8); }
    uint32_t dstIdRX() const { return le32(12); }
    uint8_t embeddedFLCO() const { return _r[16]; }
    void getEmbeddedRawData(unsigned char* data9) const { std::memcpy(data9, _r + 17, 9); }   // CDMREmbeddedData::getRawData
    uint8_t aliasFormat() const { return _r[26]; }
    uint8_t aliasLength() const { return _r[27]; }
    std::vector<unsigned char> aliasBytes() const { return std::vector<unsigned char>(_r + 32, _r + 32 + (_r[28] <= 68 ? _r[28] : 68)); }

private:
    uint32_t le32(int o) const { return (uint32_t)_r[o] | ((uint32_t)_r[o + 1] << 8) | ((uint32_t)_r[o + 2] << 16) | ((uint32_t)_r[o + 3] << 24); }
    unsigned char _r[QRL_DMR_RX_RECORD_BYTES];
};

// The collected alias bytes as UTF-8 text, what DMRControl::processTalkerAlias puts into its signal (src/DMR/dmrcontrol.cpp:578-623):
//   format 1, 2   the bytes as they are (the reference reads both as UTF-8)
//   format 0      the 7-bit characters unpacked as DMRUtils::parseISO7bitToISO8bit unpacks them (src/DMR/dmrutils.cpp:102-123: the first byte holds the
//                 top bit of the first character), the first unpacked character dropped, as the reference drops it, white space trimmed at both ends
//   format 3      UTF-16, high byte first (DMRUtils::parseUTF16, :81-100), surrogate pairs joined
// Bytes that are no valid UTF-8 (formats 1, 2) or lone surrogates (format 3) are passed on / replaced by U+FFFD; nothing here fails.
inline void dmr_utf8_append(std::string& out, uint32_t c)
{
    if (c < 0x80) out += (char)c;
    else if (c < 0x800) { out += (char)(0xC0 | (c >> 6)); out += (char)(0x80 | (c & 0x3F)); }
    else if (c < 0x10000) { out += (char)(0xE0 | (c >> 12)); out += (char)(0x80 | ((c >> 6) & 0x3F)); out += (char)(0x80 | (c & 0x3F)); }
    else { out += (char)(0xF0 | (c >> 18)); out += (char)(0x80 | ((c >> 12) & 0x3F)); out += (char)(0x80 | ((c >> 6) & 0x3F)); out += (char)(0x80 | (c & 0x3F)); }
}
inline std::string dmr_alias_text(unsigned format, const std::vector<unsigned char>& bytes)
{
    std::string out;
    const size_t size = bytes.size();
    if (format == 1 || format == 2) return std::string(bytes.begin(), bytes.end());
    if (format == 3) {
        for (size_t i = 0; i + 1 < size; i += 2) {
            uint32_t c = ((uint32_t)bytes[i] << 8) | bytes[i + 1];
            if (c >= 0xD800 && c < 0xDC00 && i + 3 < size) {
                const uint32_t lo = ((uint32_t)bytes[i + 2] << 8) | bytes[i + 3];
                if (lo >= 0xDC00 && lo < 0xE000) { c = 0x10000 + ((c - 0xD800) << 10) + (lo - 0xDC00); i += 2; }
            }
            if (c >= 0xD800 && c < 0xE000) c = 0xFFFD;
            dmr_utf8_append(out, c);
        }
        return out;
    }
    // format 0
    const size_t bit7_size = 8 * size / 7;
    std::vector<unsigned char> conv(bit7_size + 1, 0);
    unsigned remainder = 0;
    for (size_t i = 0, j = 1, k = 0; k < bit7_size && i < size; ++i, ++j, ++k) {
        if (j > 7) j = 1;
        conv[k] = (unsigned char)((remainder << (8 - j)) | (bytes[i] >> j));
        const unsigned mask = (1u << j) - 1u;
        remainder = bytes[i] & mask;
        if (mask == 0x7F) { ++k; conv[k] = (unsigned char)(remainder & 0x7F); remainder = 0; }
    }
    size_t a = bit7_size ? 1 : 0, b = bit7_size;
    auto space = [](unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); };
    while (a < b && space(conv[a])) ++a;
    while (b > a && space(conv[b - 1])) --b;
    for (size_t k = a; k < b; ++k) dmr_utf8_append(out, conv[k]);
    return out;
}

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
