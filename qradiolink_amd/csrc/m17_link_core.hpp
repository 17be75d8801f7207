// m17_link_core.hpp — the M17 link layer, free of HIP: what the reference keeps per stream above its per-frame FEC on receive, and the
// call as a function of the frame index on transmit.
//   receive, one frame       gr_modem::processReceivedData, the M17 branches            reference src/gr_modem.cpp:1370-1439
//   LSF frame                M17FrameDecoder::decodeLSF                                  src/M17/M17/M17FrameDecoder.cpp:111-117
//   stream frame             M17FrameDecoder::decodeStream, the LICH reassembly          src/M17/M17/M17FrameDecoder.cpp:119-147
//   reset                    M17FrameDecoder::reset, M17LinkSetupFrame::clear            M17FrameDecoder.cpp:37-43, M17LinkSetupFrame.cpp:38-42
//   CRC, valid()             M17LinkSetupFrame::crc16 / valid / updateCrc                M17LinkSetupFrame.cpp:119-132, :176-195
//   callsign text            M17LinkSetupFrame::getSource / getDestination, decode_callsign   M17LinkSetupFrame.cpp:49-52, :83-97, M17Callsign.cpp:70-105
//   transmit, the LSF        M17Transmitter::start, setDestination(int), encode_callsign  src/M17/M17/M17Transmitter.cpp:46-106, M17LinkSetupFrame.cpp:59-81,
//                                                                                        M17Callsign.cpp:26-68
//   transmit, a stream frame M17Transmitter::send, generateLichSegment                   M17Transmitter.cpp:108-143, M17LinkSetupFrame.cpp:139-174
// The per-frame FEC (decorrelator, interleaver, Viterbi, Golay) is not here: both directions work on the 40-byte record of k_m17_decode /
// k_m17_encode (M17_DEC_REC: type, LICH ok, 30 LSF bytes | 18 stream-frame bytes, the five LICH bytes at 32, the segment number at 37).
//
// The reference is reproduced as it stands:
//   decodeLSF overwrites lsf with whatever the Viterbi gave, valid or not; a damaged LSF frame therefore stops the audio of a running call
//   until a LICH round restores the LSF.  An LSF frame that is valid fires m17FrameInfoReceived every time, locked or not.
//   A LICH segment number is a 3-bit field; 6 and 7 set their bit in the 8-bit lsfSegmentMap like any other, so the map cannot reach 0x3F
//   again before a reset().  The reference also copies such a segment past the end of its 30-byte image, into the stream frame the same
//   call overwrites next; that write has no effect that can be seen and is not reproduced.
//   When the six segments are in, the image replaces lsf only if its CRC holds; the map and the image are cleared either way, and
//   clear() leaves the destination bytes 0xFF, not zero.
//   An EOT with an LSF that is not valid does nothing: no signal, no reset().
//   getDestination() loads the six destination bytes little endian and shifts them right by 16, so it compares bytes 2..5, read little
//   endian, with its constants: 0xFFFFFFFFFFFF ("ALL") can never match, and the byte strings setDestination(int) writes never match
//   either: they read back as "ECHO", "INFO" and "UNLINK" only because they are those callsigns in base 40, through decode_callsign,
//   and type 1 reads back as "BROADCAST".  decode_callsign gives 'x' for digit 0 and up to ten characters.
//   encode_callsign is not strict: a character outside its alphabet counts as digit 0 (lower case included), more than nine characters
//   give the zero address.
// M17FrameDecoder never initialises lsfSegmentMap: before the first reset() it holds whatever the memory held.  A fresh state here is the
// decoder after reset() with _m17_decoder_locked false.
//
// Receive record, M17_RX_REC = 64 bytes (QRL_M17_RX_RECORD_BYTES):
//   0..1     flags, little endian (F_*)             2   M17FrameType of the frame (1 link setup, 2 stream; EOT: 0xFF)      3   CAN
//   4..5     frame number of a stream frame, EOS bit (0x8000) included, little endian     6   LICH segment number     7   segment map after the frame
//   8..13    encoded source, 14..19 encoded destination
//   20       source text length, 21..30 the text; 31 destination text length, 32..41 the text
//   42..47   zero                                   48..63   the 16 payload bytes with F_AUDIO, else zero
// Bytes 3 and 8..41 are filled where the reference reads them: where lsf.valid().  A frame-synchroniser record whose size is not 46 or whose
// frame type is none of the three M17 words gives a record of zeros and leaves the state alone.
// Per-stream state, M17_RX_STATE_SIZE = 64 bytes: lsf (30 bytes), lsfSegmentMap, _m17_decoder_locked, lsfFromLich (30 bytes), two zero bytes.
// Public state, M17_RX_STATE_PUBLIC = 16 bytes: locked, lsf.valid(), CAN, segment map, encoded source, encoded destination (the last three
// as the LSF holds them, valid or not).
//
// Call descriptor of the transmit side, M17_CALL_BYTES = 32: 0..8 source characters, 9 their number (10: more than nine), 10..18 destination
// characters, 19 their number, 20 CAN, 21 destination_type, the rest zero.
#pragma once
#include <cstdint>
#include <cstddef>

#if defined(__HIPCC__)
#define QRL_M17_HD __host__ __device__
#else
#define QRL_M17_HD
#endif

namespace qrl {
namespace m17 {

enum { M17_FS_REC = 56, M17_DEC_REC = 40, M17_RX_REC = 64, M17_RX_STATE_SIZE = 64, M17_RX_STATE_PUBLIC = 16, M17_CALL_BYTES = 32, M17_FRAME = 48,
       M17_START_BYTES = 96, M17_END_BYTES = 64 };
enum { F_FRAME = 1 << 0, F_LSF_VALID = 1 << 1, F_INFO = 1 << 2, F_AUDIO = 1 << 3, F_END = 1 << 4, F_LICH_OK = 1 << 5, F_LSF_FROM_LICH = 1 << 6,
       F_LOCKED = 1 << 7 };
enum : uint32_t { FT_LSF = 0x55F7u, FT_STREAM = 0xFF5Du, FT_EOT = 0x555D555Du };   // src/layer1framing.h:21-23
enum { TYPE_LSF = 1, TYPE_STREAM = 2, TYPE_EOT = 0xFF };
enum { X_TEXT_SRC = 20, X_TEXT_DST = 31, X_PAYLOAD = 48 };

struct m17_rx_config { int can_rx; int decode_all_can; };
// byte i of an image sits in bits 8 (i & 3) .. of word i >> 2.  lsf[7]: bytes 28, 29 of the LSF, the segment map, the lock
struct m17_rx_state { uint32_t lsf[8]; uint32_t lich[8]; };
static_assert(sizeof(m17_rx_state) == M17_RX_STATE_SIZE, "m17_rx_state is 64 bytes");

// Every index below is a constant once the loops are unrolled, so the word arrays stay in registers.
QRL_M17_HD inline uint32_t wbyte(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xFFu; }
QRL_M17_HD inline void wset(uint32_t* w, int i, uint32_t v) { w[i >> 2] = (w[i >> 2] & ~(0xFFu << (8 * (i & 3)))) | ((v & 0xFFu) << (8 * (i & 3))); }

// M17LinkSetupFrame::crc16 over the first 28 bytes (polynomial 0x5935, start 0xFFFF)
QRL_M17_HD inline uint32_t lsf_crc(const uint32_t* w)
{
    uint32_t crc = 0xFFFFu;
#pragma GCC unroll 7
    for (int k = 0; k < 7; ++k) {
        uint32_t v = w[k];
        for (int j = 0; j < 4; ++j, v >>= 8) {
            crc ^= (v & 0xFFu) << 8;
            for (int b = 0; b < 8; ++b) crc = ((crc & 0x8000u) ? (crc << 1) ^ 0x5935u : crc << 1) & 0xFFFFu;
        }
    }
    return crc;
}
// valid(): the CRC field is big endian
QRL_M17_HD inline bool lsf_valid(const uint32_t* w)
{
    const uint32_t crc = lsf_crc(w);
    return (w[7] & 0xFFFFu) == ((crc >> 8) | ((crc & 0xFFu) << 8));
}
// clear(): zeros, the destination 0xFF; the upper half of word 7 is kept
QRL_M17_HD inline void lsf_clear(uint32_t* w)
{
    w[0] = 0xFFFFFFFFu; w[1] = 0x0000FFFFu;
#pragma GCC unroll 5
    for (int k = 2; k < 7; ++k) w[k] = 0;
    w[7] &= 0xFFFF0000u;
}
QRL_M17_HD inline m17_rx_state m17_rx_fresh()
{
    m17_rx_state st;
    st.lsf[7] = 0; st.lich[7] = 0;
    lsf_clear(st.lsf); lsf_clear(st.lich);
    return st;
}
QRL_M17_HD inline uint32_t lsf_can(const uint32_t* w) { return (((wbyte(w, 12) << 8) | wbyte(w, 13)) >> 7) & 0xFu; }   // getType().fields.CAN
// the twelve callsign bytes as a record holds them: source (LSF bytes 6..11), then destination (0..5)
QRL_M17_HD inline void lsf_calls(const uint32_t* w, uint32_t* three)
{
    three[0] = (w[1] >> 16) | (w[2] << 16);
    three[1] = (w[2] >> 16) | (w[0] << 16);
    three[2] = (w[0] >> 16) | (w[1] << 16);
}

QRL_M17_HD inline uint32_t base40_char(uint32_t d)   // charMap of decode_callsign
{
    return d == 0 ? 'x' : d <= 26 ? 'A' + d - 1 : d <= 36 ? '0' + d - 27 : d == 37 ? '-' : d == 38 ? '/' : '.';
}
// a text of n <= 10 characters, four to a word (character i in bits 8 (i & 3) .. of t[i >> 2]), into a record: its length at byte AT, the
// characters behind it.  The two places a record has (20, 31) are written out, so that no index depends on a loop the compiler may keep
template <int AT> QRL_M17_HD inline void put_text(uint32_t* r, uint32_t n, const uint32_t* t)
{
    static_assert(AT == X_TEXT_SRC || AT == X_TEXT_DST, "a record holds two texts");
    if (AT == X_TEXT_SRC) {                      // bytes 20 | 21..30
        r[5] |= n | (t[0] << 8);
        r[6] |= (t[0] >> 24) | (t[1] << 8);
        r[7] |= (t[1] >> 24) | ((t[2] & 0xFFFFu) << 8);
    } else {                                     // bytes 31 | 32..41
        r[7] |= n << 24;
        r[8] |= t[0]; r[9] |= t[1]; r[10] |= t[2] & 0xFFFFu;
    }
}
QRL_M17_HD constexpr uint32_t chars4(char a, char b = 0, char c = 0, char d = 0)
{
    return (uint32_t)(unsigned char)a | ((uint32_t)(unsigned char)b << 8) | ((uint32_t)(unsigned char)c << 16) | ((uint32_t)(unsigned char)d << 24);
}
// one base-40 digit of the 48-bit value hi:mid:lo (16-bit limbs), least significant first, divided out limb by limb: character I of the text
template <int I> QRL_M17_HD inline void base40_digits(uint32_t& hi, uint32_t& mid, uint32_t& lo, uint32_t* t, uint32_t& n)
{
    if (hi | mid | lo) {
        uint32_t cur = hi;
        hi = cur / 40u; cur = ((cur % 40u) << 16) | mid;
        mid = cur / 40u; cur = ((cur % 40u) << 16) | lo;
        lo = cur / 40u;
        t[I >> 2] |= base40_char(cur % 40u) << (8 * (I & 3));
        n = (uint32_t)I + 1u;
    }
    if constexpr (I < 9) base40_digits<I + 1>(hi, mid, lo, t, n);
}
// decode_callsign of the six bytes c0..c5, the 48-bit value, big endian, as three 16-bit limbs -> n characters in t.  A name replaces the
// digits by assignment, not by another path to the record: the record is written in one place
QRL_M17_HD inline void callsign_text(uint32_t hi, uint32_t mid, uint32_t lo, uint32_t* t, uint32_t& n)
{
    const bool broadcast = hi == 0xFFFFu && mid == 0xFFFFu && lo == 0xFFFFu;
    t[0] = 0; t[1] = 0; t[2] = 0; n = 0;
    base40_digits<0>(hi, mid, lo, t, n);
    if (broadcast) { n = 9; t[0] = chars4('B', 'R', 'O', 'A'); t[1] = chars4('D', 'C', 'A', 'S'); t[2] = chars4('T'); }
}
// CAN, the encoded callsigns and the texts of getSource() / getDestination() into a record
QRL_M17_HD inline void put_lsf_fields(const uint32_t* w, uint32_t* r)
{
    r[0] |= lsf_can(w) << 24;
    lsf_calls(w, r + 2);
    uint32_t t[3], n;
    callsign_text((wbyte(w, 6) << 8) | wbyte(w, 7), (wbyte(w, 8) << 8) | wbyte(w, 9), (wbyte(w, 10) << 8) | wbyte(w, 11), t, n);
    put_text<X_TEXT_SRC>(r, n, t);
    callsign_text((wbyte(w, 0) << 8) | wbyte(w, 1), (wbyte(w, 2) << 8) | wbyte(w, 3), (wbyte(w, 4) << 8) | wbyte(w, 5), t, n);
    // getDestination: memcpy of six bytes into a uint64_t, >> 16, compared with 48-bit constants
    const uint64_t v = (uint64_t)(wbyte(w, 2) | (wbyte(w, 3) << 8) | (wbyte(w, 4) << 16) | (wbyte(w, 5) << 24));
    if (v == 0xFFFFFFFFFFFFull) { n = 3; t[0] = chars4('A', 'L', 'L'); t[1] = 0; t[2] = 0; }
    else if (v == 0x0000000ED87Dull) { n = 4; t[0] = chars4('E', 'C', 'H', 'O'); t[1] = 0; t[2] = 0; }
    else if (v == 0x0000000ECDB9ull) { n = 4; t[0] = chars4('I', 'N', 'F', 'O'); t[1] = 0; t[2] = 0; }
    else if (v == 0x0000454F7745ull) { n = 6; t[0] = chars4('U', 'N', 'L', 'I'); t[1] = chars4('N', 'K'); t[2] = 0; }
    put_text<X_TEXT_DST>(r, n, t);
}

// One record of the frame synchroniser through the link layer.  ftype, word1: the record's two header words; d: the ten words of the
// frame's 40-byte decode record (not read for an EOT); r: the sixteen words of the output record.
QRL_M17_HD inline void m17_rx_step(const m17_rx_config& cfg, m17_rx_state& st, uint32_t ftype, uint32_t word1, const uint32_t* d, uint32_t* r)
{
#pragma GCC unroll 16
    for (int k = 0; k < 16; ++k) r[k] = 0;
    if ((word1 & 0xFFFFu) != 46u || (ftype != FT_LSF && ftype != FT_STREAM && ftype != FT_EOT)) return;
    uint32_t flags = F_FRAME, type, map = (st.lsf[7] >> 16) & 0xFFu;
    bool locked = ((st.lsf[7] >> 24) & 1u) != 0, valid;
    if (ftype == FT_LSF) {                                           // gr_modem.cpp:1380-1394
        type = TYPE_LSF;
#pragma GCC unroll 7
        for (int k = 0; k < 7; ++k) st.lsf[k] = (d[k] >> 16) | (d[k + 1] << 16);          // decodeLSF: record bytes 2..31
        st.lsf[7] = (st.lsf[7] & 0xFFFF0000u) | (d[7] >> 16);
        valid = lsf_valid(st.lsf);
        if (valid) { locked = true; flags |= F_INFO; put_lsf_fields(st.lsf, r); }
    } else if (ftype == FT_STREAM) {                                 // gr_modem.cpp:1396-1419
        type = TYPE_STREAM;
        if (wbyte(d, 1)) {                                           // decodeStream, M17FrameDecoder.cpp:128-147
            flags |= F_LICH_OK;
            const uint32_t seg = wbyte(d, 37) & 7u;
#pragma GCC unroll 6
            for (int s = 0; s < 6; ++s)
                if (seg == (uint32_t)s) {
#pragma GCC unroll 5
                    for (int j = 0; j < 5; ++j) wset(st.lich, 5 * s + j, wbyte(d, 32 + j));
                }
            map |= 1u << seg;
            r[1] |= seg << 16;
            if (map == 0x3Fu) {
                if (lsf_valid(st.lich)) {
#pragma GCC unroll 7
                    for (int k = 0; k < 7; ++k) st.lsf[k] = st.lich[k];
                    st.lsf[7] = (st.lsf[7] & 0xFFFF0000u) | (st.lich[7] & 0xFFFFu);
                    flags |= F_LSF_FROM_LICH;
                }
                map = 0;
                lsf_clear(st.lich);
            }
        }
        r[1] |= wbyte(d, 3) | (wbyte(d, 2) << 8);                    // getFrameNumber(): the field is big endian
        valid = lsf_valid(st.lsf);
        if (valid) {
            put_lsf_fields(st.lsf, r);
            if (lsf_can(st.lsf) == (uint32_t)cfg.can_rx || cfg.decode_all_can) {
                flags |= F_AUDIO;
#pragma GCC unroll 4
                for (int k = 0; k < 4; ++k) r[X_PAYLOAD / 4 + k] = d[1 + k];             // record bytes 4..19
            }
            if (!locked) { locked = true; flags |= F_INFO; }
        }
    } else {                                                         // gr_modem.cpp:1421-1439
        type = TYPE_EOT;
        if (lsf_valid(st.lsf)) {
            put_lsf_fields(st.lsf, r);
            locked = false;
            flags |= F_INFO;
            if (lsf_can(st.lsf) == (uint32_t)cfg.can_rx || cfg.decode_all_can) flags |= F_END;
            map = 0;                                                 // reset()
            lsf_clear(st.lsf); lsf_clear(st.lich);
        }
        valid = lsf_valid(st.lsf);
    }
    if (valid) flags |= F_LSF_VALID;
    if (locked) flags |= F_LOCKED;
    st.lsf[7] = (st.lsf[7] & 0xFFFFu) | (map << 16) | ((locked ? 1u : 0u) << 24);
    r[0] |= flags | (type << 16);
    r[1] |= map << 24;
}

// the public sixteen bytes of a state
QRL_M17_HD inline void m17_rx_public(const m17_rx_state& st, uint32_t* four)
{
    four[0] = ((st.lsf[7] >> 24) & 1u) | ((lsf_valid(st.lsf) ? 1u : 0u) << 8) | (lsf_can(st.lsf) << 16) | (((st.lsf[7] >> 16) & 0xFFu) << 24);
    lsf_calls(st.lsf, four + 1);
}

// ------------------------------------------------------------------------------------------------------------------ transmit
// encode_callsign(callsign, call, strict = false) of n characters s[0..8] (n > 9: the zero address) -> hi, mid, lo 16-bit limbs
QRL_M17_HD inline void encode_callsign(const uint8_t* s, uint32_t n, uint32_t& hi, uint32_t& mid, uint32_t& lo)
{
    uint64_t v = 0;
    if (n <= 9) {
        for (int i = 8; i >= 0; --i) {
            if ((uint32_t)i >= n) continue;
            const uint32_t c = s[i];
            v *= 40u;
            if (c >= 'A' && c <= 'Z') v += c - 'A' + 1u;
            else if (c >= '0' && c <= '9') v += c - '0' + 27u;
            else if (c == '-') v += 37u;
            else if (c == '/') v += 38u;
            else if (c == '.') v += 39u;
        }
    }
    hi = (uint32_t)(v >> 32) & 0xFFFFu; mid = (uint32_t)(v >> 16) & 0xFFFFu; lo = (uint32_t)v & 0xFFFFu;
}
QRL_M17_HD inline void put_call(uint32_t* w, int at, uint32_t hi, uint32_t mid, uint32_t lo)   // at: 0 or 6
{
    wset(w, at, hi >> 8); wset(w, at + 1, hi); wset(w, at + 2, mid >> 8); wset(w, at + 3, mid); wset(w, at + 4, lo >> 8); wset(w, at + 5, lo);
}
// the LSF M17Transmitter::start builds for a call descriptor: eight words, the upper half of the last zero
QRL_M17_HD inline void call_lsf(const uint8_t* desc, uint32_t* w)
{
    w[7] = 0;
    lsf_clear(w);
    uint32_t hi, mid, lo;
    encode_callsign(desc, desc[9], hi, mid, lo);
    put_call(w, 6, hi, mid, lo);
    const uint32_t dtype = desc[21];
    if (dtype == 0) {
        if (desc[19]) { encode_callsign(desc + 10, desc[19], hi, mid, lo); put_call(w, 0, hi, mid, lo); }
    }
    else if (dtype == 2) put_call(w, 0, 0x0000u, 0x000Eu, 0xD87Du);      // ECHO   (type 1, ALL, writes the 0xFF bytes that are there)
    else if (dtype == 3) put_call(w, 0, 0x0000u, 0x000Eu, 0xCDB9u);      // INFO
    else if (dtype == 4) put_call(w, 0, 0x0000u, 0x454Fu, 0x7745u);      // UNLINK
    const uint32_t type = 1u | (2u << 1) | ((desc[20] & 0xFu) << 7);     // stream, voice, no encryption, CAN
    wset(w, 12, type >> 8); wset(w, 13, type);
    const uint32_t crc = lsf_crc(w);
    wset(w, 28, crc >> 8); wset(w, 29, crc);
}
// the record (layout of k_m17_decode / k_m17_encode) of the LSF frame
QRL_M17_HD inline void lsf_record(const uint32_t* w, uint32_t* rec)
{
    rec[0] = TYPE_LSF | (w[0] << 16);
#pragma GCC unroll 7
    for (int k = 1; k < 8; ++k) rec[k] = (w[k - 1] >> 16) | (w[k] << 16);
    rec[8] = 0; rec[9] = 0;
}
// the record of stream frame k of the call: frame number k & 0x7FF, LICH segment k % 6; pay: the four payload words; eos: the last frame
QRL_M17_HD inline void stream_record(const uint32_t* w, uint32_t k, const uint32_t* pay, bool eos, uint32_t* rec)
{
    const uint32_t fn = k & 0x7FFu, seg = k % 6u;
    rec[0] = TYPE_STREAM | (1u << 8) | (((fn >> 8) | (eos ? 0x80u : 0u)) << 16) | ((fn & 0xFFu) << 24);
#pragma GCC unroll 4
    for (int j = 0; j < 4; ++j) rec[1 + j] = pay[j];
    rec[5] = 0; rec[6] = 0; rec[7] = 0; rec[8] = 0; rec[9] = 0;
#pragma GCC unroll 6
    for (int s = 0; s < 6; ++s)
        if (seg == (uint32_t)s) {
#pragma GCC unroll 5
            for (int j = 0; j < 5; ++j) wset(rec, 32 + j, wbyte(w, 5 * s + j));
        }
    wset(rec, 37, seg);
}

}  // namespace m17
}  // namespace qrl
