// dmr_rx_core.hpp — the DMR receive call layer, free of HIP: the per-stream protocol state the reference keeps above its frame layer, the
// receive half of DMRControl in DMO mode with an idle transmitter (reference src/DMR/dmrcontrol.cpp).
//   one burst                addFrames' loop body                              src/DMR/dmrcontrol.cpp:625-665
//   by data type             processCSBK / processDataHeader / processVoiceHeader / processTerminator / processAudio   :225-402
//   colour code              processColorCode                                  :415-442
//   timeslot (repeater mode) processTimeslot, the CACH and timeslot filters of addFrames   :444-462, :636-644
//   embedded LC              CDMREmbeddedData::addData / decodeEmbeddedData / reset / getLC / getRawData   src/MMDVM/DMREmbeddedData.cpp:47-109, :213-322
//                            CHamming::decode16114, CCRC::checkFiveBit         src/MMDVM/Hamming.cpp:231-277, CRC.cpp:122-146
//   what the LC says         processEmbeddedData, the completion rule of processTalkerAlias   src/DMR/dmrcontrol.cpp:464-623
// Input is the 80-byte record of dmr_l2_core.hpp's decode_record (validate(), the data type, colour code, IDs, the EMB's LCSS and the
// regenerated burst); output one DMR_RX_REC-byte record per burst: what addFrames did with it and the stream's state afterwards.  The
// reference is reproduced as it stands: processColorCode's chain of || over the data types is always true, so without promiscuous mode
// any burst of another colour code is refused; a voice burst is checked with _color_code_RX in place of its own colour code; a terminator
// with source and destination 0 is passed over; nothing but reset() and an LCSS 1 fragment clears the embedded data, and a terminator
// leaves a half-collected alias where it is.  The two fields the reference never initialises (_ta_df, _ta_dl) start at 0.
// In repeater mode (dmr_mode != DMR_MODE_DMO) addFrames passes over a burst whose CACH was not decoded, and one of the other timeslot unless
// promiscuous; every process* call then runs processTimeslot, which in promiscuous mode locks _timeslot_RX to the first slot seen until a
// terminator releases it.  processAudio asks the timeslot before the colour code, the other calls the colour code first, and each check
// takes its lock before the other refuses the burst; that order is kept.  The transmitter is idle.
//
// The 128 bits of an embedded LC are kept as the four fragments, first bit highest.  The matrix is sent by columns, so byte c of those 16
// is column c with row 0 in its top bit, and the de-interleave (b += 16 mod 127) is the transpose 16 columns x 8 rows -> 8 row words,
// bit j of a word = column j, the layout of dmr_tx_core.hpp's embedded_lc_fragment.  A row's five parity equations are the four (15,11,3)
// equations of the BPTC (h15_mask) and the one that makes every data column of the check matrix odd; no code table.
//
// Output record, DMR_RX_REC = 128 bytes (QRL_DMR_RX_RECORD_BYTES):
//   0..1     flags, little endian (F_*)
//   2        receiver state after the burst (RECEIVER_STATE: 0 idle, 1 late entry, 2 audio, 3 data)   3   _color_code_RX   4   _FLCO_RX
//   5        _timeslot_RX after the burst (0 in DMO mode)   6..7   zero
//   8..11    _srcId_RX, 12..15 _dstId_RX, little endian
//   16       FLCO of the embedded LC, 17..25 its nine getRawData bytes (F_EMBEDDED only, else zero)
//   26       talker-alias format, 27 its length field, 28 the number of bytes collected, 32..99 those bytes (F_TALKER_ALIAS only, else zero)
//   29..31, 100..127   zero
// Per-stream state, DMR_RX_STATE_SIZE = 128 bytes; its first 12 bytes are the public part (QRL_DMR_RX_STATE_BYTES):
//   0 receiver state, 1 _color_code_RX, 2 _FLCO_RX, 3 _timeslot_RX, 4..7 source, 8..11 destination (little endian)
// A state of all zero bytes is a fresh DMRControl.
#pragma once
#include "dmr_l2_core.hpp"

namespace qrl {
namespace dmr {

enum { DMR_RX_REC = 128, DMR_RX_STATE_SIZE = 128, DMR_RX_STATE_PUBLIC = 12, TA_MAX = 68 };
enum { F_VALID = 1 << 0, F_PROCESSED = 1 << 1, F_HEADER_VOICE = 1 << 2, F_HEADER_DATA = 1 << 3, F_TERMINATOR = 1 << 4, F_END_BEEP = 1 << 5,
       F_AUDIO = 1 << 6, F_EMBEDDED = 1 << 7, F_TALKER_ALIAS = 1 << 8, F_GPS = 1 << 9, F_UNKNOWN_FLCO = 1 << 10, F_SLOT_REFUSED = 1 << 11 };
enum { X_FLAGS = 0, X_STATE = 2, X_CC = 3, X_FLCO = 4, X_TS = 5, X_SRC = 8, X_DST = 12, X_EMB_FLCO = 16, X_EMB_RAW = 17, X_TA_FORMAT = 26, X_TA_LENGTH = 27,
       X_TA_COUNT = 28, X_TA = 32 };
enum { RX_IDLE = 0, RX_LATE_ENTRY = 1, RX_AUDIO = 2, RX_DATA = 3 };
enum { LCS_NONE = 0, LCS_FIRST = 1, LCS_SECOND = 2, LCS_THIRD = 3 };
enum { FLCO_GROUP = 0, FLCO_USER_USER = 3, FLCO_TA_HEADER = 4, FLCO_TA_BLOCK1 = 5, FLCO_TA_BLOCK3 = 7, FLCO_GPS_INFO = 8 };

// repeater: 0 = DMR_MODE_DMO (what two initialisers give), 1 = repeater mode with the timeslot 1 or 2 of Settings::dmr_timeslot
struct dmr_rx_config { int color_code; int promiscuous; int repeater; int timeslot; };
// the two bytes of a slot record (dmr_sink_core.hpp) the call layer reads
enum { SLOT_CACH_DECODED = 1, SLOT_NO = 2, SLOT_REC = 16 };

struct dmr_rx_state {
    uint8_t rx_state, cc_rx, flco_rx, ts_rx;   // ts_rx: _timeslot_RX
    uint32_t src, dst;
    uint8_t lcs, emb_valid, emb_flco, ta_received;   // CDMREmbeddedData: m_state, m_valid, m_FLCO
    uint8_t ta_df, ta_dl, ta_size, pad1;
    uint32_t raw[4];                                  // m_raw: fragment k, its first bit highest
    uint32_t emb_data[3];                             // m_data, nine bytes, as the last decode that reached the checksum left them: byte i in
                                                      // bits 8 (i & 3) .. of word i >> 2, like ta
    uint32_t ta[TA_MAX / 4];                          // _ta_data: byte i in bits 8 (i & 3) .. of word i >> 2
    uint32_t pad2[3];
};
static_assert(X_FLAGS == 0 && X_STATE == 2 && X_CC == 3 && X_EMB_FLCO == 16 && X_EMB_RAW == 17 && X_TA_FORMAT == 26 && X_TA_LENGTH == 27 && X_TA % 4 == 0,
              "dmr_rx_step packs the record's words by these offsets");
static_assert(sizeof(dmr_rx_state) == DMR_RX_STATE_SIZE, "dmr_rx_state is 128 bytes");

// ---- Hamming (16,11,4) of a row: parity p covers the data bits of h16_mask(p) and sits in bit 11 + p ----
QRL_HD constexpr unsigned h16_mask(int p)
{
    if (p < 4) return h15_mask(p);
    unsigned m = 0;   // the fifth equation: the data bits that enter an even number of the other four
    for (int j = 0; j < 11; ++j) {
        unsigned n = 0;
        for (int q = 0; q < 4; ++q) n += (h15_mask(q) >> j) & 1u;
        if (!(n & 1u)) m |= 1u << j;
    }
    return m;
}
QRL_HD constexpr unsigned h16_column(int j)   // the syndrome of an error in bit j alone
{
    if (j >= 11) return 1u << (j - 11);
    unsigned c = 0;
    for (int p = 0; p < 5; ++p) c |= ((h16_mask(p) >> j) & 1u) << p;
    return c;
}
// CHamming::decode16114 on a row word: one wrong bit is put right; false for any other syndrome
QRL_HD inline bool hamming16114_decode(unsigned& w)
{
    unsigned syn = 0;
#pragma GCC unroll 5
    for (int p = 0; p < 5; ++p) syn |= (popc32(w & (h16_mask(p) | (1u << (11 + p)))) & 1u) << p;
    unsigned flip = 0;
#pragma GCC unroll 16
    for (int j = 0; j < 16; ++j) if (h16_column(j) == syn) flip = 1u << j;
    w ^= flip;
    return !syn || flip;
}

// the 16 x 8 transpose: row r of the matrix from the four fragments
QRL_HD inline unsigned embedded_row(const uint32_t* raw, int r)
{
    unsigned w = 0;
#pragma GCC unroll 4
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = raw[k] >> (7 - r);   // column 4 k + j of the row is now bit 8 (3 - j)
        w |= (((t >> 24) & 1u) | ((t >> 15) & 2u) | ((t >> 6) & 4u) | ((t << 3) & 8u)) << (4 * k);
    }
    return w;
}

// CDMREmbeddedData::decodeEmbeddedData on the four fragments.  Returns 0 when a row fails, 1 for a column parity failure (data is left alone in
// both), 2 for a checksum failure (data is written), 3 when all is well.  data: the nine bytes in three words, byte i in bits 8 (i & 3) .. of word i >> 2.
QRL_HD inline int embedded_lc_decode(const uint32_t* raw, uint32_t* data)
{
    unsigned all = embedded_row(raw, 7), crc = 0, sum = 0, pos = 0;
    uint32_t d0 = 0, d1 = 0, d2 = 0;   // three scalars, the word picked by comparison: no array for the compiler to keep in memory
    bool rows_ok = true;
#pragma GCC unroll 7
    for (int r = 0; r < 7; ++r) {
        unsigned w = embedded_row(raw, r);
        rows_ok = hamming16114_decode(w) && rows_ok;
        all ^= w;
        const int nbits = r < 2 ? 11 : 10;
#pragma GCC unroll 11
        for (int j = 0; j < 11; ++j) {
            if (j >= nbits) break;
            const uint32_t bit = ((w >> j) & 1u) << (8u * ((pos >> 3) & 3u) + 7u - (pos & 7u));
            d0 |= pos < 32u ? bit : 0u; d1 |= pos >= 32u && pos < 64u ? bit : 0u; d2 |= pos >= 64u ? bit : 0u;
            ++pos;
        }
        if (r >= 2) crc = (crc << 1) | ((w >> 10) & 1u);
    }
    if (!rows_ok) return 0;
    if (all) return 1;
#pragma GCC unroll 9
    for (int i = 0; i < 9; ++i) sum += ((i < 4 ? d0 : i < 8 ? d1 : d2) >> (8 * (i & 3))) & 0xFFu;
    data[0] = d0; data[1] = d1; data[2] = d2;
    return sum % 31u == crc ? 3 : 2;
}
QRL_HD inline unsigned word_byte(const uint32_t* w, unsigned i) { return (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }

// CDMREmbeddedData::addData: frag is the 32 embedded bits of a voice burst B..F, lcss the EMB's.  True when the fourth fragment completes a valid LC.
QRL_HD inline bool embedded_add(dmr_rx_state& st, uint32_t frag, unsigned lcss)
{
    if (lcss == 1u) { st.raw[0] = frag; st.lcs = LCS_FIRST; st.emb_valid = 0; return false; }
    if (lcss == 3u && st.lcs == LCS_FIRST) { st.raw[1] = frag; st.lcs = LCS_SECOND; return false; }
    if (lcss == 3u && st.lcs == LCS_SECOND) { st.raw[2] = frag; st.lcs = LCS_THIRD; return false; }
    if (lcss == 2u && st.lcs == LCS_THIRD) {
        st.raw[3] = frag; st.lcs = LCS_NONE;
        if (embedded_lc_decode(st.raw, st.emb_data) == 3) { st.emb_valid = 1; st.emb_flco = (uint8_t)(st.emb_data[0] & 0x3Fu); }
        return st.emb_valid != 0;
    }
    return false;
}

// _ta_data.append of n <= 7 bytes at once, v's byte 0 first.  Every word takes its share of v by a shift, so no word is picked by an index and
// the buffer can live in registers (a loop that compares the word number with the index is turned back into an indexed store).
QRL_HD inline void ta_append(dmr_rx_state& st, uint64_t v, unsigned n)
{
    const int size = st.ta_size;
#pragma GCC unroll 17
    for (int w = 0; w < TA_MAX / 4; ++w) {
        const int d = 4 * w - size;   // bytes from the first new byte to the word's byte 0
        uint32_t c = 0;
        if (d >= 0 && d < 8) c = (uint32_t)(v >> (8 * d));
        else if (d < 0 && d > -4) c = (uint32_t)(v << (8 * -d));
        st.ta[w] |= c;
    }
    st.ta_size = (uint8_t)(size + (int)n);
}
QRL_HD inline void ta_clear(dmr_rx_state& st)
{
#pragma GCC unroll 17
    for (int w = 0; w < TA_MAX / 4; ++w) st.ta[w] = 0;
    st.ta_size = 0;
}

// the completion rule of DMRControl::processTalkerAlias; the text itself is made on the host from the record
QRL_HD inline unsigned talker_alias_check(dmr_rx_state& st, uint32_t* out)
{
    const unsigned size = st.ta_size, df = st.ta_df, dl = st.ta_dl;
    if (size < 1u) return 0;
    const unsigned bit7_size = 8u * size / 7u;
    if (!(((df == 1u || df == 2u) && size >= dl) || (df == 3u && size >= 2u * dl) || (df == 0u && bit7_size >= dl))) return 0;
    out[X_TA_FORMAT / 4] |= (df << 16) | (dl << 24);
    out[X_TA_COUNT / 4] = size;
#pragma GCC unroll 17
    for (unsigned w = 0; w < TA_MAX / 4; ++w) out[X_TA / 4 + w] = st.ta[w];   // the bytes behind `size` are zero
    st.ta_received = 1;
    ta_clear(st);
    st.ta_dl = 0; st.ta_df = 0;
    return F_TALKER_ALIAS;
}

QRL_HD inline uint64_t bytes_le(const unsigned* b, int n)
{
    uint64_t v = 0;
#pragma GCC unroll 7
    for (int i = 0; i < 7; ++i) if (i < n) v |= (uint64_t)b[i] << (8 * i);
    return v;
}
// DMRControl::processEmbeddedData; the embedded data is valid here
QRL_HD inline unsigned embedded_process(dmr_rx_state& st, uint32_t* out)
{
    const unsigned flco = st.emb_flco;
    unsigned raw[9];
#pragma GCC unroll 9
    for (unsigned i = 0; i < 9; ++i) raw[i] = word_byte(st.emb_data, i);
    unsigned flags = F_EMBEDDED;
    // bytes 16..25 of the record: the FLCO, then the nine bytes, which lie one byte further on than in the state's words
    out[4] = flco | (st.emb_data[0] << 8);
    out[5] = (st.emb_data[0] >> 24) | (st.emb_data[1] << 8);
    out[6] = (st.emb_data[1] >> 24) | ((st.emb_data[2] & 0xFFu) << 8);
    if (flco == FLCO_GROUP || flco == FLCO_USER_USER) {
        st.src = (raw[6] << 16) | (raw[7] << 8) | raw[8]; st.dst = (raw[3] << 16) | (raw[4] << 8) | raw[5]; st.flco_rx = (uint8_t)flco;
        if (st.rx_state == RX_IDLE) st.rx_state = RX_LATE_ENTRY;
    } else if (flco == FLCO_GPS_INFO) {
        flags |= F_GPS;
    } else if (flco == FLCO_TA_HEADER) {
        if (!st.ta_received) {
            st.ta_df = (uint8_t)((raw[2] >> 6) & 3u); st.ta_dl = (uint8_t)((raw[2] >> 1) & 0x1Fu);
            ta_clear(st);
            if (st.ta_df == 0u) ta_append(st, raw[2] & 1u, 1);   // 7-bit text: the first character's top bit
            ta_append(st, bytes_le(raw + 3, 6), 6);
            flags |= talker_alias_check(st, out);
        }
    } else if (flco >= FLCO_TA_BLOCK1 && flco <= FLCO_TA_BLOCK3) {
        if (!st.ta_received && st.ta_dl > 0u) {
            ta_append(st, bytes_le(raw + 2, 7), 7);
            flags |= talker_alias_check(st, out);
        }
    } else flags |= F_UNKNOWN_FLCO;
    return flags;
}

// DMRControl::processColorCode
QRL_HD inline bool colour_code_ok(const dmr_rx_config& cfg, dmr_rx_state& st, unsigned cc)
{
    if (!cfg.promiscuous) return cc == (unsigned)cfg.color_code;
    if (cc != st.cc_rx && st.cc_rx != 0u) return false;
    if (st.cc_rx == 0u) st.cc_rx = (uint8_t)cc;
    return true;
}

// DMRControl::processTimeslot
QRL_HD inline bool timeslot_ok(const dmr_rx_config& cfg, dmr_rx_state& st, unsigned slot)
{
    if (!cfg.repeater) return true;
    if (slot != (unsigned)cfg.timeslot && !cfg.promiscuous) return false;
    if (cfg.promiscuous) {
        if (slot != st.ts_rx && st.ts_rx != 0u) return false;
        if (st.ts_rx == 0u) st.ts_rx = (uint8_t)slot;
    }
    return true;
}
// a process* call's two checks: the colour code first, as everywhere but in processAudio.  slot_refused: it was the timeslot that said no
QRL_HD inline bool colour_then_slot(const dmr_rx_config& cfg, dmr_rx_state& st, unsigned cc, unsigned slot, bool& slot_refused)
{
    if (!colour_code_ok(cfg, st, cc)) return false;
    if (!timeslot_ok(cfg, st, slot)) { slot_refused = true; return false; }
    return true;
}

// one iteration of addFrames' loop.  rec: the burst's 80-byte layer-2 record; slot: its 16-byte slot record, or null (cachDecoded() false, slot
// 0: a burst of the DMO sink); out: the DMR_RX_REC bytes as 32 little-endian words, all written.
QRL_HD inline void dmr_rx_step_slots(const dmr_rx_config& cfg, dmr_rx_state& st, const uint8_t* rec, const uint8_t* slot, uint32_t* out)
{
    const bool cach_decoded = slot && slot[SLOT_CACH_DECODED];
    const unsigned slot_no = slot ? slot[SLOT_NO] : 0u;
#pragma GCC unroll 32
    for (int i = 0; i < DMR_RX_REC / 4; ++i) out[i] = 0;
    unsigned flags = 0;
    if (rec[R_VALID]) {
        const unsigned dt = rec[R_DTYPE], cc = rec[R_CC];
        const uint32_t src = (uint32_t)rec[R_SRC] | ((uint32_t)rec[R_SRC + 1] << 8) | ((uint32_t)rec[R_SRC + 2] << 16) | ((uint32_t)rec[R_SRC + 3] << 24);
        const uint32_t dst = (uint32_t)rec[R_DST] | ((uint32_t)rec[R_DST + 1] << 8) | ((uint32_t)rec[R_DST + 2] << 16) | ((uint32_t)rec[R_DST + 3] << 24);
        bool ok = true, slot_refused = false;
        flags = F_VALID;
        if (cfg.repeater && (!cach_decoded || (slot_no != (unsigned)cfg.timeslot && !cfg.promiscuous))) {
            ok = false; slot_refused = true;   // addFrames goes on to the next burst
        } else if (dt == DT_CSBK || dt == DT_MBC_HEADER || dt == DT_MBC_CONTINUATION) {
            ok = colour_then_slot(cfg, st, cc, slot_no, slot_refused);
        } else if (dt == DT_DATA_HEADER) {
            ok = colour_then_slot(cfg, st, cc, slot_no, slot_refused);
            if (ok) {
                st.cc_rx = (uint8_t)cc; st.src = src; st.dst = dst; st.flco_rx = rec[R_FLCO];
                st.rx_state = RX_DATA;
                flags |= F_HEADER_DATA;
            }
        } else if (dt == DT_VOICE_LC_HEADER) {
            ok = colour_then_slot(cfg, st, cc, slot_no, slot_refused);
            if (ok) {
                st.cc_rx = (uint8_t)cc;
                if (st.rx_state == RX_IDLE) flags |= F_END_BEEP;
                st.src = src; st.dst = dst; st.flco_rx = rec[R_FLCO];
                st.rx_state = RX_AUDIO;
                flags |= F_HEADER_VOICE;
            }
        } else if (dt == DT_TERMINATOR_WITH_LC) {
            if (dst != 0u || src != 0u) {   // one with neither ID comes from a trunking site and is passed over
                ok = colour_then_slot(cfg, st, cc, slot_no, slot_refused);
                if (ok) {
                    if (st.rx_state != RX_IDLE) flags |= F_TERMINATOR | F_END_BEEP;
                    st.src = 0; st.dst = 0; st.flco_rx = 0; st.rx_state = RX_IDLE; st.ta_received = 0; st.cc_rx = 0; st.ts_rx = 0;
                }
            }
        } else if (dt == DT_VOICE_SYNC || dt == DT_VOICE) {
            ok = timeslot_ok(cfg, st, slot_no);       // processAudio asks the timeslot first
            if (!ok) slot_refused = true;
            else ok = colour_code_ok(cfg, st, st.cc_rx);   // addFrames has put _color_code_RX into the frame
            if (ok) {
                if (dt == DT_VOICE_SYNC) {
                    st.lcs = LCS_NONE; st.emb_valid = 0;
                    if (st.rx_state == RX_IDLE) st.rx_state = RX_LATE_ENTRY;
                } else {
                    const uint8_t* b = rec + R_BURST;
                    const uint32_t frag = ((uint32_t)(b[14] & 0x0Fu) << 28) | ((uint32_t)b[15] << 20) | ((uint32_t)b[16] << 12) | ((uint32_t)b[17] << 4) |
                                          ((uint32_t)b[18] >> 4);
                    if (embedded_add(st, frag, rec[R_LCSS])) flags |= embedded_process(st, out);
                }
                if (st.rx_state == RX_AUDIO || st.rx_state == RX_LATE_ENTRY) flags |= F_AUDIO;
            }
        }
        if (ok) flags |= F_PROCESSED;
        if (slot_refused) flags |= F_SLOT_REFUSED;
    }
    out[0] = flags | ((uint32_t)st.rx_state << 16) | ((uint32_t)st.cc_rx << 24);
    out[X_FLCO / 4] = st.flco_rx | ((uint32_t)st.ts_rx << 8);
    out[X_SRC / 4] = st.src; out[X_DST / 4] = st.dst;
}
QRL_HD inline void dmr_rx_step(const dmr_rx_config& cfg, dmr_rx_state& st, const uint8_t* rec, uint32_t* out) { dmr_rx_step_slots(cfg, st, rec, nullptr, out); }
// the same, the record as bytes
QRL_HD inline void dmr_rx_step_slots_bytes(const dmr_rx_config& cfg, dmr_rx_state& st, const uint8_t* rec, const uint8_t* slot, uint8_t* out)
{
    uint32_t w[DMR_RX_REC / 4];
    dmr_rx_step_slots(cfg, st, rec, slot, w);
    for (int i = 0; i < DMR_RX_REC / 4; ++i) put32(out + 4 * i, w[i]);
}
QRL_HD inline void dmr_rx_step_bytes(const dmr_rx_config& cfg, dmr_rx_state& st, const uint8_t* rec, uint8_t* out)
{
    uint32_t w[DMR_RX_REC / 4];
    dmr_rx_step(cfg, st, rec, w);
    for (int i = 0; i < DMR_RX_REC / 4; ++i) put32(out + 4 * i, w[i]);
}
}  // namespace dmr
}  // namespace qrl
