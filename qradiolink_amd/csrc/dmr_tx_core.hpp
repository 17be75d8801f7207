// dmr_tx_core.hpp — the stateless per-burst work of DMR layer 2 on the transmit side, free of HIP: one 48-byte TX record -> one 33-byte
// burst, what the reference's frame layer does before gr_mod_base::setDMRData takes the bytes.
//   LC header / terminator   CDMRFullLC::encode, slot type, data sync       src/DMR/dmrframe.cpp:475-487, src/MMDVM/DMRFullLC.cpp:70-99
//   CSBK                     CDMRCSBK::get (CRC-CCITT, CSBK mask, BPTC)     src/DMR/dmrframe.cpp:460-473, src/MMDVM/DMRCSBK.cpp:232-263
//   data header              CDMRDataHeader::get                            src/MMDVM/DMRDataHeader.cpp:155-170
//   rate 1/2, rate 3/4       CBPTC19696::encode, CDMRTrellis::encode        src/MMDVM/BPTC19696.cpp:75-87, DMRTrellis.cpp:89-107
//   slot type                Golay(20,8)                                    src/MMDVM/DMRSlotType.cpp:56-72, Golay2087.cpp:252-262
//   voice A                  setVoice, addVoiceSync                         src/DMR/dmrframe.cpp:399-411, :498-501
//   voice B..F               setVoice, setEmbeddedData                      src/DMR/dmrframe.cpp:413-421, src/MMDVM/DMREmbeddedData.cpp:111-210,
//                            EMB through QR(16,7,6)                         src/MMDVM/DMREMB.cpp:54-70, QR1676.cpp:93-102
//   voice sequencing         DMRControl::getTxAudio                         src/DMR/dmrcontrol.cpp:128-223
// Everything here is built on dmr_l2_core.hpp (bptc_encode, rs129_parity, trellis_encode, crc_ccitt10, poly_rem) and adds no code table:
// the two systematic encoders are one polynomial remainder and a parity bit, the Hamming (16,11,4) rows of the embedded LC are the
// (15,11,3) parity equations of the BPTC plus the overall parity.  The two sync words are the MS-sourced patterns of ETSI TS 102 361-1
// table 9.2, the ones gr_dmr_dmo_sink correlates against.
//
// TX record, QRL_DMR_TX_RECORD_BYTES = 48:
//   0        kind (K_*)
//   1        FN: frame number within the voice superframe (kind 8 only: 1..4 carry fragment FN of the embedded LC, anything else a null fragment)
//   2        colour code (low four bits are sent)
//   3        data type of the slot type (kinds 1..5; kind 1 also picks the RS mask by it: 1 header, 2 terminator, anything else -> zero burst)
//   4..12    the nine LC bytes as CDMRLC(const unsigned char*) reads them: PF | R | FLCO, FID, options, destination (3), source (3)
//            (kind 1: the full LC; kind 8: the LC whose embedded form this superframe carries)
//   13..15   zero
//   16..42   payload: 10 bytes (CSBK, data header: the block without its CRC), 12 (rate 1/2), 18 (rate 3/4), 27 (voice: three codec frames)
//   43..47   zero
// Call descriptor, QRL_DMR_CALL_BYTES = 40 (voice_call_record):
//   0..2     source id, high byte first          3..5   destination id, high byte first
//   6        FLCO of the call (0 group, 3 private)       7      FID (0, or 0xC2 for Codec2 voice)
//   8        colour code                         9..35  the 27 talker-alias bytes, zero padded       36..39 zero
#pragma once
#include "dmr_l2_core.hpp"

namespace qrl {
namespace dmr {

enum { TX_REC = 48, CALL_REC = 40 };
enum { K_EMPTY = 0, K_LC = 1, K_CSBK = 2, K_DATA_HEADER = 3, K_RATE12 = 4, K_RATE34 = 5, K_VOICE_SYNC = 7, K_VOICE = 8 };
enum { T_KIND = 0, T_FN = 1, T_CC = 2, T_DTYPE = 3, T_LC = 4, T_PAYLOAD = 16 };
enum { C_SRC = 0, C_DST = 3, C_FLCO = 6, C_FID = 7, C_CC = 8, C_ALIAS = 9 };
enum { FLCO_TALKER_ALIAS_HEADER = 4 };   // blocks 1..3 follow: 5, 6, 7

// ---- the two short systematic codes, encoder side ----
// Golay(20,8): data, the 11 remainder bits of the (19,8) code, the overall parity bit (CGolay2087::encode keeps it as byte 0, byte 1, high
// nibble of byte 2)
QRL_HD inline uint32_t golay2087_word(unsigned data)
{
    const uint32_t w = ((uint32_t)data << 11) | poly_rem((uint32_t)data << 11, 18, 11, 0xC75);
    return (w << 1) | (popc32(w) & 1u);
}
// QR(16,7,6): data, the 8 remainder bits of the (15,7) code, the overall parity bit
QRL_HD inline uint32_t qr1676_word(unsigned data)
{
    const uint32_t w = ((uint32_t)data << 8) | poly_rem((uint32_t)data << 8, 14, 8, 0x139);
    return (w << 1) | (popc32(w) & 1u);
}
// CDMRSlotType::getData: the 20 bits go to the ten bits on either side of the sync
QRL_HD inline void slot_type_encode(uint8_t* d, unsigned cc, unsigned dt)
{
    const uint32_t w = golay2087_word(((cc << 4) & 0xF0u) | (dt & 0x0Fu));
    const unsigned s0 = (w >> 12) & 0xFFu, s1 = (w >> 4) & 0xFFu, s2 = (w << 4) & 0xF0u;
    d[12] = (uint8_t)((d[12] & 0xC0u) | ((s0 >> 2) & 0x3Fu));
    d[13] = (uint8_t)((d[13] & 0x0Fu) | ((s0 << 6) & 0xC0u) | ((s1 >> 2) & 0x30u));
    d[19] = (uint8_t)((d[19] & 0xF0u) | ((s1 >> 2) & 0x0Fu));
    d[20] = (uint8_t)((d[20] & 0x03u) | ((s1 << 6) & 0xC0u) | ((s2 >> 2) & 0x3Cu));
}
// CDMREMB::getData with PI clear: the 16 bits go to the eight bits on either side of the embedded field
QRL_HD inline void emb_encode(uint8_t* d, unsigned cc, unsigned lcss)
{
    const unsigned e = ((cc << 4) & 0xF0u) | ((lcss << 1) & 0x06u);
    const uint32_t w = qr1676_word((e >> 1) & 0x7Fu);
    const unsigned e0 = (w >> 8) & 0xFFu, e1 = w & 0xFFu;
    d[13] = (uint8_t)((d[13] & 0xF0u) | ((e0 >> 4) & 0x0Fu));
    d[14] = (uint8_t)((d[14] & 0x0Fu) | ((e0 << 4) & 0xF0u));
    d[18] = (uint8_t)((d[18] & 0xF0u) | ((e1 >> 4) & 0x0Fu));
    d[19] = (uint8_t)((d[19] & 0x0Fu) | ((e1 << 4) & 0xF0u));
}
// CSync::addDMRDataSync / addDMRAudioSync, not duplex: the 48 bits from the low nibble of byte 13 to the high nibble of byte 19
QRL_HD inline void add_sync(uint8_t* d, bool audio)
{
    const uint64_t w = audio ? 0x7F7D5DD57DFDull : 0xD5D7F77FD757ull;
    d[13] = (uint8_t)((d[13] & 0xF0u) | (unsigned)((w >> 44) & 0x0Fu));
    for (int i = 0; i < 5; ++i) d[14 + i] = (uint8_t)(w >> (36 - 8 * i));
    d[19] = (uint8_t)((d[19] & 0x0Fu) | (unsigned)((w << 4) & 0xF0u));
}

// ---- embedded LC: CDMREmbeddedData::setLC + getData(data, n) for one fragment n = 1..4, nothing kept between fragments ----
// The 128-bit matrix: rows 0..6 hold 11, 11, 10, 10, 10, 10, 10 bits of the LC, rows 2..6 the five checksum bits (sum of the nine bytes
// mod 31, high bit first) in column 10, every row its Hamming (16,11,4) parity in columns 11..15; row 7 is the column parity.  Bit j of a
// row word is column j.  The matrix is sent by columns: transmitted bit a is matrix bit 16 a mod 127 (bit 127 stays).
QRL_HD inline unsigned hamming16114_row(unsigned w)   // w: the 11 data bits
{
    for (int p = 0; p < 4; ++p) w |= (popc32(w & h15_mask(p)) & 1u) << (11 + p);
    return w | ((popc32(w) & 1u) << 15);
}
QRL_HD inline void embedded_lc_fragment(const uint8_t* lc9, unsigned n, uint8_t* d)
{
    unsigned sum = 0;
    for (int i = 0; i < 9; ++i) sum += lc9[i];
    const unsigned crc = sum % 31u;
    unsigned row[8], pos = 0, all = 0;
    for (int r = 0; r < 7; ++r) {
        const int nbits = r < 2 ? 11 : 10;
        unsigned w = 0;
        for (int j = 0; j < nbits; ++j, ++pos) w |= rd_bit(lc9, pos) << j;
        if (r >= 2) w |= ((crc >> (6 - r)) & 1u) << 10;
        row[r] = hamming16114_row(w);
        all ^= row[r];
    }
    row[7] = all;
    uint32_t frag = 0;
    for (unsigned a = 32u * (n - 1u); a < 32u * n; ++a) {
        const unsigned b = a == 127u ? 127u : (16u * a) % 127u;
        frag = (frag << 1) | ((row[b >> 4] >> (b & 15u)) & 1u);
    }
    d[14] = (uint8_t)((d[14] & 0xF0u) | (frag >> 28));
    d[15] = (uint8_t)(frag >> 20); d[16] = (uint8_t)(frag >> 12); d[17] = (uint8_t)(frag >> 4);
    d[18] = (uint8_t)((d[18] & 0x0Fu) | ((frag << 4) & 0xF0u));
}

// ---- one record -> one burst ----
QRL_HD inline void encode_record(const uint8_t* rec, uint8_t* burst)
{
    for (int i = 0; i < BURST; ++i) burst[i] = 0;
    const unsigned kind = rec[T_KIND], cc = rec[T_CC], dt = rec[T_DTYPE];
    const uint8_t* pay = rec + T_PAYLOAD;
    if (kind == K_VOICE_SYNC || kind == K_VOICE) {
        // DMRFrame::setVoice: the low nibble of payload byte 13 crosses the 48 middle bits
        for (int i = 0; i < 14; ++i) burst[i] = pay[i];
        burst[13] &= 0xF0u;
        burst[19] = pay[13] & 0x0Fu;
        for (int i = 0; i < 13; ++i) burst[20 + i] = pay[14 + i];
        if (kind == K_VOICE_SYNC) { add_sync(burst, true); return; }
        const unsigned fn = rec[T_FN];
        unsigned lcss = 0;
        if (fn >= 1u && fn <= 4u) { embedded_lc_fragment(rec + T_LC, fn, burst); lcss = fn == 1u ? 1u : fn == 4u ? 2u : 3u; }
        emb_encode(burst, cc, lcss);
        return;
    }
    uint8_t d[12];
    if (kind == K_LC) {
        if (dt != DT_VOICE_LC_HEADER && dt != DT_TERMINATOR_WITH_LC) return;   // CDMRFullLC::encode writes nothing: the reference's burst is undefined
        const uint8_t m = dt == DT_VOICE_LC_HEADER ? 0x96u : 0x99u;
        uint8_t p[3];
        for (int i = 0; i < 9; ++i) d[i] = rec[T_LC + i];
        rs129_parity(d, p);
        d[9] = p[2] ^ m; d[10] = p[1] ^ m; d[11] = p[0] ^ m;   // the reference keeps the parity bytes in reversed order
        bptc_encode(d, burst);
    } else if (kind == K_CSBK || kind == K_DATA_HEADER) {
        for (int i = 0; i < 10; ++i) d[i] = pay[i];
        if (kind == K_DATA_HEADER && (d[0] & 0x0Fu) == 0u) d[9] &= 0xFEu;   // CDMRDataHeader::get on a UDT header
        const unsigned crc = crc_ccitt10(d) ^ (kind == K_CSBK ? 0xA5A5u : 0xCCCCu);
        d[10] = (uint8_t)(crc >> 8); d[11] = (uint8_t)crc;
        bptc_encode(d, burst);
    } else if (kind == K_RATE12) {
        bptc_encode(pay, burst);
    } else if (kind == K_RATE34) {
        trellis_encode(pay, burst);
    } else return;   // K_EMPTY, reserved and unknown kinds: the all-zero frame_end
    slot_type_encode(burst, cc, dt);
    add_sync(burst, false);
}

// ---- the record of voice burst k of a call: DMRControl::getTxAudio as a function of the absolute burst index ----
// FN = k mod 6; superframe s = (k div 6) mod 5 carries the call's own LC (s = 0: no options byte is set on it), the talker-alias header
// (s = 1: options (1 << 6) | (0x1B << 1), alias bytes 0..5) or block s - 1 (alias byte 6 (s - 1) as options, the six bytes behind it).
// The reference builds the alias LCs as CDMRLC(flco, a2, a1), source first, so a1 lands in the destination bytes: the alias bytes stay
// in order.  Alias bytes 25 and 26 are never sent, byte 12 and 18 twice.
QRL_HD inline void voice_call_record(const uint8_t* call, uint64_t k, const uint8_t* voice27, uint8_t* rec)
{
    for (int i = 0; i < TX_REC; ++i) rec[i] = 0;
    const unsigned fn = (unsigned)(k % 6u), s = (unsigned)((k / 6u) % 5u);
    rec[T_KIND] = fn == 0u ? K_VOICE_SYNC : K_VOICE;
    rec[T_FN] = (uint8_t)fn;
    rec[T_CC] = call[C_CC];
    uint8_t* lc = rec + T_LC;
    const uint8_t* ta = call + C_ALIAS;
    if (s == 0u) {
        lc[0] = call[C_FLCO]; lc[1] = call[C_FID]; lc[2] = 0;
        for (int i = 0; i < 3; ++i) { lc[3 + i] = call[C_DST + i]; lc[6 + i] = call[C_SRC + i]; }
    } else if (s == 1u) {
        lc[0] = FLCO_TALKER_ALIAS_HEADER; lc[1] = 0; lc[2] = (1u << 6) | (0x1Bu << 1);
        for (int i = 0; i < 6; ++i) lc[3 + i] = ta[i];
    } else {
        lc[0] = (uint8_t)(FLCO_TALKER_ALIAS_HEADER + s - 1u); lc[1] = 0;
        for (int i = 0; i < 7; ++i) lc[2 + i] = ta[6u * (s - 1u) + i];
    }
    for (int i = 0; i < 27; ++i) rec[T_PAYLOAD + i] = voice27[i];
}
}  // namespace dmr
}  // namespace qrl
