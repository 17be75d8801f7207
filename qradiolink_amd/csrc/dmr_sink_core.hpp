// dmr_sink_core.hpp — the repeater-mode DMR burst sink, free of HIP: what the reference's gr_dmr_sink does with the hard bits of port 2 of
// gr_demod_dmr, per stream (reference src/gr/gr_dmr_sink.cpp).
//   one bit                  work()'s loop body, processBits                   src/gr/gr_dmr_sink.cpp:79-139, :171-197
//   the sync search          findSync, countSyncErrs (errs < 1: equality)       :201-271, src/DMR/constants.h:9-13, :90-94
//   the burst                DMRFrame(bits, type), packFrame, setFN             src/DMR/dmrframe.cpp:58-80, :300-303, :370-384
//   the CACH                 DMRFrame::setDownlink                              src/DMR/dmrframe.cpp:255-288
//   flush                    gr_dmr_sink::flush                                 src/gr/gr_dmr_sink.cpp:55-60
// Plain inline functions behind a host / device macro: kernels_dmr_sink.hip calls them one lane per stream, tests/host/dmr_sink_core_shim.cpp
// and tests/host/test_dmr_sink_core.cpp run them on the CPU.
//
// The reference is reproduced as it stands.  There are two slot contexts; a bit goes only to the context _next_slot, which changes hands
// after every burst that context emits, so a context that waits for a sync word keeps the other one's voice call waiting.  The four sync
// words match on equality alone.  A sync word found with fewer than DATA_AND_SYNC_BITS = 180 buffered bits clears the context.
//
// What is kept of _bit_buffer.  While a context searches, the reference appends every bit to its buffer, and work() erases 288 bits at its
// entry once the buffer holds 864 (:163-169).  Of a searching buffer findSync reads two things only: whether it holds at least 180 bits,
// and, if so, its last 180 bits (:238-250).  An erase at 864 leaves at least 576, so it changes neither; in the other states the buffer
// never holds more than 288 bits and the erase does not happen.  So the erase can never change a result, however the bits are cut into
// calls, and the context keeps: a bit count that saturates at SIZE_SAT, and the last 192 + phase search bits as a lazily shifted register
// (sr, the reference's own 64-bit _shift_register, plus five 32-bit groups that move on once in 32 bits).  A searching buffer is always a
// suffix of the bits that went through findSync (a context starts to search with an empty buffer, and flush() only empties it), so at a
// sync word with at least 180 bits the 180 are the last 180 of that register.  From then on the context collects: the 180 bits are laid
// into buf, and the 108 bits that follow, or the 288 of a voice burst, are appended a word at a time, not bit by bit.
//
// After a flush() in the middle of a data or voice-sync burst the reference builds the frame from a buffer shorter than 288 bits and reads
// past its end; here the bits that are missing read as zero.
#pragma once
#include <cstdint>
#include <cstddef>

#if defined(__HIPCC__)
#define QRL_SINK_HD __host__ __device__
#else
#define QRL_SINK_HD
#endif

namespace qrl {
namespace dmr_sink {

enum { FRAME_REC = 40, INFO_REC = 16, BURST_BITS = 288, DATA_AND_SYNC_BITS = 180, PAYLOAD_BITS = 108, SIZE_SAT = 288, STATE_BYTES = 160 };
enum { FT_DATA = 0, FT_VOICE = 1, FT_VOICE_SYNC = 2 };
enum { RECV_NONE = 0, RECV_DATA = 1, RECV_VOICE_SYNC = 2, RECV_VOICE = 3 };
// offsets into the 16-byte slot record
enum { I_DOWNLINK = 0, I_CACH_DECODED = 1, I_SLOT = 2, I_LCSS = 3, I_AT = 4, I_CACH = 5, I_END_BIT = 8 };

constexpr uint64_t MS_DATA_SYNC = 0xD5D7F77FD757ull, MS_VOICE_SYNC = 0x7F7D5DD57DFDull, BS_DATA_SYNC = 0xDFF57D75DF5Dull,
                   BS_VOICE_SYNC = 0x755FD7DF75F7ull, SYNC_MASK = 0xFFFFFFFFFFFFull;

struct dmr_sink_ctx {
    uint64_t sr;          // _shift_register: the last 64 bits that went through findSync
    uint32_t hist[5];     // the 32-bit groups before those: hist[0] the newest; moved on when phase wraps
    uint32_t buf[9];      // _bit_buffer while collecting: bit i in word i >> 5, bit 31 - (i & 31); zero behind `size`
    uint16_t size;        // _bit_buffer.size(); saturates at SIZE_SAT while searching
    uint8_t state, to_receive, frames, uplink, phase, pad;   // _state, _bits_to_receive, _frames_to_receive, !_downlink, search bits since hist moved
};
struct dmr_sink_state {
    dmr_sink_ctx c[2];
    uint64_t total;       // bits consumed since creation or reset
    uint8_t next, pad[7]; // _next_slot
};
static_assert(sizeof(dmr_sink_ctx) == 72 && sizeof(dmr_sink_state) == STATE_BYTES, "the state moves as ten 16-byte words; all zero bytes = a fresh sink");

// the state as the walk holds it: the context the bits go to, and the other one
struct dmr_sink_run { dmr_sink_ctx cur, oth; uint64_t total; unsigned next; };

// a or b, field by field: a whole-struct choice by a run-time flag would be an indexed copy, and the state would leave the registers
QRL_SINK_HD inline dmr_sink_ctx ctx_pick(const dmr_sink_ctx& a, const dmr_sink_ctx& b, bool second)
{
    dmr_sink_ctx c;
    c.sr = second ? b.sr : a.sr;
#pragma GCC unroll 5
    for (int i = 0; i < 5; ++i) c.hist[i] = second ? b.hist[i] : a.hist[i];
#pragma GCC unroll 9
    for (int i = 0; i < 9; ++i) c.buf[i] = second ? b.buf[i] : a.buf[i];
    c.size = second ? b.size : a.size; c.state = second ? b.state : a.state; c.to_receive = second ? b.to_receive : a.to_receive;
    c.frames = second ? b.frames : a.frames; c.uplink = second ? b.uplink : a.uplink; c.phase = second ? b.phase : a.phase; c.pad = 0;
    return c;
}
QRL_SINK_HD inline void run_load(dmr_sink_run& r, const dmr_sink_state& s)
{
    r.next = s.next & 1u; r.total = s.total;
    r.cur = ctx_pick(s.c[0], s.c[1], r.next != 0); r.oth = ctx_pick(s.c[1], s.c[0], r.next != 0);
}
QRL_SINK_HD inline void run_store(const dmr_sink_run& r, dmr_sink_state& s)
{
    s.next = (uint8_t)r.next; s.total = r.total;
    for (int i = 0; i < 7; ++i) s.pad[i] = 0;
    s.c[0] = ctx_pick(r.cur, r.oth, r.next != 0); s.c[1] = ctx_pick(r.oth, r.cur, r.next != 0);
}

QRL_SINK_HD inline void buf_clear(dmr_sink_ctx& c)
{
#pragma GCC unroll 9
    for (int w = 0; w < 9; ++w) c.buf[w] = 0;
    c.size = 0;
}
// gr_dmr_sink::flush() on one context
QRL_SINK_HD inline void ctx_flush(dmr_sink_ctx& c) { buf_clear(c); }

// _bit_buffer.push_back of k bits (1..32) at once: v holds them top-aligned, the first bit in bit 31.  Every word takes its share by a shift, so
// no word is picked by an index.
QRL_SINK_HD inline void buf_append(dmr_sink_ctx& c, uint32_t v, unsigned k)
{
    const int fill = c.size;
#pragma GCC unroll 9
    for (int w = 0; w < 9; ++w) {
        const int d = 32 * w - fill;   // bits from the first new bit to the word's top bit
        uint32_t x = 0;
        if (d <= 0 && d > -32) x = v >> (-d);
        else if (d > 0 && d < 32) x = v << d;
        c.buf[w] |= x;
    }
    c.size = (uint16_t)(fill + (int)k);
}

// the last 180 search bits into buf[0..179] (findSync's erase down to DATA_AND_SYNC_BITS, :246-250)
QRL_SINK_HD inline void buf_from_search(dmr_sink_ctx& c)
{
    const unsigned p = c.phase;
    // the register as eight words, oldest first: 192 + p bits, then zeros
    const uint32_t W[8] = {c.hist[4], c.hist[3], c.hist[2], c.hist[1], c.hist[0], (uint32_t)(c.sr >> p), p ? (uint32_t)c.sr << (32u - p) : 0u, 0u};
    const unsigned o = 12u + p, q = o >> 5, r = o & 31u;   // the 180 start o bits in
#pragma GCC unroll 6
    for (int w = 0; w < 6; ++w) {
        const uint32_t a = q ? W[w + 1] : W[w], b = q ? W[w + 2] : W[w + 1];
        c.buf[w] = r ? (a << r) | (b >> (32u - r)) : a;
    }
    c.buf[5] &= 0xFFFFF000u;
    c.buf[6] = 0; c.buf[7] = 0; c.buf[8] = 0;
    c.size = DATA_AND_SYNC_BITS;
}

// findSync on one bit.  True when the context starts to collect.
QRL_SINK_HD inline bool search_bit(dmr_sink_ctx& c, unsigned bit)
{
    c.sr = (c.sr << 1) | (uint64_t)(bit & 1u);
    if (++c.phase == 32u) {
        c.phase = 0;
        c.hist[4] = c.hist[3]; c.hist[3] = c.hist[2]; c.hist[2] = c.hist[1]; c.hist[1] = c.hist[0];
        c.hist[0] = (uint32_t)(c.sr >> 32);
    }
    if (c.size < SIZE_SAT) ++c.size;
    const uint64_t t = c.sr & SYNC_MASK;
    const bool bs_data = t == BS_DATA_SYNC, ms_data = t == MS_DATA_SYNC, bs_voice = t == BS_VOICE_SYNC, ms_voice = t == MS_VOICE_SYNC;
    if (!(bs_data || ms_data || bs_voice || ms_voice)) return false;
    c.uplink = (bs_data || bs_voice) ? 0 : 1;
    if (c.size < DATA_AND_SYNC_BITS) {
        c.state = RECV_NONE; c.to_receive = 0; c.frames = 0;
        buf_clear(c);
        return false;
    }
    c.state = (bs_data || ms_data) ? RECV_DATA : RECV_VOICE_SYNC;
    buf_from_search(c);
    c.to_receive = PAYLOAD_BITS;
    if (c.state == RECV_VOICE_SYNC) c.frames = 5;
    return true;
}

QRL_SINK_HD inline uint32_t buf_byte(const uint32_t* buf, unsigned k) { return (buf[k >> 2] >> (24u - 8u * (k & 3u))) & 0xFFu; }

// DMRFrame(bits, type) + setFN + setDownlink on a collected buffer: the 40-byte frame record as ten little-endian words, the 16-byte slot
// record as four
QRL_SINK_HD inline void make_records(const uint32_t* buf, unsigned type, unsigned fn, bool downlink, uint64_t end_bit, uint32_t* frame, uint32_t* info)
{
    frame[0] = type | (fn << 8);
#pragma GCC unroll 9
    for (unsigned j = 1; j < 10; ++j) {
        uint32_t w = 0;
#pragma GCC unroll 4
        for (unsigned m = 0; m < 4; ++m) {
            const unsigned i = 4u * j + m;   // record byte i = buffer byte i - 1 for the 33 frame bytes
            if (i <= 36u) w |= buf_byte(buf, i - 1u) << (8u * m);
        }
        frame[j] = w;
    }
    const uint32_t c0 = buf_byte(buf, 0), c1 = buf_byte(buf, 1), c2 = buf_byte(buf, 2);
    uint32_t decoded = 0, slot = 0, lcss = 0, at_out = 0;
    if (downlink) {
        const uint32_t at = (c0 >> 7) & 1u, tc = (c0 >> 3) & 1u, ls1 = (c1 >> 7) & 1u, ls0 = (c1 >> 3) & 1u;
        const uint32_t h0 = at ^ tc ^ ls1, h1 = tc ^ ls1 ^ ls0, h2 = at ^ tc ^ ls0;
        if (h0 == ((c1 >> 1) & 1u) && h1 == ((c2 >> 5) & 1u) && h2 == ((c2 >> 1) & 1u)) {
            decoded = 1; slot = tc ? 2u : 1u; lcss = (ls1 << 1) | ls0; at_out = at;
        }
    }
    info[0] = (downlink ? 1u : 0u) | (decoded << 8) | (slot << 16) | (lcss << 24);
    info[1] = at_out | (c0 << 8) | (c1 << 16) | (c2 << 24);
    info[2] = (uint32_t)end_bit; info[3] = (uint32_t)(end_bit >> 32);
}

// nbits (0..32) bits of the stream, top-aligned in word (the first bit in bit 31), through work()'s loop.  emit(frame words, info words) is
// called for every burst, in order.
template <class Emit>
QRL_SINK_HD inline void sink_bits(dmr_sink_run& r, uint32_t word, unsigned nbits, Emit&& emit)
{
    while (nbits) {
        dmr_sink_ctx& c = r.cur;
        if (c.state == RECV_NONE) {
            search_bit(c, word >> 31);
            word <<= 1; --nbits; ++r.total;
            continue;
        }
        // collecting: the reference only counts here, so the bits are taken as far as the word and the burst go
        const bool voice = c.state == RECV_VOICE;
        const unsigned need = voice ? (unsigned)BURST_BITS - c.size : c.to_receive;
        const unsigned k = need < nbits ? need : nbits;
        buf_append(c, k < 32u ? word & ~(0xFFFFFFFFu >> k) : word, k);
        word = k < 32u ? word << k : 0u;
        nbits -= k; r.total += k;
        if (!voice) c.to_receive = (uint8_t)(c.to_receive - k);
        if (k != need) continue;
        unsigned type, fn = 0;
        if (voice) {
            type = FT_VOICE; fn = 6u - c.frames;
            if (--c.frames == 0) c.state = RECV_NONE;
        } else if (c.state == RECV_DATA) {
            type = FT_DATA; c.state = RECV_NONE;
        } else {
            type = FT_VOICE_SYNC; c.state = RECV_VOICE;
        }
        uint32_t frame[FRAME_REC / 4], info[INFO_REC / 4];
        make_records(c.buf, type, fn, !c.uplink, r.total, frame, info);
        emit(frame, info);
        buf_clear(c);
        const dmr_sink_ctx t = r.cur; r.cur = r.oth; r.oth = t;   // _next_slot = nextSlot(ts_index)
        r.next ^= 1u;
    }
}

}  // namespace dmr_sink
}  // namespace qrl
