"""The repeater-mode DMR burst sink for the tests: the reference's own gr_dmr_sink / DMRFrame / DMRTiming behind tests/host/dmr_sink_ref.cpp
(load_ref, where the reference is present), the scalar core behind tests/host/dmr_sink_core_shim.cpp (load_core), the scenario set that
tools/make_dmr_sink_golden.py records into tests/golden/ref/dmr_sink.npz, and small helpers the CPU and GPU tests share.  The records are
those of include/qrl_hip.h.  A scenario is a stream of unpacked bits, the sizes of the work() calls it is cut into, what is done between
calls (flush, reset), its rx_time tags and the mailbox size.  The bursts come from the reference's encoders (tests/dmr_rx.py's Stream); the
48 sync bits are replaced by the BS or MS pattern of src/DMR/constants.h:9-12 and a 24-bit CACH built from (AT, TC, LCSS) goes in front."""
import ctypes as C
import os
import subprocess

import numpy as np

import dmr_l2
import dmr_rx
import dmr_tx

ROOT = dmr_l2.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref", "dmr_sink.npz")
REFERENCE, REF_LIB = dmr_l2.REFERENCE, dmr_l2.REF_LIB
STUBS = tuple(os.path.join(ROOT, "tests", "host", d) for d in ("dmr_sink_stub", "dmr_rx_stub", "dmr_ctl_stub"))

FRAME, INFO, STATE_BYTES, BURST_BITS = 40, 16, 160, 288
SYNC = {"ms_data": 0xD5D7F77FD757, "ms_voice": 0x7F7D5DD57DFD, "bs_data": 0xDFF57D75DF5D, "bs_voice": 0x755FD7DF75F7}
FT_DATA, FT_VOICE, FT_VOICE_SYNC = 0, 1, 2
NONE, FLUSH, RESET = 0, 1, 2
RECV_NONE = 0
TIME_PER_SAMPLE = 41667
NSTREAMS = 72
MODE_REPEATER, MODE_DMO = 0, 1
SLOT_REFUSED = 1 << 11


def end_bit(info):
    return int.from_bytes(bytes(np.asarray(info, np.uint8)[8:16]), "little")


# ------------------------------------------------------------------------------------------------------------------ the reference, the core
def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Ref:
    def __init__(self, lib):
        self.lib = lib
        u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        lib.ref_dmr_sink_new.restype = C.c_void_p
        for n in ("free", "reset", "flush"):
            getattr(lib, "ref_dmr_sink_" + n).argtypes = [C.c_void_p]
            getattr(lib, "ref_dmr_sink_" + n).restype = None
        lib.ref_dmr_sink_work.argtypes = [C.c_void_p, u8p, C.c_int, u64p, u64p, C.POINTER(C.c_double), C.c_int, u8p, u8p, C.c_int, u64p,
                                          C.POINTER(C.c_int)]
        lib.ref_dmr_sink_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.ref_dmr_sink_state.restype = None
        lib.ref_dmr_rxs_new.restype = C.c_void_p
        lib.ref_dmr_rxs_new.argtypes = [C.c_int] * 5
        lib.ref_dmr_rxs_set.argtypes = [C.c_void_p] + [C.c_int] * 4
        lib.ref_dmr_rxs_set.restype = None
        lib.ref_dmr_rxs_free.argtypes = [C.c_void_p]
        lib.ref_dmr_rxs_free.restype = None
        lib.ref_dmr_rxs_step.argtypes = [C.c_void_p, u8p, u8p, u8p]

    def run_call(self, x):
        """a call-layer scenario (RxScenario) through the reference's DMRControl, one addFrames call per burst -> [n, 128]"""
        h = self.lib.ref_dmr_rxs_new(*x.config[:2], dmr_rx.AUDIO_FEC, *x.config[2:])
        out = np.zeros((len(x.frames), dmr_rx.REC), np.uint8)
        change = {r[0]: r[1:] for r in x.reconfig}
        try:
            for i in range(len(x.frames)):
                if i in change:
                    self.lib.ref_dmr_rxs_set(h, *change[i])
                f, sl, o = np.ascontiguousarray(x.frames[i]), np.ascontiguousarray(x.slots[i]), np.zeros(dmr_rx.REC, np.uint8)
                rc = self.lib.ref_dmr_rxs_step(h, _p(f, C.c_uint8), _p(sl, C.c_uint8), _p(o, C.c_uint8))
                assert rc == 0, "%s, burst %d: the driver's two DMRControl objects disagree (%d)" % (x.name, i, rc)
                out[i] = o
        finally:
            self.lib.ref_dmr_rxs_free(h)
        return out

    def run(self, scn):
        """-> dict: frames [k, 40], info [k, 16], call_of [k] (the call that found the burst), counts [calls], states [calls, 11] (the
        sink's private state after each call), timing [m, 3] (call, slot, value of every set_slot_times)"""
        h = self.lib.ref_dmr_sink_new()
        cap = 64
        frames, info, call_of, counts, states, timing = [], [], [], [], [], []
        tb = np.array([t[0] for t in scn.tags], np.uint64)
        ts = np.array([t[1] for t in scn.tags], np.uint64)
        tf = np.array([t[2] for t in scn.tags], np.float64)
        at, base = 0, 0     # base: the bit offset of the last reset (the tags are given in stream position)
        try:
            for k, n in enumerate(scn.cuts):
                op = scn.ops.get(k, NONE)
                if op == FLUSH:
                    self.lib.ref_dmr_sink_flush(h)
                elif op == RESET:
                    self.lib.ref_dmr_sink_reset(h)
                    base = at
                bits = np.ascontiguousarray(scn.bits[at:at + n]) if n else np.zeros(1, np.uint8)
                f, i = np.zeros((cap, FRAME), np.uint8), np.zeros((cap, INFO), np.uint8)
                tm, ntm = np.zeros((cap, 2), np.uint64), C.c_int(0)
                rel = (tb - np.uint64(base)).astype(np.uint64) if len(tb) else tb
                got = self.lib.ref_dmr_sink_work(h, _p(bits, C.c_uint8), int(n), _p(rel, C.c_uint64), _p(ts, C.c_uint64), _p(tf, C.c_double),
                                                 len(scn.tags), _p(f, C.c_uint8), _p(i, C.c_uint8), cap, _p(tm, C.c_uint64), C.byref(ntm))
                assert got >= 0, "%s, call %d: the reference's sink fed bit by bit disagrees with the one fed whole calls (%d)" % (scn.name, k, got)
                at += n
                frames += list(f[:got])
                info += list(i[:got])
                call_of += [k] * got
                counts.append(got)
                st = np.zeros(11, np.uint32)
                self.lib.ref_dmr_sink_state(h, _p(st, C.c_uint32))
                states.append(st)
                timing += [(k, int(tm[j, 0]), int(tm[j, 1])) for j in range(ntm.value)]
        finally:
            self.lib.ref_dmr_sink_free(h)
        return dict(frames=np.array(frames, np.uint8).reshape(-1, FRAME), info=np.array(info, np.uint8).reshape(-1, INFO),
                    call_of=np.array(call_of, np.int32), counts=np.array(counts, np.int32), states=np.array(states, np.uint32).reshape(-1, 11),
                    timing=np.array(timing, np.uint64).reshape(-1, 3))


def ref_command(so):
    """the compiler call that builds tests/host/dmr_sink_ref.cpp with the reference's sources, unmodified, where they lie"""
    src = [os.path.join(REFERENCE, "src", *p) for p in (("gr", "gr_dmr_sink.cpp"), ("DMR", "dmrframe.cpp"), ("DMR", "dmrtiming.cpp"),
                                                             ("DMR", "dmrcontrol.cpp"))]
    return (["g++", "-std=gnu++17", "-O1", "-w", "-shared", "-fPIC"] + ["-D%s=dmr_sink_ref_%s" % (n, n) for n in dmr_tx.RENAMED]
            + [os.path.join(ROOT, "tests", "host", "dmr_sink_ref.cpp")] + src + ["-I" + s for s in STUBS]
            + ["-I" + REFERENCE, "-I" + os.path.join(REFERENCE, "src", "MMDVM"), "-I" + os.path.join(ROOT, "oracle", "gr_stub"),
               "-o", so, "-L" + os.path.dirname(REF_LIB), "-lqrl_ref", "-Wl,-rpath," + os.path.dirname(REF_LIB)])


def load_ref(build_dir):
    """None where the reference is absent"""
    if not (os.path.isdir(os.path.join(REFERENCE, "src", "MMDVM")) and os.path.isfile(REF_LIB)):
        return None
    so = os.path.join(str(build_dir), "libdmr_sink_ref.so")
    subprocess.check_call(ref_command(so))
    return Ref(C.CDLL(so))


class Core:
    def __init__(self, lib):
        self.lib = lib
        u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
        lib.core_dmr_sink_run.argtypes = [u8p, u8p, C.c_size_t, u8p, u8p, C.c_uint]
        lib.core_dmr_sink_run.restype = C.c_uint
        lib.core_dmr_sink_flush.argtypes = [u8p]
        lib.core_dmr_sink_flush.restype = None
        lib.core_dmr_slot_time.argtypes = [C.c_uint64, u64p, u64p, C.POINTER(C.c_double), C.c_size_t]
        lib.core_dmr_slot_time.restype = C.c_uint64
        lib.core_dmr_slot_time_set.argtypes = [u8p]
        lib.core_dmr_rxs_run.argtypes = [C.c_int] * 5 + [u8p, u8p, u8p, C.c_size_t, u8p, u8p]
        lib.core_dmr_rxs_run.restype = None

    def run_call(self, x, with_slots=True):
        """a call-layer scenario through dmr_rx_core.hpp, its configuration switched where the scenario says -> [n, 128]"""
        state = np.zeros(dmr_rx.STATE_BYTES, np.uint8)
        cuts = [0] + [r[0] for r in x.reconfig] + [len(x.frames)]
        cfgs = [tuple(x.config)] + [tuple(r[1:]) for r in x.reconfig]
        out = np.zeros((len(x.frames), dmr_rx.REC), np.uint8)
        for (a, b), (cc, prom, mode, ts) in zip(zip(cuts[:-1], cuts[1:]), cfgs):
            if b == a:
                continue
            f, sl = np.ascontiguousarray(x.frames[a:b]), np.ascontiguousarray(x.slots[a:b])
            l2, o = np.zeros((b - a, 80), np.uint8), np.zeros((b - a, dmr_rx.REC), np.uint8)
            self.lib.core_dmr_rxs_run(cc, prom, 1 if mode == MODE_REPEATER else 0, ts, dmr_rx.AUDIO_FEC, _p(state, C.c_uint8), _p(f, C.c_uint8),
                                      _p(sl, C.c_uint8) if with_slots else None, b - a, _p(l2, C.c_uint8), _p(o, C.c_uint8))
            out[a:b] = o
        return out

    def call(self, state, bits, cap=64, fill=0):
        """one call on one stream -> (frames [cap, 40], info [cap, 16], found); state: a STATE_BYTES uint8 array, carried"""
        bits = np.ascontiguousarray(bits, np.uint8)
        f, i = np.full((cap, FRAME), fill, np.uint8), np.full((cap, INFO), fill, np.uint8)
        src = bits if bits.size else np.zeros(1, np.uint8)
        got = self.lib.core_dmr_sink_run(_p(state, C.c_uint8), _p(src, C.c_uint8), bits.size, _p(f, C.c_uint8), _p(i, C.c_uint8), cap)
        return f, i, int(got)

    def run(self, scn, cap=None):
        """the scenario through the core, the calls, flushes and resets as the scenario has them -> the dict of Ref.run without states and timing"""
        cap = scn.cap if cap is None else cap
        state = np.zeros(STATE_BYTES, np.uint8)
        frames, info, call_of, counts = [], [], [], []
        at = 0
        for k, n in enumerate(scn.cuts):
            op = scn.ops.get(k, NONE)
            if op == FLUSH:
                self.lib.core_dmr_sink_flush(_p(state, C.c_uint8))
            elif op == RESET:
                state[:] = 0
            f, i, got = self.call(state, scn.bits[at:at + n], cap)
            at += n
            w = min(got, cap)
            frames += list(f[:w])
            info += list(i[:w])
            call_of += [k] * w
            counts.append(got)
        return dict(frames=np.array(frames, np.uint8).reshape(-1, FRAME), info=np.array(info, np.uint8).reshape(-1, INFO),
                    call_of=np.array(call_of, np.int32), counts=np.array(counts, np.int32))

    def slot_time(self, end, tags):
        tb = np.array([t[0] for t in tags], np.uint64)
        ts = np.array([t[1] for t in tags], np.uint64)
        tf = np.array([t[2] for t in tags], np.float64)
        return int(self.lib.core_dmr_slot_time(int(end), _p(tb, C.c_uint64), _p(ts, C.c_uint64), _p(tf, C.c_double), len(tags)))

    def slot_time_set(self, info):
        return bool(self.lib.core_dmr_slot_time_set(_p(np.ascontiguousarray(info, np.uint8), C.c_uint8)))


def load_core(build_dir):
    so = os.path.join(str(build_dir), "libdmr_sink_core.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "dmr_sink_core_shim.cpp"), "-o", so])
    return Core(C.CDLL(so))


# ------------------------------------------------------------------------------------------------------------------ bits on the air
TACT_POS = (0, 4, 8, 12, 14, 18, 22)     # AT, TC, LCSS 1, LCSS 0, the three Hamming (7,4) parities (ETSI TS 102 361-1 9.1.4, B.3.2 by rule)


def cach_bits(at, tc, lcss, fill=0x15A6B):
    """the 24 CACH bits: the TACT at TACT_POS, the 17 payload bits taken from `fill`"""
    ls1, ls0 = (lcss >> 1) & 1, lcss & 1
    tact = (at, tc, ls1, ls0, at ^ tc ^ ls1, tc ^ ls1 ^ ls0, at ^ tc ^ ls0)
    c = np.zeros(24, np.uint8)
    rest = [p for p in range(24) if p not in TACT_POS]
    for j, p in enumerate(rest):
        c[p] = (fill >> j) & 1
    for p, v in zip(TACT_POS, tact):
        c[p] = v
    return c


def word_bits(v, n=48):
    return np.array([(v >> (n - 1 - j)) & 1 for j in range(n)], np.uint8)


def air(burst, sync=None, cach=(0, 0, 0), flip=()):
    """a 33-byte burst -> its 288 bits on the air: CACH, 108 bits, the sync word (sync: a key of SYNC; None keeps the burst's middle 48 bits,
    the EMB and embedded data of voice bursts B..F), 108 bits.  flip: positions 0..287 inverted afterwards"""
    b = np.unpackbits(np.asarray(burst, np.uint8))
    if sync is not None:
        b[108:156] = word_bits(SYNC[sync])
    out = np.concatenate([cach_bits(*cach), b]).astype(np.uint8)
    for p in flip:
        out[p] ^= 1
    return out


class Scenario:
    def __init__(self, name, bits, cuts=None, ops=None, tags=(), cap=64):
        self.name, self.bits, self.ops, self.tags, self.cap = name, np.ascontiguousarray(bits, np.uint8), dict(ops or {}), list(tags), cap
        self.cuts = list(cuts) if cuts is not None else ragged(len(self.bits))
        assert sum(self.cuts) == len(self.bits), name


def ragged(n, sizes=(97, 288, 31, 500, 1, 0, 7, 640, 33, 129)):
    """n bits cut into calls of uneven sizes"""
    out, k = [], 0
    while n > 0:
        c = min(sizes[k % len(sizes)], n)
        out.append(c)
        n -= c
        k += 1
    return out


def has_sync(bits):
    """the positions at which a 48-bit window of bits equals one of the four sync words"""
    bits = np.asarray(bits, np.uint8)
    hits = []
    for v in SYNC.values():
        w = word_bits(v)
        if bits.size >= 48:
            win = np.lib.stride_tricks.sliding_window_view(bits, 48)
            hits += list(np.nonzero((win == w).all(axis=1))[0])
    return sorted(hits)


def quiet(n, seed):
    """n bits with no sync word in them"""
    bits = np.random.RandomState(seed).randint(0, 2, n).astype(np.uint8)
    assert not has_sync(bits)
    return bits


K = dmr_tx
OWN, PRIVATE = dmr_rx.OWN, dmr_rx.PRIVATE


def idle(cc):
    return K.record(K.K_EMPTY, cc=cc, dt=9)


def bursts_of(tx_ref, stream):
    """tests/dmr_rx.py's Stream -> [(33-byte burst, frame type)]"""
    b = tx_ref.bursts(np.stack(stream.tx))
    return [(b[i], stream.ftype[i]) for i in range(len(stream.tx))]


def downlink(ts1, ts2, sourced="bs", lcss=(0, 1, 3, 2), at=(1, 0, 0, 1, 1)):
    """two lists of (burst, frame type) -> the bits of the downlink, TS1 and TS2 alternating, a CACH in front of each burst; a voice burst
    B..F keeps its EMB, the others get the sync word of their kind"""
    out, k = [], 0
    for a, b in zip(ts1, ts2):
        for tc, (burst, ft) in ((0, a), (1, b)):
            sync = None if ft == FT_VOICE else sourced + ("_voice" if ft == FT_VOICE_SYNC else "_data")
            out.append(air(burst, sync, (at[k % len(at)], tc, lcss[k % len(lcss)])))
            k += 1
    return np.concatenate(out)


def build_scenarios(tx_ref):
    S = dmr_rx.Stream
    idles = bursts_of(tx_ref, S("i", 1, 0).add(idle(1), 0).add(idle(1), 0).add(idle(1), 0).add(idle(1), 0))
    call = bursts_of(tx_ref, S("c", 1, 0).header(OWN, 1).superframe(OWN, 1).terminator(OWN, 1))          # header, A..F, terminator
    call2 = bursts_of(tx_ref, S("d", 1, 0).header(PRIVATE, 1).superframe(PRIVATE, 1).terminator(PRIVATE, 1))
    csbk = bursts_of(tx_ref, S("k", 1, 0).csbk(1))[0]
    hdr, voice, term = call[0], call[1:7], call[7]
    s = []
    # 1 a continuous downlink: LC header and terminator on TS1, idle data bursts on TS2
    s.append(Scenario("downlink_header_terminator", downlink([hdr, hdr, term], idles[:3])))
    # 2 a voice superframe A..F on TS1 with data bursts on TS2
    s.append(Scenario("voice_superframe", downlink([hdr] + voice + [term], [csbk] * 8)))
    # 3 voice on both slots, TS1's without its burst A: context 0 finds no sync word in TS1's bursts B..F and searches on through TS2's, while
    # context 1, in the middle of TS2's superframe, gets no bit; TS1's terminator then lets it go on with whatever comes next
    late = voice[1:]
    s.append(Scenario("voice_both_slots", downlink([hdr] + late + [term, hdr, term], call2[1:7] + call2[1:4])))
    # 4 MS-sourced data and voice sync
    ms = [air(hdr[0], "ms_data", (1, 0, 1)), air(voice[0][0], "ms_voice", (0, 1, 2))] + [air(b, None, (1, 1, 3)) for b, _ in voice[1:]]
    ms.append(air(term[0], "ms_data", (0, 0, 0)))
    s.append(Scenario("ms_sourced", np.concatenate(ms)))
    # 5 a TACT with one bit wrong: each parity bit, then a data bit, then a clean one
    bad = [air(csbk[0], "bs_data", (1, k & 1, k & 3), flip=(p,)) for k, p in enumerate((14, 18, 22, 4))] + [air(csbk[0], "bs_data", (1, 1, 2))]
    s.append(Scenario("tact_bit_wrong", np.concatenate(bad)))
    # 6 a sync word with one bit wrong: no burst; the next one is whole
    s.append(Scenario("sync_bit_wrong", np.concatenate([air(hdr[0], "bs_data", (0, 0, 0), flip=(24 + 108 + 17,)), air(term[0], "bs_data", (0, 1, 0)),
                                                        air(csbk[0], "bs_data", (0, 0, 0))])))
    # 7 a sync word that completes at buffered bit 179 (the stream's first bit is missing) against one at 180
    two = np.concatenate([air(hdr[0], "bs_data", (0, 0, 0)), air(csbk[0], "bs_data", (0, 1, 0)), air(term[0], "bs_data", (0, 0, 0))])
    s.append(Scenario("sync_at_179", two[1:]))
    s.append(Scenario("sync_at_180", two))
    # 8 3 x 288 + 300 sync-free bits before the first sync: one call, and many
    long = np.concatenate([quiet(3 * 288 + 300, 8), downlink([hdr, term], idles[:2])])
    s.append(Scenario("long_quiet_one_call", long, cuts=[len(long)]))
    s.append(Scenario("long_quiet_many_calls", long, cuts=ragged(len(long), (37, 288, 5, 101))))
    # 9 calls of 0, 1 and 7 bits across a sync word and across a burst end
    tiny = downlink([hdr, term], idles[:2])
    cuts, left = [], len(tiny)
    for big in (120, 40, 288, 200, 10 ** 6):
        for c in [0, 1, 7] * 6 + [big]:
            c = min(c, left)
            cuts.append(c)
            left -= c
    s.append(Scenario("tiny_calls", tiny, cuts=cuts))
    # 10 cap_frames 2 under a call that finds five bursts
    five = downlink([hdr, hdr, term], idles[:3])[:5 * 288]
    s.append(Scenario("cap_two", five, cuts=[len(five)], cap=2))
    # 11 flush in the middle of a voice burst and in the middle of the search; reset in mid-burst against a fresh handle fed the remainder.
    # (flush in the middle of a data burst: the reference then reads past the end of its buffer; see tests/test_dmr_sink_conditions.py)
    v = downlink(voice + [term], [csbk] * 7)
    s.append(Scenario("flush_mid_voice", v, cuts=[2 * 288 + 100, len(v) - 2 * 288 - 100], ops={1: FLUSH}))
    s.append(Scenario("flush_in_search", two, cuts=[100, len(two) - 100], ops={1: FLUSH}))
    s.append(Scenario("reset_mid_burst", v, cuts=[2 * 288 + 100, len(v) - 2 * 288 - 100], ops={1: RESET}))
    s.append(Scenario("reset_remainder", v[2 * 288 + 100:], cuts=[len(v) - 2 * 288 - 100]))
    # 12 rx_time tags on a symbol's first and second bit
    t = downlink([hdr, hdr, term, hdr], idles[:4])
    s.append(Scenario("tags", t, tags=[(40, 1700000000, 0.25), (288 + 301, 1700000000, 0.28), (3 * 288 + 2, 1700000001, 0.5), (5 * 288 + 287, 1700000002, 0.125)]))
    # the same streams behind d sync-free bits, up to NSTREAMS streams: other positions in the device's tiles and words
    shifted = [x for x in s if x.name in ("downlink_header_terminator", "voice_superframe", "voice_both_slots", "ms_sourced", "tact_bit_wrong",
                                          "long_quiet_many_calls")]
    k = 0
    ops = [x for x in s if x.ops]
    s = [x for x in s if not x.ops]
    while len(s) < NSTREAMS:
        base = shifted[k % len(shifted)]
        d = 1 + 13 * k % 211
        bits = np.concatenate([quiet(d, 100 + k), base.bits])
        s.append(Scenario("%s+%d" % (base.name, d), bits, cuts=ragged(len(bits), (61 + k, 300, 3, 127, 0, 288))))
        k += 1
    # a flush or a reset is the whole handle's: these run alone, behind the NSTREAMS streams that share a handle on the device
    s += ops
    return s


# ------------------------------------------------------------------------------------------------------------------ over the air
RADIO_LEVEL, RADIO_PADS = 0.05, (0, 3, 7)


def radio_rows(g):
    """three streams for the DMR modulator: the bits of downlink_header_terminator as bytes behind 0, 3 and 7 zero bytes, zero bytes behind
    them up to one length (the modulator sends every byte, so the receiver sees the downlink bit for bit) -> [3, n] uint8"""
    x, _ = scenario(g, "downlink_header_terminator")
    body = np.packbits(x.bits)
    n = -(-(max(RADIO_PADS) + body.size + 40) // 72) * 72     # whole 72-byte slots: the modulator takes three bytes at a time
    rows = np.zeros((len(RADIO_PADS), n), np.uint8)
    for k, pad in enumerate(RADIO_PADS):
        rows[k, pad:pad + body.size] = body
    return rows


def sync_slots(bits):
    """the TC bit of the CACH in front of every exact sync word in bits -> list of 0 / 1"""
    return [int(bits[p - 132 + 4]) for p in has_sync(bits) if p >= 132]


# ------------------------------------------------------------------------------------------------------------------ the call layer, repeater mode
class RxScenario:
    """frames [n, 40] and slots [n, 16] as the sink writes them; config (colour code, promiscuous, mode, timeslot); reconfig [(burst, colour
    code, promiscuous, mode, timeslot)]: set before that burst"""

    def __init__(self, name, config, reconfig=()):
        self.name, self.config, self.reconfig = name, tuple(config), [tuple(r) for r in reconfig]
        self.frames, self.slots = np.zeros((0, FRAME), np.uint8), np.zeros((0, INFO), np.uint8)

    def add(self, tx_ref, stream, slot, decoded=1):
        """the bursts of a tests/dmr_rx.py Stream, all on timeslot `slot` (or, a list, one each)"""
        rec = dmr_rx.slicer_records(stream, tx_ref)
        rec[:, 2] = 0                    # the repeater-mode sink leaves the colour code to the slot type
        n = rec.shape[0]
        sl = np.zeros((n, INFO), np.uint8)
        sl[:, 0] = 1
        sl[:, 1] = decoded
        sl[:, 2] = np.where(sl[:, 1] != 0, slot, 0)
        self.frames, self.slots = np.concatenate([self.frames, rec]), np.concatenate([self.slots, sl])
        return self


def interleave(a, b):
    """two RxScenario burst lists burst by burst, a first"""
    n = min(len(a.frames), len(b.frames))
    f, s = [], []
    for i in range(n):
        f += [a.frames[i], b.frames[i]]
        s += [a.slots[i], b.slots[i]]
    f += list(a.frames[n:]) + list(b.frames[n:])
    s += list(a.slots[n:]) + list(b.slots[n:])
    return np.array(f, np.uint8), np.array(s, np.uint8)


def build_rx_scenarios(tx_ref):
    S = dmr_rx.Stream
    R, D = MODE_REPEATER, MODE_DMO
    call_a = lambda cc: S("a", cc, 0).header(OWN, cc).superframe(OWN, cc).terminator(OWN, cc)
    call_b = lambda cc: S("b", cc, 0).header(PRIVATE, cc).superframe(PRIVATE, cc).terminator(PRIVATE, cc)
    out = []
    # 13 a fixed timeslot 1 with calls on both slots
    x = RxScenario("fixed_slot_1_calls_on_both", (1, 0, R, 1))
    x.frames, x.slots = interleave(RxScenario("", ()).add(tx_ref, call_a(1), 1), RxScenario("", ()).add(tx_ref, call_b(1), 2))
    out.append(x)
    # 14 promiscuous: locks to the first slot seen, the terminator lets go, the next call comes on the other slot
    x = RxScenario("promiscuous_slot_lock", (9, 1, R, 1))
    x.frames, x.slots = interleave(RxScenario("", ()).add(tx_ref, call_b(3), 2), RxScenario("", ()).add(tx_ref, call_a(3), 1))
    out.append(x.add(tx_ref, call_a(5), 1).add(tx_ref, call_b(5), 2))
    # 15 an undecoded CACH inside a call
    v = S("v", 1, 0).header(OWN, 1).superframe(OWN, 1).superframe(PRIVATE, 1).terminator(PRIVATE, 1)
    dec = np.ones(len(v.tx), np.uint8)
    dec[[3, 8, 9]] = 0
    out.append(RxScenario("undecoded_cach_in_a_call", (1, 0, R, 1)).add(tx_ref, v, 1, decoded=dec))
    # 16 the order of the checks.  Fixed colour code 1, idle: a voice burst on the right slot passes processTimeslot and is refused by
    # processColorCode (_color_code_RX is 0).  Promiscuous, idle: a voice burst on slot 2 locks the timeslot, the colour code stays 0; a CSBK of
    # colour code 5 on slot 1 then passes processColorCode, which locks 5, and is refused by processTimeslot; one of colour code 7 on slot 2 is
    # refused by processColorCode before the timeslot is asked; a voice burst on slot 1 is refused by processTimeslot before the colour code is asked
    out.append(RxScenario("order_audio_fixed", (1, 0, R, 1)).add(tx_ref, S("o", 1, 0).superframe(OWN, 1, fns=(0, 1)).header(OWN, 1).superframe(OWN, 1, fns=(0, 1)), 1))
    o = RxScenario("order_promiscuous", (1, 1, R, 1)).add(tx_ref, S("o", 1, 1).superframe(OWN, 2, fns=(0,)), 2).add(tx_ref, S("o", 1, 1).csbk(5), 1)
    o.add(tx_ref, S("o", 1, 1).csbk(7), 2).add(tx_ref, S("o", 1, 1).superframe(OWN, 2, fns=(1,)), 1).add(tx_ref, S("o", 1, 1).csbk(5).header(OWN, 5), 2)
    out.append(o.add(tx_ref, S("o", 1, 1).terminator(OWN, 5), 2).add(tx_ref, S("o", 1, 1).header(PRIVATE, 2).terminator(PRIVATE, 2), 1))
    # 17 the mode switched between two calls, the state carried: DMO (the slot records are not asked), then repeater mode on slot 2 with
    # the promiscuous timeslot lock taken in the middle of a call that the switch back to DMO leaves locked
    m = RxScenario("mode_switched", (1, 1, D, 1), reconfig=[(8, 1, 1, R, 2), (12, 1, 1, D, 1), (20, 1, 0, R, 2)])
    m.add(tx_ref, call_a(1), 1, decoded=0).add(tx_ref, S("m", 1, 1).header(PRIVATE, 4).superframe(PRIVATE, 4), 2).add(tx_ref, S("m", 1, 1).terminator(PRIVATE, 4), 1)
    out.append(m.add(tx_ref, call_b(1), 2).add(tx_ref, call_a(1), 1))
    return out


# ------------------------------------------------------------------------------------------------------------------ the golden file
def record_rx_golden(ref, tx_ref):
    scn = build_rx_scenarios(tx_ref)
    n = max(len(x.frames) for x in scn)
    g = dict(rx_names=np.array([x.name for x in scn]), rx_frames=np.zeros((len(scn), n, FRAME), np.uint8), rx_slots=np.zeros((len(scn), n, INFO), np.uint8),
             rx_counts=np.array([len(x.frames) for x in scn], np.int32), rx_config=np.array([x.config for x in scn], np.int32),
             rx_expected=np.zeros((len(scn), n, dmr_rx.REC), np.uint8))
    rc = []
    for k, x in enumerate(scn):
        m = len(x.frames)
        g["rx_frames"][k, :m], g["rx_slots"][k, :m], g["rx_expected"][k, :m] = x.frames, x.slots, ref.run_call(x)
        rc += [(k,) + r for r in x.reconfig]
    g["rx_reconfig"] = np.array(rc, np.int32).reshape(-1, 6)
    return g


def rx_scenario(g, k):
    """call-layer scenario k (an index or a name) of the golden -> (RxScenario, expected [n, 128])"""
    if not isinstance(k, (int, np.integer)):
        k = list(g["rx_names"]).index(k)
    n = int(g["rx_counts"][k])
    x = RxScenario(str(g["rx_names"][k]), [int(v) for v in g["rx_config"][k]], [tuple(int(v) for v in r[1:]) for r in g["rx_reconfig"] if r[0] == k])
    x.frames, x.slots = g["rx_frames"][k, :n], g["rx_slots"][k, :n]
    return x, g["rx_expected"][k, :n]


CHAIN_CONFIG = (1, 1, MODE_REPEATER, 1)     # the tracker behind the NSTREAMS streams of the chained device test: promiscuous, repeater mode


def record_golden(ref, tx_ref):
    g = record_sink_golden(ref, tx_ref)
    g.update(record_rx_golden(ref, tx_ref))
    # the sink's own bursts of the first NSTREAMS streams through the reference's DMRControl: the records of the three-stage chain
    g["chain_call"] = np.zeros((NSTREAMS, g["frames"].shape[1], dmr_rx.REC), np.uint8)
    for k in range(NSTREAMS):
        m = int((g["call_of"][k] >= 0).sum())
        x = RxScenario("chain %d" % k, CHAIN_CONFIG)
        x.frames, x.slots = g["frames"][k, :m], g["info"][k, :m]
        g["chain_call"][k, :m] = ref.run_call(x)
    return g


def record_sink_golden(ref, tx_ref):
    scn = build_scenarios(tx_ref)
    runs = [ref.run(x) for x in scn]
    n = len(scn)
    nb, nc, nf = max(len(x.bits) for x in scn), max(len(x.cuts) for x in scn), max(r["frames"].shape[0] for r in runs)
    g = dict(names=np.array([x.name for x in scn]), bits=np.zeros((n, (nb + 7) // 8), np.uint8), nbits=np.zeros(n, np.int32),
             cuts=np.full((n, nc), -1, np.int32), ops=np.zeros((n, nc), np.uint8), cap=np.zeros(n, np.int32),
             frames=np.zeros((n, nf, FRAME), np.uint8), info=np.zeros((n, nf, INFO), np.uint8), call_of=np.full((n, nf), -1, np.int32),
             counts=np.zeros((n, nc), np.int32), states=np.zeros((n, nc, 11), np.uint32))
    tags, timing = [], []
    for k, (x, r) in enumerate(zip(scn, runs)):
        packed = np.packbits(x.bits)
        g["bits"][k, :packed.size], g["nbits"][k], g["cap"][k] = packed, len(x.bits), x.cap
        g["cuts"][k, :len(x.cuts)] = x.cuts
        for c, op in x.ops.items():
            g["ops"][k, c] = op
        m = r["frames"].shape[0]
        g["frames"][k, :m], g["info"][k, :m], g["call_of"][k, :m] = r["frames"], r["info"], r["call_of"]
        g["counts"][k, :len(x.cuts)], g["states"][k, :len(x.cuts)] = r["counts"], r["states"]
        tags += [(k, t[0], t[1], t[2]) for t in x.tags]
        timing += [(k, int(t[0]), int(t[1]), int(t[2])) for t in r["timing"]]
    g["tag_where"] = np.array([(t[0], t[1], t[2]) for t in tags], np.uint64).reshape(-1, 3)
    g["tag_fracs"] = np.array([t[3] for t in tags], np.float64)
    g["timing"] = np.array(timing, np.uint64).reshape(-1, 4)
    return g


def load_golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def scenario(g, k):
    """scenario k (an index or a name) of the golden -> (Scenario, expected dict like Ref.run's)"""
    if not isinstance(k, (int, np.integer)):
        k = list(g["names"]).index(k)
    cuts = [int(c) for c in g["cuts"][k] if c >= 0]
    ops = {c: int(g["ops"][k, c]) for c in range(len(cuts)) if g["ops"][k, c]}
    tags = [(int(w[1]), int(w[2]), float(f)) for w, f in zip(g["tag_where"], g["tag_fracs"]) if int(w[0]) == k]
    x = Scenario(str(g["names"][k]), np.unpackbits(g["bits"][k])[:int(g["nbits"][k])], cuts, ops, tags, int(g["cap"][k]))
    m = int((g["call_of"][k] >= 0).sum())
    exp = dict(frames=g["frames"][k, :m], info=g["info"][k, :m], call_of=g["call_of"][k, :m], counts=g["counts"][k, :len(cuts)],
               states=g["states"][k, :len(cuts)], timing=np.array([t[1:] for t in g["timing"] if int(t[0]) == k], np.uint64).reshape(-1, 3))
    return x, exp


def written(exp, cap):
    """of the reference's bursts, those a mailbox of cap records per call holds: (frames, info, call_of)"""
    keep = []
    for c in range(len(exp["counts"])):
        keep += list(np.nonzero(exp["call_of"] == c)[0][:cap])
    return exp["frames"][keep], exp["info"][keep], exp["call_of"][keep]
