"""Shared by tests/test_reset_conditions.py (CPU) and tests/test_gpu_reset.py: a handle is dirtied with a stream A, reset, and then fed a
DIFFERENT stream B; what it gives for B must be what the oracle gives for B alone.  This module builds A and B for every case, cuts them into
calls and runs the oracle, so both files see the same streams.

A differs from B the way a radio that changes mode differs from a new one (builders below): about eight times the level, a carrier a few
hundred Hz beside B's, another payload seed, fed in THREE calls (every two-slot ring, parity and flip sits on the other buffer) and of a
length that is even, as the ABI asks, but no multiple of the decimation, of the samples per symbol at 1 Msps, of the decoder's 160-symbol
block, of the RSSI block's 2000 or of a frame.  tests/test_reset_conditions.py asserts on the oracle alone that each A leaves state behind
that changes B's output -- a case that passes with no reset at all proves nothing -- and that each A ends where it is meant to."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import analog_controls as ac
import orc
import sig

NB = 3                      # streams per handle, all different
DIRT_LEVEL = 8.0            # A's amplitude over B's
DIRT_SHIFT = 300.0          # Hz: A's carrier beside B's
OFFSET_1M = 1200.0          # the handle's carrier offset at 1 Msps (kept by a reset); the streams are shifted so that the rotator centres B
OPT_OVERLAP, OPT_UNFUSED_DEC2, OPT_INPUT_RESIDENT = 1, 2, 5          # include/qrl_hip.h
CHAN_OPT_LEGACY_TAIL = 2


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _shift(x, hz, fs=1e6):
    """x moved up by hz (float64 phasor, rounded once)"""
    n = np.arange(x.shape[-1])
    return (x * np.exp(2j * np.pi * hz * n / fs)).astype(np.complex64)


def dirt_length(n, bump=0):
    """the largest length <= n that is 502 modulo 1000 (less `bump` thousands): even, and 2 modulo every decimation (25, 50, 100, 125) and every
    samples-per-symbol figure at 1 Msps (4, 10, 50, 100, 250, 500) of the chains; 2 and 5 divide none of the lengths either way round but the 1:2 stages,
    which an even length cannot avoid"""
    m = (n - 502) // 1000 * 1000 + 502 - 1000 * bump
    assert 0 < m <= n
    return m


def three_calls(n, quantum=2):
    """n samples as three calls of different sizes, each a multiple of `quantum` but the last (a stream of fewer than five quanta: one call -- the
    DSSS modulator's single byte of dirt is a million samples)"""
    if n < 5 * quantum:
        return [n]
    a = n // 3 // quantum * quantum + 2 * quantum
    b = n // 5 // quantum * quantum
    c = n - a - b
    assert min(a, b, c) > 0
    return [a, b, c]


def ragged(n, D=1):
    """B's calls: the ragged cuts of test_gpu_front_end_rates.py, scaled to the stream (every size a multiple of 4 samples: an int16 call needs a
    16-byte aligned base) -- 4 samples | 2 D | 58 D (shorter than a front end's edge region) | a third of the stream | 10 D | 700 D and a bit | the rest"""
    def r4(k):
        return (k + 3) // 4 * 4
    c = [4, r4(2 * D), r4(58 * D + 2), r4(n // 3 + 6), r4(10 * D + 2), r4(min(700, n // (8 * D)) * D + 2 * (D // 3) + 2)]
    c.append(n - sum(c))
    assert all(k > 0 and k % 2 == 0 for k in c), c
    return c


def capped_calls(n, chunk, quantum=2, odd=False):
    """n samples in ragged calls of at most `chunk` (a handle with a small max_chunk has small rings: the dirt then laps every one of them, and
    what a reset leaves in a ring lies where the clean stream's first look-back reads); odd: an odd number of calls"""
    q = quantum
    pattern = [chunk // q * q, 2 * q, (chunk - 102) // q * q, 29 * q, chunk // 3 // q * q]
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(pattern[len(sizes) % len(pattern)], n - sum(sizes)))
    if odd and len(sizes) % 2 == 0:
        half = sizes[0] // (2 * q) * q
        sizes[0:1] = [half, sizes[0] - half]
    assert all(k > 0 and k <= chunk for k in sizes) and sum(sizes) == n
    return sizes


def byte_cuts(n):
    """a transmitter's B in ragged calls of whole bytes"""
    c = [1, 3, max(n // 3, 1), 2]
    c = [k for k in c if k > 0]
    while sum(c) >= n:
        c.pop()
    return c + [n - sum(c)]


def quantise(x, scale):
    """[.., n] complex64 -> [.., 2 n] int16 such that float(v) * scale is the nearest representable sample"""
    return np.clip(np.rint(x.view(np.float32) / np.float32(scale)), -32768, 32767).astype(np.int16)


def converted(v, scale):
    return (v.astype(np.float32) * np.float32(scale)).view(np.complex64)


def _bits_equal(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.kind in "fc":
        got, want = got.view(np.float32) + np.float32(0), want.view(np.float32) + np.float32(0)     # test_gpu_parity._compare's rule for the sign of zero
        return got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return got.size == want.size and np.array_equal(got, want)


def assert_same(got, want, what):
    """bit for bit, sizes included (floats: up to the sign of an exact zero)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.size == want.size, (what, got.size, want.size)
    assert _bits_equal(got, want), what


class Case:
    """One handle's A and B.  streams() -> (A, B), each a sequence of NB per-stream arrays; oracle(x, b) -> {port: array} for stream b fed x from a
    fresh start; PORTS: what the GPU test compares."""
    name = kind = None
    nb = NB
    THREADS = False         # the oracle entries that take their settings through orc_set_* globals (analogue controls, zero runs, ...) run one at a time
    SILENT = ()             # ports on which neither B alone nor B behind A delivers an item: the GPU test compares two empty arrays there

    def __repr__(self):
        return self.name

    def refs(self):
        """oracle(B) per stream, computed once (read-only)"""
        if not hasattr(self, "_refs"):
            _, B = self.streams()
            if self.THREADS:                                   # ctypes drops the GIL
                with ThreadPoolExecutor(self.nb) as pool:
                    self._refs = list(pool.map(lambda b: self.oracle_clean(B[b], b), range(self.nb)))
            else:
                self._refs = [self.oracle_clean(B[b], b) for b in range(self.nb)]
            for r in self._refs:
                for v in r.values():
                    v.setflags(write=False)
        return self._refs

    def oracle_clean(self, x, b):
        """the oracle for B as the GPU test expects it: oracle(), but for what a restarting setter lets run on"""
        return self.oracle(x, b)

    def join(self, a, b):
        return np.concatenate([a, b], axis=-1)

    def carried(self, b):
        """-> {port: (what the oracle gives for B behind A with NO reset, what it gives for B alone)}"""
        A, B = self.streams()
        oa, oab, ob = self.oracle(A[b], b), self.oracle(self.join(A[b], B[b]), b), self.refs()[b]
        return {p: (oab[p][oa[p].shape[-1]:] if oab[p].ndim == 1 else oab[p][..., oa[p].shape[-1]:], ob[p]) for p in self.PORTS}


# ---------------------------------------------------------------- receivers (Demod.reset)
_SCOPE_TAPS = None


def scope_items(fe):
    """gr_demod_base::enable_time_domain's 100 ksps items of a 1 Msps front-end signal (test_time_domain_scope_tap_bit_exact)"""
    global _SCOPE_TAPS
    if _SCOPE_TAPS is None:
        _SCOPE_TAPS = orc.low_pass(1, 1000000, 50000, 25000)
    return orc.decim_auto(fe, _SCOPE_TAPS, 10)


def chain_oracle(mode, fe):
    """test_gpu_parity._oracle behind a given 1 Msps front-end signal, plus the 4FSK symbol demodulators and DSSS"""
    if mode == "dmr":
        return orc.demod_dmr(fe)
    if mode == "m17":
        return orc.demod_m17(fe)
    if mode == "dsss":
        return orc.demod_dsss(fe)
    if mode.startswith("2fsk"):
        return orc.demod_2fsk(fe, sps=10, filter_width=2500 if mode.endswith("fm") else 2000, fm=mode.endswith("fm"))
    if mode == "gmsk10k":
        return orc.demod_gmsk(fe, sps=1, filter_width=20000)
    if mode == "gmsk1k":
        return orc.demod_gmsk(fe, sps=10, filter_width=2000)
    if mode == "qpsk250k":
        return orc.demod_qpsk(fe, sps=2, filter_width=160000)
    if mode == "qpsk2k":
        return orc.demod_qpsk(fe, sps=125, filter_width=1300)
    if mode == "4fsk2k":
        return orc.demod_4fsk(fe, sps=5, filter_width=4000, fm=False)
    if mode == "4fsk2kfm":
        return orc.demod_4fsk(fe, sps=5, filter_width=3000, fm=True)
    if mode == "4fsk100k":
        return orc.demod_4fsk(fe, sps=2, filter_width=125000, fm=True)
    if mode == "bpsk1k":
        return orc.demod_bpsk(fe, sps=10)
    raise ValueError(mode)


# mode -> (decimation of the chain's first stage at 1 Msps, samples per channel symbol at 1 Msps, both branches decoded)
CHAIN = {"2fsk1k": (50, 50, True), "2fsk1kfm": (50, 50, True), "gmsk1k": (50, 100, True), "gmsk10k": (25, 10, True), "qpsk250k": (2, 4, False),
         "qpsk2k": (100, 500, False), "4fsk2k": (50, 25, False), "4fsk2kfm": (50, 25, False), "4fsk100k": (2, 2, False), "bpsk1k": (50, 500, True),
         "dmr": (125, 625.0 / 3, False), "m17": (125, 625.0 / 3, False), "dsss": (50, 2500.0 / 13, True)}


class Rx(Case):
    """A digital receiver at 1 Msps.  A and B from sig.make_batch (sig.make_4fsk / make_dsss for the symbol demodulators and DSSS)."""
    kind = "rx"
    THREADS = True
    rate, D = 1000000, 1
    a_sc16 = b_sc16 = False
    sc16_scale = None

    def __init__(self, name, mode, modem, shift=DIRT_SHIFT, bump=0, frames_a=1, frames_b=1, resident=True, pre=(), post=(), scope=False, chunk=0, ring=0):
        self.name, self.mode, self.modem, self.shift, self.bump = name, mode, modem, shift, bump
        # chunk: the handle's max_chunk, A and B in calls no longer than that; ring: items of the decimated rings such a handle has (engine.cpp:
        # pow2_at_least(2 x items of a call + 1024)), which A must lap
        self.chunk, self.ring = chunk, ring
        self.frames_a, self.frames_b, self.resident, self.pre, self.post, self.scope = frames_a, frames_b, resident, tuple(pre), tuple(post), scope
        self.offset = OFFSET_1M
        self.decim, self.sps_1m, two = CHAIN[mode]
        self.PORTS = ("filtered", "constellation", "bits_a") + (("bits_b",) if two else ()) + (("scope",) if scope else ())

    def _raw(self, dirt):
        """[NB, n] at baseband, before the carrier shift"""
        seed, amp = (900, DIRT_LEVEL) if dirt else (300, 1.0)
        if self.mode in ("dmr", "m17"):
            kw = dict(alpha=0.5, dev=2400.0) if self.mode == "m17" else {}
            xs = [sig.make_4fsk(nsym=150 if dirt else 260, seed=seed + 11 + b, amp=0.3 * amp, noise=0.002 * amp, **kw)[0] for b in range(NB)]     # test_gpu_fuzz.py's inputs
        elif self.mode == "dsss":
            rng = np.random.default_rng(seed + 5)
            bits = rng.integers(0, 2, (NB, 16 if dirt else 60), dtype=np.uint8)        # test_dsss_bit_exact's 60 information bits
            with ThreadPoolExecutor(NB) as pool:
                xs = list(pool.map(lambda b: sig.make_dsss(bits[b], seed=seed + b, amp=0.05 * amp, noise=0.0005 * amp, cfo=3.0 * b), range(NB)))
        else:
            return sig.make_batch(self.mode, NB, nframes=self.frames_a if dirt else self.frames_b, device_rate=1000000, seed=seed, amp=0.05 * amp)
        n = min(x.size for x in xs) & ~1
        return np.stack([x[:n] for x in xs])

    @functools.lru_cache(maxsize=None)
    def streams(self):
        a, b = self._raw(True), self._raw(False)
        a = _shift(a, self.offset + self.shift)[:, :dirt_length(a.shape[1], self.bump)]
        return _readonly(np.ascontiguousarray(a), _shift(b, self.offset))

    def cuts(self):
        A, B = self.streams()
        if self.chunk:
            return capped_calls(A.shape[1], self.chunk, odd=True), capped_calls(B.shape[1], self.chunk)
        return three_calls(A.shape[1]), ragged(B.shape[1])

    def oracle(self, x, b):
        fe = orc.frontend(x, self.rate, self.offset)
        out = chain_oracle(self.mode, fe)
        if self.scope:
            out["scope"] = scope_items(fe)
        return out


class RxFrontEnd(Rx):
    """GMSK-10k behind a device-rate front end: test_gpu_front_end_rates.py's input (noise plus a tone, M_OUT outputs per stream at 1 Msps) as B;
    A is other noise and a tone DIRT_SHIFT beside B's at DIRT_LEVEL, 7001 D + 2 samples.  a_sc16 / b_sc16: that stream goes in as int16 IQ."""
    M_A = 7001

    def __init__(self, D, a_sc16=False, b_sc16=False):
        Rx.__init__(self, "gmsk10k-%dM%s" % (D, "-dirt-sc16" if a_sc16 else "-clean-sc16" if b_sc16 else ""), "gmsk10k", 22)
        self.D, self.rate, self.offset, self.a_sc16, self.b_sc16 = D, D * 1000000, 25000.0, a_sc16, b_sc16
        # the int16 scale is a setting a reset keeps: set before A, used by whichever stream goes in as int16 (A: 2.4 + noise of 0.4 fits 8 / 32768)
        self.sc16_scale = np.float32(8.0 / 32768.0) if a_sc16 else np.float32(1.0 / 16384.0) if b_sc16 else None

    @functools.lru_cache(maxsize=None)
    def streams(self):
        import test_gpu_front_end_rates as fr
        D = self.D
        rng = np.random.default_rng(20183)
        noise = (np.float32(0.05) * rng.standard_normal((NB, 2 * fr.M_OUT * D), dtype=np.float32)).view(np.complex64)
        b = fr._input(noise, D, [self.offset] * NB)
        na = self.M_A * D + 2            # even, no multiple of D (D = 10, the int16 dirt: a multiple of 4 samples as well)
        assert na % D and (na % 4 == 0 or not self.a_sc16)
        rng = np.random.default_rng(20184)
        a = (np.float32(0.05 * DIRT_LEVEL) * rng.standard_normal((NB, 2 * na), dtype=np.float32)).view(np.complex64)
        t = np.arange(na) / float(self.rate)
        for s in range(NB):
            f = self.offset + 3000.0 * (s + 1) * (-1) ** s + DIRT_SHIFT
            a[s] += (0.3 * DIRT_LEVEL * np.exp(2j * np.pi * (f * t + 0.2 * s))).astype(np.complex64)
        if self.a_sc16:
            a = converted(quantise(a, self.sc16_scale), self.sc16_scale)
        if self.b_sc16:
            b = converted(quantise(b, self.sc16_scale), self.sc16_scale)
        return _readonly(a, b)

    def cuts(self):
        A, B = self.streams()
        return three_calls(A.shape[1], 4), ragged(B.shape[1], self.D)


RX_CASES = [
    Rx("2fsk1k-default", "2fsk1k", 18, resident=False, frames_b=2),
    Rx("2fsk1k-overlap-on", "2fsk1k", 18, resident=False, frames_b=2, pre=[(OPT_OVERLAP, 1)]),
    Rx("2fsk1k-overlap-off", "2fsk1k", 18, resident=False, frames_b=2, pre=[(OPT_OVERLAP, 0)]),
    Rx("2fsk1k-input-resident", "2fsk1k", 18, resident=False, frames_b=2, pre=[(OPT_INPUT_RESIDENT, 1)]),
    Rx("2fsk1kfm", "2fsk1kfm", 16, frames_b=2),
    Rx("gmsk1k", "gmsk1k", 21, frames_b=2),
    Rx("gmsk10k-1M-scope", "gmsk10k", 22, scope=True),
    RxFrontEnd(4), RxFrontEnd(8), RxFrontEnd(10, a_sc16=True), RxFrontEnd(66, b_sc16=True),
    Rx("qpsk250k", "qpsk250k", 26),
    Rx("qpsk250k-unfused-after-reset", "qpsk250k", 26, post=[(OPT_UNFUSED_DEC2, 1)]),
    Rx("qpsk2k", "qpsk2k", 7, frames_b=2),
    Rx("4fsk2k", "4fsk2k", 3, frames_b=2),
    Rx("4fsk2kfm", "4fsk2kfm", 5, frames_b=2),
    Rx("4fsk100k", "4fsk100k", 27),
    Rx("bpsk1k", "bpsk1k", 24, frames_b=2),
    # small calls, small rings: the dirt laps the decimated rings (s2, s2l, s2f, s2d, s2g, s3, soft), so a ring that a reset forgets holds A where
    # B's first look-back reads
    Rx("2fsk1k-small-calls", "2fsk1k", 18, frames_b=2, chunk=10000, ring=2048),
    Rx("gmsk10k-small-calls", "gmsk10k", 22, chunk=4000, ring=2048),
    Rx("qpsk250k-small-calls", "qpsk250k", 26, chunk=4096, ring=8192),
    Rx("4fsk2k-small-calls", "4fsk2k", 3, frames_a=3, frames_b=2, chunk=10000, ring=2048),
    Rx("bpsk1k-small-calls", "bpsk1k", 24, frames_b=2, chunk=10000, ring=2048),
    Rx("dmr", "dmr", 41),
    Rx("m17", "m17", 40),
    Rx("dsss", "dsss", 25, shift=20.0),
]
RX_CASES[-1].SILENT = ("bits_a", "bits_b")      # 16 + 60 information bits are 152 coded symbols: short of the decoder's first block of 160


# ---------------------------------------------------------------- analogue receivers
class Analog(Case):
    """An analogue receiver on analog_controls' fading streams.  controls: what the oracle chain is built with (squelch, agc, gain, ctcss,
    set_width) and the GPU test sets on the handle before A.  mid: the one setter that is called between A and B INSTEAD of a reset
    ("set_width" or "ctcss"); the oracle chain is the one that setter leaves, from a fresh start."""
    kind = "analog"
    PORTS = ("filtered", "audio")

    def __init__(self, name, rx, n_a, n_b, controls, mid=None, tone=0.0, weak_start=0):
        self.name, self.rx, self.n_a, self.n_b, self.controls, self.mid, self.tone, self.weak_start = name, rx, n_a, n_b, dict(controls), mid, tone, weak_start
        self.R = ac.RECEIVERS[rx]
        self.decim, self.sps_1m = self.R["decim"], None

    @functools.lru_cache(maxsize=None)
    def streams(self):
        weak = (0, self.weak_start, 0.01) if self.weak_start else None        # B's start 40 dB down: under the squelch threshold that A had opened
        b = np.stack([ac.stream(self.rx, s, weak=weak, tone=self.tone, n=self.n_b) for s in (0, 2, 6)])       # fading, shallow fade, fading: every one opens
        na = dirt_length(self.n_a)
        a = np.stack([ac.stream(self.rx, s, tone=0.0 if self.mid == "ctcss" else self.tone, n=self.n_a) for s in (3, 4, 5)])     # other seeds, all of them fading carriers
        a = _shift(a * np.float32(DIRT_LEVEL), DIRT_SHIFT)[:, :na]
        return _readonly(np.ascontiguousarray(a), b)

    def cuts(self):
        A, B = self.streams()
        return three_calls(A.shape[1]), ragged(B.shape[1])

    def oracle(self, x, b):
        c = self.controls
        if self.R["kind"] == "ssb":
            return orc.demod_ssb(x, sb=self.R["sb"], filter_width=self.R["fw"], **c)
        return orc.demod_analog(x, self.R["kind"], filter_width=self.R["fw"], **c)


ANALOG_CASES = [
    # the CTCSS block needs a second of audio before it opens: B is 2.5 s, as in analog_controls.ctcss_case.  A's carriers (8 x 0.05) open the power squelch at -34 dB, the first
    # 60 000 samples of B (40 dB down) do not
    Analog("nbfm5000-ctcss-squelch", "nbfm5000", 300000, 2500000, dict(ctcss=88.5, squelch=ac.THRESHOLD), tone=88.5, weak_start=60000),
    Analog("am-agc", "am", 300000, 400000, dict(squelch=ac.THRESHOLD, agc=ac.knob_rates((3, 2)))),
    Analog("wbfm", "wbfm", 300000, 400000, dict(squelch=ac.THRESHOLD)),
    Analog("usb-gain", "usb", 600000, 700000, dict(squelch=ac.THRESHOLD, gain=0.5)),
    Analog("nbfm5000-set-filter-width", "nbfm5000", 300000, 400000, dict(squelch=ac.THRESHOLD, set_width=4000), mid="set_width"),
    Analog("am-set-filter-width", "am", 300000, 400000, dict(squelch=ac.THRESHOLD, set_width=4000), mid="set_width"),
    Analog("usb-set-filter-width", "usb", 600000, 700000, dict(squelch=ac.THRESHOLD, set_width=2400), mid="set_width"),
    Analog("nbfm5000-set-ctcss", "nbfm5000", 300000, 2500000, dict(ctcss=88.5, squelch=ac.THRESHOLD), mid="ctcss", tone=88.5),
]


# ---------------------------------------------------------------- transmitters (Mod.reset, AMod.reset, Synth.reset)
def back_end(x1, rate, offset):
    """gr_mod_base back end on a 1 Msps stream: rotator, then the interpolator to the device rate (test_gpu_sc16_output.back_end)"""
    y = orc.rotator(x1, orc.phase_inc_to_turn(2 * np.pi * offset / 1000000.0)) if offset != 0.0 else x1
    return orc.tx_interp(y, rate) if rate > 1000000 else y


def to_sc16(x, scale):
    """the float_to_short rule on cf32 samples (test_gpu_sc16_output.conv): (int16 [2 n], clipped components)"""
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return np.clip(r, -32768, 32767).astype(np.int16), int(np.count_nonzero((r > 32767) | (r < -32768)))


class Tx(Case):
    """A digital modulator: A and B are payload bytes of different seeds, A in three calls of an odd total (whole blocks of 3 bytes for M17 / DMR).
    zero_run = (items behind the END of A, count): queued while A runs, it lies wholly in what would be B's time and must not fire there.
    sc16: every call through process_sc16 at that scale, with a clip-count array that a reset leaves registered (the counts keep adding)."""
    kind = "mod"
    PORTS = ("iq",)

    def __init__(self, name, modem, fn, n_a, n_b, rate=0, offset=0.0, bb_gain=1.0, block=1, items_per_block=0, zero_run=None, sc16=None):
        self.name, self.modem, self.fn, self.n_a, self.n_b, self.rate, self.offset, self.bb_gain = name, modem, fn, n_a, n_b, rate, offset, bb_gain
        self.block, self.items_per_block, self.zero_run, self.sc16 = block, items_per_block, zero_run, sc16
        assert n_a % block == 0 and n_b % block == 0

    @functools.lru_cache(maxsize=None)
    def streams(self):
        rng = np.random.default_rng(4000 + self.modem)
        return _readonly(rng.integers(0, 256, (NB, self.n_a), dtype=np.uint8), rng.integers(0, 256, (NB, self.n_b), dtype=np.uint8))

    def cuts(self):
        k = self.block
        a = [c * k for c in three_calls(self.n_a // k, 1)]
        b = [c * k for c in byte_cuts(self.n_b // k)]
        return a, b

    def queued_runs(self):
        """[(stream, T, count)] in the zero-idle block's input items, counted from the handle's first byte"""
        if not self.zero_run:
            return []
        t = self.n_a // self.block * self.items_per_block + self.zero_run[0]
        return [(s, t + 7 * s, self.zero_run[1]) for s in range(NB)]

    def oracle(self, x, b):
        return {"iq": back_end(self.fn(x, self.bb_gain), self.rate, self.offset)}

    def oracle_if_fired(self, b):
        """B alone with the queued run where it would lie had the reset kept it (DMR)"""
        _, B = self.streams()
        return orc.mod_dmr(B[b], bb_gain=self.bb_gain, zero_runs=[(self.zero_run[0] + 7 * b, self.zero_run[1])])


MOD_CASES = [
    Tx("qpsk250k-4M", 26, lambda d, g: orc.mod_qpsk(d), 201, 300, rate=4000000, offset=25000.0),                          # matrix-pipe interpolator
    Tx("qpsk250k-4M-sc16", 26, lambda d, g: orc.mod_qpsk(d), 201, 300, rate=4000000, offset=25000.0, sc16=40000.0),                 # a few hundred components clip
    Tx("gmsk10k-2M", 22, lambda d, g: orc.mod_gmsk(d, sps=10, filter_width=20000), 61, 90, rate=2000000, offset=-12500.0),     # k_tx_interp_c
    Tx("2fsk1k", 18, lambda d, g: orc.mod_2fsk(d, sps=50, filter_width=2000, fm=False), 7, 12),
    Tx("4fsk2kfm", 5, lambda d, g: orc.mod_4fsk(d, sps=25, filter_width=3500, fm=True), 11, 20),
    Tx("bpsk1k", 24, lambda d, g: orc.mod_bpsk(d, sps=500, filter_width=1500), 7, 12),
    Tx("m17", 40, lambda d, g: orc.mod_m17(d, bb_gain=g), 33, 96, bb_gain=0.9, block=3),
    # DMR: 105 bytes are 2100 items at 24 ksps, past the 1439 items of silence of gr_zero_idle_bursts' history; the run is queued for items
    # 3700 - 4100 of the handle's life, which is 1600 - 2000 of B's 2640
    Tx("dmr-zero-run-queued", 41, lambda d, g: orc.mod_dmr(d, bb_gain=g), 105, 132, bb_gain=0.9, block=3, items_per_block=60, zero_run=(1600, 400)),
    Tx("dsss", 25, lambda d, g: orc.mod_dsss(d, bb_gain=g), 1, 2, bb_gain=0.9),
]


def _voice(n, seed, level=1.0):
    """[NB, n] float32 audio at 8 ksps: two tones, noise, an amplitude-modulated tone (test_gpu_sc16_output._audio), each with its own seed"""
    t = np.arange(n) / 8000.0
    rng = np.random.default_rng(seed)
    f = rng.uniform(300.0, 2500.0, 3)
    return (level * np.stack([0.5 * np.sin(2 * np.pi * f[0] * t) + 0.2 * np.sin(2 * np.pi * f[1] * t), rng.uniform(-0.7, 0.7, n),
                              0.6 * np.sin(2 * np.pi * f[2] * t) * rng.uniform(0.2, 1.0, n)])).astype(np.float32)


class ATx(Case):
    """An analogue modulator.  kind: nbfm / am / usb / cw (key down: no audio goes in, A and B are lengths only).  mid_width: qrl_amod_set_filter_width
    between A and B instead of a reset -- the chain restarts, the CTCSS tone source runs on (tone_k0 = A's audio items)."""
    kind = "amod"
    PORTS = ("iq",)
    MODEM = {"nbfm": 9, "am": 14, "usb": 11, "cw": 13}

    def __init__(self, name, mode, n_a, n_b, tone=0.0, rate=0, offset=0.0, mid_width=0, bb_gain=0.75):
        self.name, self.mode, self.n_a, self.n_b, self.tone, self.rate, self.offset, self.mid_width, self.bb_gain = name, mode, n_a, n_b, tone, rate, offset, mid_width, bb_gain
        self.modem = self.MODEM[mode]

    @functools.lru_cache(maxsize=None)
    def streams(self):
        # A drives the AM modulator's rail and AGC and the SSB clipper (1.4 x full scale)
        return _readonly(_voice(self.n_a, 5100 + self.modem, level=2.0), _voice(self.n_b, 5200 + self.modem))

    def cuts(self):
        q = 4 if self.mode == "nbfm" else 1          # NBFM: calls of whole groups of four audio items
        a = [c * q for c in three_calls(self.n_a // q, 1)]
        b = [c * q for c in byte_cuts(self.n_b // q)]
        return a, b

    def oracle_clean(self, x, b):
        return self.oracle(x, b, tone_k0=self.n_a if self.mid_width else 0)

    def oracle(self, x, b, tone_k0=0):
        if self.mode == "nbfm":
            y = orc.mod_nbfm(x, filter_width=5000, bb_gain=self.bb_gain, ctcss=self.tone, set_width=self.mid_width, tone_k0=tone_k0)
        elif self.mode == "am":
            y = orc.mod_am(x, bb_gain=self.bb_gain)
        elif self.mode == "usb":
            y = orc.mod_ssb(x, sb=0, bb_gain=self.bb_gain)
        else:   # gr_mod_ssb(125, 1e6, ., 1000, 0) over sig_source_f(8000, GR_SIN_WAVE, 600, 0.98, 1): test_gpu_tx._cw_reference
            y = orc.mod_ssb(orc.sig_source_sin(8000, 600, 0.98, x.size, k0=0, offset=1.0), sb=0, filter_width=1000, bb_gain=self.bb_gain)
        return {"iq": back_end(y, self.rate, self.offset)}


AMOD_CASES = [
    ATx("nbfm-ctcss", "nbfm", 1004, 2000, tone=88.5),                  # the tone's phase restarts with a reset
    ATx("am", "am", 163, 240),                                        # (the oracle's 4545-tap band-pass at 1 Msps is slow)
    ATx("usb", "usb", 1501, 3 * 1024 + 300),                           # A ends inside a 1024-chunk of the stretcher
    ATx("cw-key-down", "cw", 1501, 3 * 1024 + 300),
    ATx("nbfm-4M", "nbfm", 604, 1200, rate=4000000, offset=25000.0),
    ATx("nbfm-ctcss-set-filter-width", "nbfm", 1004, 2000, tone=88.5, mid_width=4000),
]


def _pcm(N, n, seed, level=1.0):
    """[N, n] int16 FM baseband at 24 ksps (test_gpu_sc16_output._pcm)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return np.stack([(level * rng.uniform(3000, 12000) * np.sin(2 * np.pi * rng.uniform(200, 2500) * t / 24000 + rng.uniform(0, 6))
                      + rng.normal(0, 300, n)).astype(np.int16) for _ in range(N)])


class SynthCase(Case):
    """The MMDVM synthesizer: N channels of int16 per stream.  zero_run as in Tx, in items of gr_zero_idle_bursts' input (25 ksps behind the 25 / 24
    resampler of the multi-carrier graph, 24 ksps in the single-carrier one), on channel N - 1."""
    kind = "synth"
    PORTS = ("iq",)

    def __init__(self, name, N, n_a, n_b, single=False, zero_run=None, bb_gain=1.0):
        self.name, self.N, self.n_a, self.n_b, self.single, self.zero_run, self.bb_gain = name, N, n_a, n_b, single, zero_run, bb_gain

    @functools.lru_cache(maxsize=None)
    def streams(self):
        a = np.stack([_pcm(self.N, self.n_a, 6100 + 10 * self.N + s, level=2.0) for s in range(NB)])
        b = np.stack([_pcm(self.N, self.n_b, 6200 + 10 * self.N + s) for s in range(NB)])
        return _readonly(a, b)

    def cuts(self):
        return three_calls(self.n_a, 1), byte_cuts(self.n_b)

    def queued_runs(self):
        if not self.zero_run:
            return []
        t = (self.n_a if self.single else self.n_a * 25 // 24) + self.zero_run[0]
        return [(s, self.N - 1, t + 7 * s, self.zero_run[1]) for s in range(NB)]

    def oracle(self, x, b):
        return {"iq": orc.mod_mmdvm(x[0], bb_gain=self.bb_gain) if self.single else orc.mod_mmdvm_multi(x)}

    def oracle_if_fired(self, b):
        _, B = self.streams()
        orc.set_zero_runs([(self.N - 1, self.zero_run[0] + 7 * b, self.zero_run[1])])
        try:
            return self.oracle(B[b], b)["iq"]
        finally:
            orc.set_zero_runs(None)


SYNTH_CASES = [
    SynthCase("7-channels", 7, 5001, 6000),
    SynthCase("single-carrier", 1, 5001, 6000, single=True, bb_gain=0.75),
    SynthCase("3-channels-zero-run-queued", 3, 5001, 6000, zero_run=(1500, 750)),
    SynthCase("single-carrier-zero-run-queued", 1, 5001, 6000, single=True, zero_run=(1500, 750)),
]


# ---------------------------------------------------------------- wideband receivers (Channelizer.reset)
class Chan(Case):
    """A wideband receiver.  form 0: the PFB channelizer (M channels on the 25 kHz grid); 1: the frequency-translating bank (N = 7, D = 10);
    2: 64 translating decimators; "single": gr_demod_mmdvm; 3: the per-channel chains alone, fed channel samples through process_channels
    (its "streams" are the channels of ONE wideband signal).  Ports are lists with one array per channel: int16 samples, RSSI tags and, with
    fsk, the 4FSK tail's dibits.  a_sc16: A goes in as int16 IQ.  post: options set behind the reset."""
    kind = "chan"
    CAL = -7.25

    def __init__(self, name, M, form=0, inst_a=2501, inst_b=6000, fsk=False, a_sc16=False, post=(), nb=2, chunk_inst=0, ring=0):
        self.chunk_inst, self.ring = chunk_inst, ring          # calls of at most that many instants; the channel ring r1 of such a handle (chan.cpp: m1)
        self.name, self.M, self.form, self.inst_a, self.inst_b, self.fsk, self.a_sc16, self.post, self.nb = name, M, form, inst_a, inst_b, fsk, a_sc16, tuple(post), nb
        self.PORTS = ("pcm", "rssi") + (("dibits",) if fsk else ())
        self.sc16_scale = np.float32(16.0 / 32768.0) if a_sc16 else None
        self.D = {0: M, 1: 10, 2: 64, "single": 1, 3: 1}[form]          # input samples per instant of the calls' grid
        self.fs = {0: 25000.0 * M, 1: 240000.0, 2: 1600000.0, "single": 250000.0, 3: 25000.0}[form]

    def _wide(self, n, seed, ns):
        import test_gpu_chan as tc
        if self.form == 1:
            return tc._wideband_xl(self.fs, n, seed, ns, [0.0, 25000.0, -50000.0, 75000.0])
        if self.form in ("single", 3):
            return tc._wideband(1, n, seed, ns)                  # FM carriers at 0 Hz
        x = tc._wideband(self.M if self.form == 0 else 64, n, seed, ns)
        if self.fsk:          # true 4FSK carriers (4800 sym/s) on three channels of every stream, as in test_channelizer_64_4fsk_tail_rssi_bit_exact
            M, t = self.M, np.arange(n)
            for s in range(ns):
                for c in (3, M // 2 + 1, M - 2):
                    y, _ = sig.make_4fsk(nsym=int(n / self.fs * 4800) - 2, seed=seed + 10 * s + c, amp=0.4, noise=0.0, fs=self.fs)
                    f0 = c * 25000.0 if c <= M // 2 else (c - M) * 25000.0
                    m = min(n, y.size)
                    x[s, :m] += (y[:m] * np.exp(2j * np.pi * f0 * t[:m] / self.fs)).astype(np.complex64)
        return x

    @functools.lru_cache(maxsize=None)
    def streams(self):
        ns = 6 if self.form == 3 else self.nb
        na, nb_ = self.inst_a * self.D, self.inst_b * self.D
        if self.form in (1, 2):
            na += 2               # even, and off the decimation
        a = _shift(self._wide(na, 7100 + self.M, ns) * np.float32(DIRT_LEVEL), DIRT_SHIFT, self.fs)
        b = self._wide(nb_, 7200 + self.M, ns)
        if self.a_sc16:
            a = converted(quantise(a, self.sc16_scale), self.sc16_scale)
        if self.form == 3:
            a, b = a[None], b[None]
        return _readonly(np.ascontiguousarray(a), np.ascontiguousarray(b))

    def cuts(self):
        A, B = self.streams()
        q = self.M if self.form == 0 else 1 if self.form == 3 else 2
        qa = 4 * q if self.a_sc16 else q          # an int16 call needs a 16-byte aligned base: calls of whole groups of four samples
        assert A.shape[-1] % qa == 0
        if self.chunk_inst:
            return capped_calls(A.shape[-1], self.chunk_inst * self.D, q, odd=True), capped_calls(B.shape[-1], self.chunk_inst * self.D, q)
        a = [c * qa for c in three_calls(A.shape[-1] // qa, 1)]
        nq = B.shape[-1] // q
        b = [c * q for c in (31, 1, 777, 1200)]
        b.append(B.shape[-1] - sum(b))
        assert b[-1] > 0 and nq * q == B.shape[-1]
        return a, b

    def oracle(self, x, b):
        if self.form == 0:
            if self.fsk:
                pcm, rssi, dib = orc.demod_mmdvm_multi_full(x, self.M, cal=self.CAL)
            else:
                pcm, rssi = orc.demod_mmdvm_multi_rssi(x, self.M, cal=self.CAL)
        elif self.form == 1:
            pcm, rssi = orc.demod_mmdvm_xlating(x, self.M, D=10, cal=self.CAL)
        elif self.form == 2:
            pcm, rssi, dib = orc.demod_mmdvm_xlating_bank_4fsk(x, 64, cal=self.CAL)
        elif self.form == 3:
            pcm, rssi, dib = orc.mmdvm_channel_tails(x, cal=self.CAL)
        else:
            pcm, rssi = orc.demod_mmdvm(x, cal=self.CAL)
            pcm, rssi = pcm[None], rssi[None]
        out = {"pcm": list(pcm), "rssi": list(rssi)}
        if self.fsk:
            out["dibits"] = list(dib)
        return out

    def carried(self, b):
        A, B = self.streams()
        oa, oab, ob = self.oracle(A[b], b), self.oracle(self.join(A[b], B[b]), b), self.refs()[b]
        cat = np.concatenate
        return {p: (cat([y[x.size:] for x, y in zip(oa[p], oab[p])]), cat(ob[p])) for p in self.PORTS}

    def refs(self):
        if not hasattr(self, "_refs"):
            _, B = self.streams()
            self._refs = [self.oracle(B[b], b) for b in range(B.shape[0])]
        return self._refs


CHAN_CASES = [
    Chan("pfb-10", 10),
    Chan("pfb-10-dirt-sc16", 10, inst_a=2504, a_sc16=True),
    Chan("pfb-10-small-calls", 10, inst_a=4501, chunk_inst=256, ring=2048),          # the dirt laps the channel ring r1 (3 x 256 + look-back -> 2048 items)
    Chan("pfb-64-4fsk-rssi", 64, fsk=True, inst_b=4000),
    Chan("pfb-64-4fsk-rssi-legacy-tail-after-reset", 64, fsk=True, inst_b=4000, post=[(CHAN_OPT_LEGACY_TAIL, 1)]),
    Chan("xlating-7x10", 7, form=1, inst_a=4801, inst_b=9600),
    Chan("xlating-bank-64", 64, form=2, fsk=True, inst_a=801, inst_b=1800),          # (the oracle runs 64 decimators per stream)
    Chan("single-carrier", 1, form="single", inst_a=25002, inst_b=60000),
    Chan("channel-tails", 1, form=3, fsk=True, inst_b=4000),
]


# ---------------------------------------------------------------- bit-level blocks (Deframer, FrameSync, Rssi) and the spectrum tap's set_fft_size
DEFRAMER_SYNC = {1: [0x89ED, 0xED89, 0x98DE, 0xED77, 0x8CC8, 0x4C8A2B], 2: [0xB5, 0x4C8A2B], 3: [0x89ED, 0xED89, 0x4C8A2B]}      # test_gpu_deframe.SYNC


def _word_bits(w, nb):
    return np.array([(w >> (nb - 1 - k)) & 1 for k in range(nb)], np.uint8)


def _planted(rng, n, type_):
    """test_gpu_deframe._stream: random bits with the deframer's sync words planted at random places"""
    bits = rng.integers(0, 2, n, dtype=np.uint8)
    pos = 5
    while pos + 40 < n:
        w = DEFRAMER_SYNC[type_][rng.integers(0, len(DEFRAMER_SYNC[type_]))]
        nb = 24 if w > 0xFFFF else (8 if w < 0x100 else 16)
        bits[pos:pos + nb] = _word_bits(w, nb)
        pos += int(rng.integers(30, 700))
    return bits


class Bits(Case):
    """Deframer (block = "deframer", arg = its type) or FrameSync (block = "framesync", arg = the modem type).  A ends inside a frame: a sync word
    and the first 19 bits behind it are its last bits.  The oracle carries its state in arrays: state(x, b) runs it over x and returns them."""
    kind = "bits"

    def __init__(self, block, arg):
        self.block, self.arg, self.name = block, arg, "%s-%d" % (block, arg)
        self.PORTS = ("records",) if block == "deframer" else ("records", "activity")

    def _frames(self, rng, nframes):
        import ctypes
        bl = ctypes.c_int()
        cls = orc.lib.orc_modem_sync_geometry(self.arg, ctypes.byref(bl), ctypes.byref(ctypes.c_int()))
        words = {0: [(0xB5, 8)], 1: [(0xDE98AA, 24), (0x98DEAA, 24), (0x4C8A2B, 24)], 2: [(0xED89, 16), (0x89EDAA, 24), (0xED77AA, 24), (0x8CC8DD, 24), (0x4C8A2B, 24)],
                 3: [(0x55F7, 16), (0xFF5D, 16), (0x555D555D, 32)]}[cls]              # test_gpu_deframe._bits_with_frames
        parts = []
        for _ in range(nframes):
            parts.append(rng.integers(0, 2, int(rng.integers(3, 200)), dtype=np.uint8))
            w, nb = words[int(rng.integers(0, len(words)))]
            parts += [_word_bits(w, nb), rng.integers(0, 2, bl.value, dtype=np.uint8)]
        return np.concatenate(parts), words[0]

    @functools.lru_cache(maxsize=None)
    def streams(self):
        rng = np.random.default_rng(8000 + self.arg + (100 if self.block == "deframer" else 0))
        a, b = [], []
        for s in range(NB):
            if self.block == "deframer":
                w = DEFRAMER_SYNC[self.arg][0]
                head, tail, clean = _planted(rng, 1500 + 37 * s, self.arg), _word_bits(w, 16 if w > 0xFF else 8), _planted(rng, 4000, self.arg)
            else:
                head, (w, nb) = self._frames(rng, 2)
                tail, clean = _word_bits(w, nb), np.concatenate([self._frames(rng, 4)[0], rng.integers(0, 2, 50, dtype=np.uint8)])
            a.append(np.concatenate([head, rng.integers(0, 2, 33, dtype=np.uint8), tail, rng.integers(0, 2, 19, dtype=np.uint8)]))
            b.append(clean)
        na, nb_ = min(x.size for x in a), min(x.size for x in b)
        return _readonly(np.stack([x[x.size - na:] for x in a]), np.stack([x[:nb_] for x in b]))          # (A keeps its END)

    def cuts(self):
        A, B = self.streams()
        b = [1, 63, 64, 65, 7, 129]
        return three_calls(A.shape[1], 1), b + [B.shape[1] - sum(b)]

    def run(self, x, st=None):
        """-> (records, bits collected under a held sync, the state arrays)"""
        if self.block == "deframer":
            st = np.zeros(3, np.uint32) if st is None else st
            return orc.deframer(self.arg, x, st), 0, st
        st = orc.ModemSync(self.arg) if st is None else st
        rec = st.feed_raw(x)
        return rec, st.collected, st

    def in_frame(self, b):
        """the oracle's sync_found flag and bit index behind A"""
        st = self.run(self.streams()[0][b])[2]
        st = st if self.block == "deframer" else st.st
        return int(st[1]), int(st[2])

    def oracle(self, x, b):
        rec, act, _ = self.run(x)
        return {"records": rec, "activity": np.array([act], np.int32)}

    def carried(self, b):
        A, B = self.streams()
        st = self.run(A[b])[2]
        rec, act, _ = self.run(B[b], st)
        got = {"records": rec, "activity": np.array([act], np.int32)}
        return {p: (got[p], self.refs()[b][p]) for p in self.PORTS}


BITS_CASES = [Bits("deframer", t) for t in (1, 2, 3)] + [Bits("framesync", m) for m in (18, 22, 26, 40)]

RSSI_STREAMS, RSSI_DIRT, RSSI_CLEAN, RSSI_LEVEL = 70, 2500, 4300, -20.0        # two workgroups; A ends 500 items into a block of 2000 with the IIR charged


@functools.lru_cache(maxsize=None)
def rssi_streams():
    """(A, B) for the RSSI block: A noise at 0.2 - 1.0 per component, B at a fortieth of that with a step up in the middle (test_gpu_side.py's shape)"""
    rng = np.random.default_rng(8500)
    a = np.stack([(0.2 * (1 + b % 5) * (rng.standard_normal(RSSI_DIRT) + 1j * rng.standard_normal(RSSI_DIRT))).astype(np.complex64) for b in range(RSSI_STREAMS)])
    amp = lambda b: np.where(np.arange(RSSI_CLEAN) < 1500 + 37 * b, 0.005 * (1 + b % 5), 0.1)
    b = np.stack([(amp(b) * (rng.standard_normal(RSSI_CLEAN) + 1j * rng.standard_normal(RSSI_CLEAN))).astype(np.complex64) for b in range(RSSI_STREAMS)])
    return _readonly(a, b)


FFT_SIZE, FFT_WINDOW = 1024, 0          # the spectrum tap starts at 1024 bins (Hamming) and is set to 512 with its buffer half filled


@functools.lru_cache(maxsize=None)
def fft_streams():
    """(A, B): a tone plus noise per stream, B's tone elsewhere; A half fills the buffer of FFT_SIZE, B is one frame of the new size and a few samples"""
    rng = np.random.default_rng(8600)
    def tone(n, f):
        t = np.arange(n)
        return np.stack([(0.3 * np.exp(2j * np.pi * (f + 0.11 * b) * t) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64) for b in range(NB)])
    return _readonly(tone(FFT_SIZE // 2, 0.07), tone(FFT_SIZE // 2 + 7, -0.21))
