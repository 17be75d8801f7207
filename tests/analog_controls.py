"""Shared by tests/test_analog_controls_restatement.py (CPU) and tests/test_gpu_analog_controls.py: the analogue voice receivers under a
working squelch threshold and AGC rates.  Signals (sig.fade_envelope on sig.make_analog / make_ssb), the cuttings into calls, the oracle
runs (computed once per case and shared) and the conditions both files assert on the oracle's result before anything is compared:
a future signal change cannot quietly turn these back into tests at the constructor's -140 dB."""
import functools

import numpy as np

import orc
import sig

# receiver -> modem type (include/qrl_hip.h), oracle entry, rate and first-stage decimation of the squelch's input (port 0), the squelch's
# ramp, the audio stage's I : D behind the gate (I = 0: the cessb stretcher's whole chunks of 1024), stream length at 1 Msps,
# drop-out lengths in squelch items (NBFM: the 320-item DECAY keeps the gate open through a short one)
RECEIVERS = {
    "nbfm5000": dict(kind="nbfm", modem=9, fw=5000, rate=20000, decim=50, ramp=320, I=2, D=5, n=400000, dropouts=(150, 400, 700, 1500)),
    "nbfm2500": dict(kind="nbfm", modem=8, fw=2500, rate=20000, decim=50, ramp=320, I=2, D=5, n=400000, dropouts=(150, 400, 700, 1500)),
    "am": dict(kind="am", modem=14, fw=5000, rate=20000, decim=50, ramp=0, I=2, D=5, n=400000, dropouts=(150, 260, 420, 900)),
    "wbfm": dict(kind="wbfm", modem=10, fw=75000, rate=200000, decim=5, ramp=0, I=1, D=25, n=400000, dropouts=(150, 260, 420, 900)),
    "usb": dict(kind="ssb", sb=0, modem=11, fw=2700, rate=8000, decim=125, ramp=0, I=0, D=1, n=1200000, dropouts=(150, 260, 420, 900)),
    "lsb": dict(kind="ssb", sb=1, modem=12, fw=2700, rate=8000, decim=125, ramp=0, I=0, D=1, n=1200000, dropouts=(150, 260, 420, 900)),
}
THRESHOLD = -34.0          # dB: the carriers sit near -26 dB, their fades swing through it, the noise floor is below -70 dB
AN_PREFETCH = 16           # k_an_gate fetches sixteen items ahead of its recursion

# the GUI's integer knobs and what gr_demod_base::set_agc_attack(int) / set_agc_decay(int) make of them (reference src/gr/gr_demod_base.cpp:1420-1461)
AGC_KNOBS = [(-10, -10), (0, 0), (3, 2), (-100, 5), (1, 100)]
# the AGC cases: the gate is open but for the first items of a stream, the drop-outs and the deepest fades, and the middle of every stream,
# carrier and noise, is 90 dB down: a carrier near -116 dB, magnitudes around 1.5e-6, which no gain up to the 65536 clamp brings to the
# reference.  There the gain climbs by decay x reference per item (decay 100 reaches the clamp within 700 - 2700 items), and the return of
# the full carrier drives it below zero (the 10e-5 clamp)
AGC_THRESHOLD = -130.0


def agc_weak(rx):
    n = RECEIVERS[rx]["n"]
    return (3 * n // 8, 3 * n // 4, 3e-5)


def knob_attack(v):
    return np.float32(1.0) if v == 0 else np.float32(1.0) / np.float32(-v) if v < 0 else np.float32(v) * np.float32(20.0)


def knob_decay(v):
    return np.float32(1.0) if v == 0 else np.float32(1.0) / np.float32(-v) if v < 0 else np.float32(v)


def knob_rates(knob):
    return float(knob_attack(knob[0])), float(knob_decay(knob[1]))


ROLES = ("fade", "shut", "open")   # streams 0 / 1 / 2 of every batch; further streams fade, each with its own seed


def stream(rx, b, weak=None, tone=0.0, n=None):
    """Stream b of receiver rx's batch: 'fade' = deep multi-tone fade with drop-outs, 'shut' = the same 26 dB down (never opens at
    THRESHOLD), 'open' = a shallow fade without drop-outs (never closes once open).  Seed, fade and drop-out positions differ per stream.
    weak: a very weak stretch for an AGC to climb on (agc_weak); tone: NBFM with that CTCSS tone under the audio."""
    R = RECEIVERS[rx]
    n = n or R["n"]
    role = ROLES[b] if b < 3 else "fade"
    seed = 11 + b
    if role == "open":
        env = sig.fade_envelope(n, seed, R["rate"], depth=0.3, dropouts=())
    else:
        env = sig.fade_envelope(n, seed, R["rate"], dropouts=R["dropouts"])
    level = 0.05 if role == "shut" else 1.0
    if R["kind"] == "ssb":
        x = sig.make_ssb(n=n, seed=seed, amp=0.08 * level, lsb=bool(R["sb"]), envelope=env)
    elif tone:
        x = nbfm_with_tone(n, seed, tone, 0.05 * level * env)
    else:
        x = sig.make_analog(R["kind"], n=n, seed=seed, amp=0.05 * level, envelope=env)[0]
    if weak:   # (start, stop, factor): that stretch of the finished signal, noise included, scaled down
        x[weak[0]:weak[1]] *= np.float32(weak[2])
    return x


def nbfm_with_tone(n, seed, tone, amp, fs=1000000.0):
    """NBFM carrier of per-sample amplitude `amp` whose audio is a voice-band tone plus a sub-audible CTCSS tone (deviation ~ 15 %)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    a = 0.5 * np.sin(2 * np.pi * 1000.0 * t) + 0.15 * np.sin(2 * np.pi * tone * t)
    ph = 2 * np.pi * 2500.0 * np.cumsum(a) / fs
    x = amp * np.exp(1j * ph) + 0.0005 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=4)
def batch(rx, B=3, weak=None, tone=0.0, n=None):
    iq = np.stack([stream(rx, b, weak=weak, tone=tone, n=n) for b in range(B)])
    iq.setflags(write=False)
    return iq


def oracle(rx, x, **controls):
    R = RECEIVERS[rx]
    if R["kind"] == "ssb":
        return orc.demod_ssb(x, sb=R["sb"], filter_width=R["fw"], **controls)
    return orc.demod_analog(x, R["kind"], filter_width=R["fw"], **controls)


@functools.lru_cache(maxsize=8)
def oracle_batch(rx, B=3, weak=None, tone=0.0, n=None, **controls):
    """the oracle's outputs for every stream of batch(rx, B, ...), computed once and shared (the arrays are read-only)"""
    iq = batch(rx, B, weak, tone, n)
    refs = [oracle(rx, iq[b], **({"ctcss": tone} if tone else {}), **controls) for b in range(B)]
    for r in refs:
        for v in r.values():
            v.setflags(write=False)
    return refs


# ---- cuttings: the sizes of the calls one stream of n samples is fed in
def cutting(name, rx, gate0, n=None):
    """'one': a single call.  'ragged': seeded sizes of 20 000 - 90 000 samples, odd ones among them, one call that lies wholly inside
    the longest stretch for which stream 0's gate is shut and one that ends just behind the opening (gate0 = the oracle's Gate of stream 0: the channel filters delay port 0 against
    the samples, so the place is taken from the oracle's trace, not from the envelope).  'fine': the same sizes, but the 600 squelch items
    around the end of that stretch -- shut, then the opening -- are cut into calls of 3 - 18 items (a few hundred samples; WBFM, five samples
    per item: a few dozen), so transitions fall next to call boundaries and many calls pass nothing."""
    R = RECEIVERS[rx]
    n = n or R["n"]
    if name == "one":
        return [n]
    D = R["decim"]
    t = gate0.transitions
    shut = [(int(b - a), int(a), int(b)) for a, b in zip(t[:-1], t[1:]) if not gate0.passed[a]]     # closed runs between two openings
    _, s0, s1 = max(shut)
    rng = np.random.default_rng(len(rx) * 7 + (5 if name == "fine" else 0))
    cuts, pos = set(), 0
    while pos < n:
        cuts.add(pos)
        pos += int(rng.integers(20000, 90000))
    if name == "ragged":
        q = (s1 - s0) // 4
        cuts |= {(s0 + q) * D + 1, (s1 - q) * D, (s1 + 7) * D + 3}      # shut throughout; then a call that ends seven items after the opening
    else:
        lo, hi = (s1 - 300) * D, (s1 + 300) * D
        cuts = {c for c in cuts if not lo < c < hi}
        pos = lo
        while pos < hi:
            cuts.add(pos)
            pos += int(rng.integers(3, 18)) * D + int(rng.integers(0, D))
        cuts.add(hi)
    edges = sorted(c for c in cuts if 0 <= c < n) + [n]
    return [int(b - a) for a, b in zip(edges[:-1], edges[1:])]


def call_items(rx, sizes):
    """cumulative port-0 item counts at the call boundaries: [0, items after call 0, after call 1, ...]"""
    D = RECEIVERS[rx]["decim"]
    return [0] + [int(orc.lib.orc_decim_count(int(c), 1, D)) for c in np.cumsum(sizes)]


def audio_count(rx, g):
    """audio items delivered once g items have passed the gate (the kernels' an_decim_count): rational resampler I : D, or the stretcher"""
    I, D = RECEIVERS[rx]["I"], RECEIVERS[rx]["D"]
    if I == 0:
        return 1024 * ((g - 2) // 1024) if g >= 2 else 0
    return ((g - 1) * I + I - 1) // D + 1 if g else 0


class Gate:
    """What the squelch did with one stream's port-0 items, from the oracle's item-by-item trace"""

    def __init__(self, rx, filtered, db=THRESHOLD, switch=None):
        self.passed, self.state, self.mute = orc.pwr_squelch_trace(filtered, db, RECEIVERS[rx]["ramp"], switch)
        self.transitions = np.flatnonzero(np.diff(self.passed.astype(np.int8))) + 1          # first item of each new gate position
        flips = np.flatnonzero(np.diff(self.mute.astype(np.int8))) + 1
        self.mute_runs = np.diff(flips)                                                        # lengths of the complete mute-flag runs
        self.cum = np.concatenate([[0], np.cumsum(self.passed)])                               # items passed before item i

    def per_call(self, bounds):
        return [int(self.cum[b1] - self.cum[b0]) for b0, b1 in zip(bounds[:-1], bounds[1:])]

    def near_call_edge(self, bounds):
        """a gate transition within the first or last AN_PREFETCH items of a call"""
        for b0, b1 in zip(bounds[:-1], bounds[1:]):
            t = self.transitions[(self.transitions >= b0) & (self.transitions < b1)]
            if t.size and (np.any(t - b0 < AN_PREFETCH) or np.any(b1 - t <= AN_PREFETCH)):
                return True
        return False


def check_conditions(rx, refs, gates, bounds=None, n=None):
    """The conditions of a chatter case, on the oracle's result (refs = oracle outputs per stream, gates = Gate per stream)"""
    R = RECEIVERS[rx]
    assert max(g.transitions.size for g in gates) >= 6, [g.transitions.size for g in gates]
    if R["kind"] == "nbfm":   # a mute flag that comes back inside a ramp: runs of the flag shorter than the ramp, both polarities
        g = gates[0]
        flips = np.flatnonzero(np.diff(g.mute.astype(np.int8))) + 1
        short = [(int(g.mute[a]), int(b - a)) for a, b in zip(flips[:-1], flips[1:]) if b - a < R["ramp"]]
        assert any(m == 1 for m, _ in short) and any(m == 0 for m, _ in short), short
        # ... and the machine was in DECAY / ATTACK while the flag pointed the other way
        assert np.any((g.state == 3) & ~g.mute) and np.any((g.state == 1) & g.mute)
    t = gates[0].transitions
    opens = [int(b1 - a1) for a1, b1 in zip(t[:-1], t[1:]) if gates[0].passed[a1]]                 # lengths of stream 0's complete openings
    if R["ramp"]:             # the shortest opening there is: an ATTACK that runs straight into its DECAY
        assert min(opens) == 2 * R["ramp"] + 1, opens
    else:                     # shorter than the 419 items the audio resampler looks back (and than one chunk of the SSB stretcher)
        assert min(opens) < 419, opens
    for b, (ref, g) in enumerate(zip(refs, gates)):
        role = ROLES[b] if b < 3 else "fade"
        want = audio_count(rx, int(g.cum[-1]))
        assert ref["audio"].size == want, (b, ref["audio"].size, want)
        if role == "shut":
            assert ref["audio"].size == 0 and g.cum[-1] == 0 and ref["filtered"].size == orc.lib.orc_decim_count(n or R["n"], 1, R["decim"])
        else:
            assert ref["audio"].size >= 1024, (b, ref["audio"].size)
        if role == "open":   # opens once and stays open
            assert g.transitions.size == 1 and g.passed[-1]
    if bounds is not None and len(bounds) > 2:
        live = [g for g in gates if g.transitions.size >= 6]
        assert any(0 in g.per_call(bounds) for g in live), "no call of a chattering stream passes zero items"
        assert any(g.near_call_edge(bounds) for g in live), "no transition near a call boundary"


# ---- the GPU side: feed a batch in calls of the given sizes, collect port 0, port 1 and both counts of every call
def run_calls(dem, iq, sizes, between=None):
    """iq: [B, n] complex64 numpy.  between(k, delivered): called before call k with the port-0 items delivered so far (settings moved while
    receiving).  -> (filtered[b], audio[b], counts[call][b] = (port 0, port 1))"""
    import torch
    B = iq.shape[0]
    dev = torch.from_numpy(np.ascontiguousarray(iq)).cuda()
    filt, aud, counts = [[] for _ in range(B)], [[] for _ in range(B)], []
    pos = delivered = 0
    for k, c in enumerate(sizes):
        if between:
            between(k, delivered)
        part = torch.zeros((B, c + (c & 1)), dtype=dev.dtype, device=dev.device)     # own buffer: 16-byte aligned base, even pitch
        part[:, :c] = dev[:, pos:pos + c]
        out = dem.process(part[:, :c])
        cnt = out["counts"].cpu().numpy()
        f, a = out["filtered"].cpu().numpy(), out["audio"].cpu().numpy()
        for b in range(B):
            filt[b].append(f[b, :cnt[b, 0]].copy())
            aud[b].append(a[b, :cnt[b, 1]].copy())
        counts.append([(int(cnt[b, 0]), int(cnt[b, 1])) for b in range(B)])
        delivered += int(cnt[0, 0])
        pos += c
    return [np.concatenate(v) for v in filt], [np.concatenate(v) for v in aud], counts


def assert_bit_equal(got, want, what):
    """bit-identical up to the sign of an exact zero (x + 0.0 maps -0 to +0), sizes included"""
    got, want = np.asarray(got).view(np.float32) + np.float32(0), np.asarray(want).view(np.float32) + np.float32(0)
    assert got.size == want.size, (what, got.size, want.size)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


# ---- the cases both test files run
CUTTINGS = ("one", "ragged", "fine")


@functools.lru_cache(maxsize=8)
def chatter_case(rx, B=3):
    """-> (iq, refs, gates) of receiver rx at THRESHOLD"""
    refs = oracle_batch(rx, B, squelch=THRESHOLD)
    return batch(rx, B), refs, [Gate(rx, r["filtered"]) for r in refs]


@functools.lru_cache(maxsize=1)
def ctcss_case():
    """NBFM 5000 with set_ctcss(88.5) on 2.5 M samples (two and a half blocks of the tone detector), every stream carrying the tone under its
    fade, in the ragged cutting: the tone gate behind the audio resampler sees an item count that changes from call to call.
    -> (iq, refs, gates of the power squelch, sizes)"""
    n = 2500000
    iq = batch("nbfm5000", 3, None, 88.5, n)
    refs = oracle_batch("nbfm5000", 3, None, 88.5, n, squelch=THRESHOLD)
    gates = [Gate("nbfm5000", r["filtered"]) for r in refs]
    return iq, refs, gates, cutting("ragged", "nbfm5000", gates[0], n)


MOVES = {"up": (THRESHOLD, -24.0), "down": (-24.0, -40.0)}    # set_squelch(db2) on a receiver that ran at db1


@functools.lru_cache(maxsize=4)
def moved_threshold_case(rx, direction):
    """The threshold moved between two calls of the ragged cutting, at the first call boundary behind 45 % of the stream.
    -> (iq, sizes, k, switch_item, refs, gates): set_squelch(db2) comes before call k, when switch_item items of port 0 have been delivered"""
    db1, db2 = MOVES[direction]
    iq, _, gates0 = chatter_case(rx)
    sizes = cutting("ragged", rx, gates0[0])
    bounds = call_items(rx, sizes)
    k = int(np.searchsorted(np.cumsum(sizes), 0.45 * RECEIVERS[rx]["n"])) + 1
    refs = oracle_batch(rx, squelch=db1, squelch_switch=(bounds[k], db2))
    gates = [Gate(rx, r["filtered"], db1, (bounds[k], db2)) for r in refs]
    return iq, sizes, k, bounds[k], refs, gates


def check_moved_threshold(rx, direction, case):
    _, sizes, k, at, refs, gates = case
    db1, db2 = MOVES[direction]
    assert 0 < k < len(sizes) and 0 < at < refs[0]["filtered"].size
    for b, (ref, g) in enumerate(zip(refs, gates)):
        assert ref["audio"].size == audio_count(rx, int(g.cum[-1])), b
        still = Gate(rx, ref["filtered"], db1)          # had the threshold stayed
        assert np.array_equal(still.passed[:at], g.passed[:at])
        assert not np.array_equal(still.passed[at:], g.passed[at:]) or ROLES[b] == "shut", b
    g = gates[2]                                         # the stream that never closes at THRESHOLD
    if direction == "up":     # the gate closes on a signal it had passed
        first = int(g.transitions[0])
        assert g.passed[first:at].all() and not g.passed[at:].all()
    else:                     # shut most of the time before the move; behind it (and the estimate's rise) open for good
        assert g.cum[at] < at // 2 and g.passed[at + 400:].all()


@functools.lru_cache(maxsize=12)
def agc_case(rx, knob, switch_knob=None):
    """AM / SSB at AGC_THRESHOLD on the batch with a noise-only middle; the rates of `knob` from the start, those of `switch_knob` (if any) from the
    first call boundary of the ragged cutting behind 30 % of the stream.  -> (iq, sizes, k, switch_item, refs)"""
    weak = agc_weak(rx)
    iq = batch(rx, 3, weak)
    plain = oracle_batch(rx, 3, weak, squelch=AGC_THRESHOLD)
    sizes = cutting("ragged", rx, Gate(rx, oracle_batch(rx, squelch=THRESHOLD)[0]["filtered"]))
    if switch_knob is None:
        return iq, sizes, None, None, oracle_batch(rx, 3, weak, squelch=AGC_THRESHOLD, agc=knob_rates(knob))
    bounds = call_items(rx, sizes)
    k = int(np.searchsorted(np.cumsum(sizes), 0.30 * RECEIVERS[rx]["n"])) + 1
    a2, d2 = knob_rates(switch_knob)
    refs = oracle_batch(rx, 3, weak, squelch=AGC_THRESHOLD, agc=knob_rates(knob), agc_switch=(bounds[k], a2, d2))
    assert all(r["filtered"].size == p["filtered"].size for r, p in zip(refs, plain))
    return iq, sizes, k, bounds[k], refs


def agc_input(rx, filtered, db=AGC_THRESHOLD):
    """what the receiver's AGC sees: the gated stream (complex for SSB's agc2_cc, its magnitude for AM's agc2_ff), float32 as the oracle computes it"""
    g = orc.pwr_squelch_cc(filtered, db, ramp=0, gate=True)
    if RECEIVERS[rx]["kind"] == "ssb":
        return g
    re, im = g.real.astype(np.float32), g.imag.astype(np.float32)
    return np.sqrt(re * re + im * im)


def agc_restated(x, attack, decay, ref, switch=None, gain=1.0, max_gain=65536.0):
    """agc2_ff (x float32) / agc2_cc (x complex64) restated with numpy float32 scalars, one operation per line as in
    gr-analog/include/gnuradio/analog/agc2.h; switch = (item, attack2, decay2): set_attack_rate / set_decay_rate before that item, gain kept.
    -> (out, times the gain < 0 clamp was taken, times the max-gain clamp was taken, the gain before item `switch[0]`)"""
    f = np.float32
    cc = np.iscomplexobj(x)
    attack, decay, ref, gain, max_gain = f(attack), f(decay), f(ref), f(gain), f(max_gain)
    out = np.empty(x.size, x.dtype)
    low = high = 0
    gain_at = None
    re, im = (x.real.astype(f), x.imag.astype(f)) if cc else (x.astype(f), None)
    with np.errstate(all="ignore"):
        for i in range(x.size):
            if switch is not None and i == switch[0]:
                gain_at, attack, decay = gain, f(switch[1]), f(switch[2])
            if cc:
                o_re, o_im = re[i] * gain, im[i] * gain
                out[i] = complex(o_re, o_im)
                tmp = -ref + np.sqrt(o_re * o_re + o_im * o_im)
                fast = tmp > gain
            else:
                o = re[i] * gain
                out[i] = o
                tmp = -ref + np.abs(o)
                fast = np.abs(tmp) > gain
            rate = attack if fast else decay
            gain = gain - tmp * rate
            if gain < f(0.0):
                gain = f(10e-5)
                low += 1
            if max_gain > f(0.0) and gain > max_gain:
                gain = max_gain
                high += 1
    return out, low, high, gain_at
