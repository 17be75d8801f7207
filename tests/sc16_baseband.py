"""Shared by tests/test_sc16_baseband_plan.py (CPU), tests/test_gpu_sc16_baseband.py and tests/test_gpu_sc16_baseband_facade.py: int16 IQ
(sc16) into a receiver WITHOUT a device-rate front end (1 Msps, QRL_OPT_SC16_BASEBAND).  The cut schedule, the receivers (one per reader of
the caller's buffer), their inputs -- tests/sig.py signals quantised to int16 without saturating -- and the oracle runs on the converted
floats np.float32(v) * np.float32(scale), computed once per case and shared.

The schedule (SCHEDULE: samples, format, scale of each call in front of the last one, which takes the rest of the stream):
  * every reader sees a call with n % 4 != 0 (no whole 16-byte pieces per row: the per-output kernels), a 2-sample call, a call shorter than
    any stage's look-back (100 samples; the shortest look-back, k_dec2_fir's, is 130), a row pitch larger than n (every call is a slice
    of the whole stream's tensor), a scale that is no power of two from the sixth call on, and cf32 calls between the int16 ones;
  * an int16 call needs a 16-byte aligned base, so a slice of the stream's tensor is a valid call only at a sample = 0 (mod 4); the call
    behind the one of n = 2 (mod 4) starts at a sample = 2 (mod 4) and is taken from a copy of the stream shifted by two samples.
N_PM, the length of the receivers whose bits start early enough, comes from pm_segments (restated below; the plan test holds the
restatement to decim_plan.hpp's): the shortest stream, under a bound on the call's edge outputs, whose last call gives the 1:50 stage SEGMENTS_WANTED streamed segments per stream,
each of them several turns of a wave's 8 KiB ring at 200 bytes per block -- about 2^17 samples
(tests/host/test_sc16_baseband_plan.cpp evaluates the real split of every call, and which outputs take which route)."""
import functools

import numpy as np

import analog_controls as ac
import orc
import sig

B = 3
SHARED_OFFSET = 1200.0
PS_OFFSETS = [1200.0, -850.0, 400.0]
SCALE0 = np.float32(1.0 / 32768.0)          # the default of qrl_demod_set_sc16_scale
SCALE1 = np.float32(1.0 / 32767.0)          # set between two calls: the multiply rounds
SC16, CF32 = "sc16", "cf32"
# (samples, format, scale) of the calls in front of the last one
SCHEDULE = [(30000, SC16, SCALE0), (100, SC16, SCALE0), (10002, SC16, SCALE0), (2, SC16, SCALE0), (20000, CF32, SCALE0),
            (8192, SC16, SCALE1), (4000, CF32, SCALE1)]
PM_D, PM_NT, PM_LAGS = 50, 419, 9           # the 1:50 first stage: low_pass(1, 1e6, 10e3, 10e3, BH), 9 block lags (pm_kernel_lags)
WAVE_SLOTS = 256 * 4 * 4                     # CUs x workgroups per CU (38 KiB of LDS each) x waves: what launch_decim_pm asks the runtime on an MI355X
SEGMENTS_WANTED = 10


def pm_segments(M, batch, cap, J):
    """(S, nseg) of decim_plan.hpp's pm_segments for mult = 1: the cheapest split of M main outputs per stream, ties to the finer one"""
    best_cost, best_S = None, 16
    n_lo, n_hi = (M + 4095) // 4096, (M + 127) // 128
    nseg = n_lo
    while M > 16 and nseg <= max(n_hi, n_lo):
        S = ((M + nseg - 1) // nseg + 15) // 16 * 16
        units = (M + S - 1) // S * batch
        cost = (units + cap - 1) // cap * (S + J - 1 + 16)
        if best_cost is None or cost <= best_cost:
            best_cost, best_S = cost, S
        nseg += 1
    return best_S, (M + best_S - 1) // best_S


def _stream_length():
    """the shortest stream (a multiple of 4 samples) whose last call is surely cut into SEGMENTS_WANTED segments per stream.  Of the call's outputs
    at most 15 + (J - 1) + (J + 16) lie in front of the first aligned segment (decim_pm_edge_len) and one behind the last whole block"""
    head = sum(k for k, _, _ in SCHEDULE)
    tail = 4
    while pm_segments(tail // PM_D - (2 * PM_LAGS + 31), B, WAVE_SLOTS, PM_LAGS)[1] < SEGMENTS_WANTED:
        tail += 4
    return head + tail


N_PM = _stream_length()
assert abs(N_PM - (1 << 17)) < (1 << 17) // 16
PEAK_MAX = 20000                             # bound on the largest component after quantisation: nothing saturates


def calls(n):
    """[(start, samples, format, scale)] for a stream of n samples (n % 4 == 0): SCHEDULE, then one int16 call with the rest"""
    out, pos = [], 0
    for k, fmt, scale in SCHEDULE:
        out.append((pos, k, fmt, scale))
        pos += k
    assert n % 4 == 0 and n - pos >= 50000 and pos % 4 == 0
    out.append((pos, n - pos, SC16, SCALE1))
    assert any(k % 4 for _, k, f, _ in out if f == SC16) and any(k == 2 for _, k, f, _ in out if f == SC16)
    assert all(s % 4 in (0, 2) for s, _, f, _ in out if f == SC16)
    return out


def placement(n, start, fmt):
    """Where the GPU tests take a call's samples from, given 16-byte aligned tensors: ("plain", start) = a slice of the stream's tensor
    (pitch n samples); ("shifted", start + 2) = a slice of a copy with two samples of padding in front (pitch n + 4) for the int16 calls
    that start at a sample = 2 (mod 4).  Returns (tensor, first sample in it, pitch in samples, byte address of that sample modulo 16)."""
    if fmt == SC16 and start % 4 == 2:
        return "shifted", start + 2, n + 4, (4 * (start + 2)) % 16
    return "plain", start, n, ((4 if fmt == SC16 else 8) * start) % 16


def scales(n):
    """the scale every sample of a stream of n samples is converted with, as a float32 vector over the 2 n int16 components"""
    s = np.empty(2 * n, np.float32)
    for start, k, _, scale in calls(n):
        s[2 * start:2 * (start + k)] = scale
    return s


def quantise(iq):
    """[B, n] complex -> [B, 2 n] int16 at 32768 counts per unit: the signals keep their level (the squelch thresholds theirs) and stay far
    from +-32768 (amplitudes 0.05 - 0.3: 1 600 - 10 000 counts)"""
    f = np.ascontiguousarray(iq, np.complex64).view(np.float32)
    v = np.rint(f * np.float32(32768.0))
    assert 1000 < np.abs(v).max() < PEAK_MAX
    return v.astype(np.int16)


def converted(v):
    """what the oracle (and a cf32 call) is fed: np.float32(v) * np.float32(scale), the scale of the call each sample belongs to"""
    return (v.astype(np.float32) * scales(v.shape[1] // 2)[None, :]).view(np.complex64)


def _shift(x, hz):
    """the signal hz above the tuned centre; the receiver's rotator (-hz) brings it back"""
    n = np.arange(x.size)
    return (x.astype(np.complex128) * np.exp(2j * np.pi * hz * n / 1e6)).astype(np.complex64)


def _digital(mode, nframes=1):
    return lambda b: sig.make_stream(mode, nframes, 1000000, seed=5 + 101 * b, lead=37 * b)[0]


def _dsss(b):
    return sig.make_dsss(np.random.default_rng(50 + b).integers(0, 2, 100, dtype=np.uint8), seed=1 + b, cfo=3.0 * b)


# name -> receiver: modem type (include/qrl_hip.h), the stream of index b at 1 Msps, stream length (None: what the signal gives, cut to a
# multiple of 4), the oracle chain behind orc.frontend, the ports compared, handle options, squelch threshold.  `reader`: the kernel that
# reads the caller's buffer
CASES = {
    "2fsk1k": dict(modem=18, sig=_digital("2fsk1k"), n=N_PM, reader="k_decim_pm 1:50, one lag tile (J = 9)",
                   oracle=lambda x: orc.demod_2fsk(x, sps=10, filter_width=2000), ports=("filtered", "constellation", "bits_a", "bits_b")),
    "2fsk1k_serial": dict(like="2fsk1k", options=(("OPT_OVERLAP", 0),)),
    "2fsk2k": dict(modem=17, sig=_digital("2fsk2k", 2), n=N_PM, reader="1:25 decimator, interp = 1",
                   oracle=lambda x: orc.demod_2fsk(x, sps=5, filter_width=4000), ports=("filtered", "constellation", "bits_a", "bits_b")),
    "gmsk10k": dict(modem=22, sig=_digital("gmsk10k", 3), n=N_PM, reader="k_resamp 2:25",
                    oracle=lambda x: orc.demod_gmsk(x, sps=1, filter_width=20000), ports=("filtered", "constellation", "bits_a", "bits_b")),
    "dmr": dict(modem=41, sig=lambda b: sig.make_4fsk(nsym=700, seed=1 + b)[0], n=N_PM, reader="k_resamp 3:125, its output is port 0",
                oracle=lambda x: orc.demod_dmr(x), ports=("filtered", "constellation", "bits_a")),
    "qpsk250k": dict(modem=26, sig=_digital("qpsk250k", 3), n=N_PM, reader="k_dec2_fir",
                     oracle=lambda x: orc.demod_qpsk(x, sps=2, filter_width=160000), ports=("filtered", "constellation", "bits_a")),
    "qpsk250k_unfused": dict(like="qpsk250k", options=(("OPT_UNFUSED_DEC2", 1),), reader="1:2 decimator (k_decim)"),
    "qpsk2k": dict(modem=7, sig=_digital("qpsk2k", 2), n=N_PM, reader="k_decim_pm 1:100 with 3 621 taps, three lag tiles",
                   oracle=lambda x: orc.demod_qpsk(x, sps=125, filter_width=1300), ports=("filtered", "constellation", "bits_a")),
    "4fsk1kfm": dict(modem=6, sig=_digital("4fsk1kfm"), n=N_PM, reader="k_decim_plx 1:100 with 837 taps (the pl edge scratch, k_decim_pl_gen)",
                     oracle=lambda x: orc.demod_4fsk(x, sps=10, filter_width=2000, fm=True), ports=("filtered", "constellation", "bits_a")),
    "usb2500": dict(modem=11, sig=lambda b: ac.stream("usb", b, n=400000), n=400000, reader="1:125 decimator", squelch=ac.THRESHOLD,
                    oracle=lambda x: ac.oracle("usb", x, squelch=ac.THRESHOLD), ports=("filtered", "audio")),
    "wbfm": dict(modem=10, sig=lambda b: ac.stream("wbfm", b), n=400000, reader="1:5 decimator", squelch=ac.THRESHOLD,
                 oracle=lambda x: ac.oracle("wbfm", x, squelch=ac.THRESHOLD), ports=("filtered", "audio")),
    "nbfm5000": dict(modem=9, sig=lambda b: ac.stream("nbfm5000", b), n=400000, reader="k_decim_pm 1:50 behind a working squelch",
                     squelch=ac.THRESHOLD, oracle=lambda x: ac.oracle("nbfm5000", x, squelch=ac.THRESHOLD), ports=("filtered", "audio")),
    "bpsk8": dict(modem=25, sig=_dsss, n=None, reader="k_decim_pm 1:50 in front of the DSSS chain",
                  oracle=lambda x: orc.demod_dsss(x), ports=("filtered", "constellation", "bits_a", "bits_b")),
}


def case(name):
    c = dict(CASES[name])
    if "like" in c:
        c = {**CASES[c["like"]], **{k: v for k, v in c.items() if k != "like"}}
    c.setdefault("options", ())
    c.setdefault("squelch", None)
    return c


def base_name(name):
    return CASES[name].get("like", name)


@functools.lru_cache(maxsize=None)
def _stream(name, b):
    return case(name)["sig"](b)      # (shared by the two offset variants of a receiver)


@functools.lru_cache(maxsize=None)
def inputs(name, per_stream):
    """(v [B, 2 n] int16, offsets) of a receiver: its three streams, each shifted to its carrier offset, cut to the case's length, quantised"""
    c = case(base_name(name))
    offsets = PS_OFFSETS if per_stream else [SHARED_OFFSET] * B
    xs = [_shift(_stream(base_name(name), b), offsets[b]) for b in range(B)]
    n = (c["n"] or min(x.size for x in xs)) & ~3
    assert all(x.size >= n for x in xs), (name, [x.size for x in xs], n)
    v = quantise(np.stack([x[:n] for x in xs]))
    v.setflags(write=False)
    return v, tuple(offsets)


@functools.lru_cache(maxsize=None)
def refs(name, per_stream):
    """the oracle's outputs per stream, with the conditions that make a comparison against them mean something"""
    c = case(base_name(name))
    v, offsets = inputs(name, per_stream)
    x = converted(v)
    out = [c["oracle"](orc.frontend(x[b], 1000000, offsets[b])) for b in range(B)]      # (one after another: the oracle's receiver controls are process-wide)
    alive = 0
    for r in out:
        assert r["filtered"].size > 100, name
        if "bits_a" in c["ports"]:
            assert all(r[p].size >= 16 for p in c["ports"] if p.startswith("bits")), (name, {p: r[p].size for p in c["ports"]})
        alive += "audio" in c["ports"] and r["audio"].size > 200
    if "audio" in c["ports"]:      # a WORKING squelch: stream 1 ('shut') never opens at the threshold, the other two deliver audio
        assert alive == 2 and out[1]["audio"].size == 0, (name, [r["audio"].size for r in out])
    return out
