"""Shared by tests/test_iq8_baseband_conditions.py, tests/test_iq8_baseband_plan.py (CPU), tests/test_gpu_iq8_baseband.py and
tests/test_gpu_iq8_baseband_facade.py: 8-bit IQ (sc8, cu8) into a receiver WITHOUT a device-rate front end (1 Msps, QRL_OPT_IQ8_BASEBAND).
The receivers are those of tests/sc16_baseband.py (CASES, one per reader of the caller's buffer) and so is pm_segments; the cut schedule, the
quantisation to 8 bits and the oracle runs on the converted floats are this file's, computed once per case and shared.

The schedule (SCHEDULE: samples, format, step of each call in front of the last one, which takes the rest of the stream as cu8):
  * both 8-bit formats, each in streamed calls (n % 8 == 0) and in calls the per-output kernels take (n % 8 != 0);
  * a 2-sample call and a 100-sample call, shorter than every stage's look-back (the shortest, k_dec2_fir's, is 130 samples);
  * cf32 and int16 calls between the 8-bit ones -- the handle has QRL_OPT_SC16_BASEBAND and QRL_OPT_IQ8_BASEBAND on;
  * step 0: the case's power-of-two scale with the default cu8 bias 127.5; step 1, from the sixth call on: a scale that is no power of two
    and the cu8 bias BIAS1 = 127.4;
  * a row pitch larger than n (every call is a slice of the whole stream's tensor).
A call needs a 16-byte aligned base: 8 samples of 2 bytes, 4 of 4, 2 of 8.  The 8-bit calls that start at a sample = 4 or 6 (mod 8) are taken
from copies of the stream shifted by 4 and 2 samples (placement()).
Quantisation (levels()): per case a gain -- the largest power of two that keeps the largest component of the three streams at or below 127
counts, so that it lies above 63 -- and the matching scale 1 / gain; in step 1 the gain is 3/4 or 5/4 of that, whichever keeps the peak in
[64, 127], and the scale float32(1 / gain), no power of two.  sc8: v = rint(x gain); cu8: u = rint(x gain + bias); int16: rint(x gain 256)
with the scale / 256.  The signals keep their level (the squelch thresholds theirs) and nothing saturates (asserted).
N_PM, the length of the receivers whose bits start early enough, comes from pm_segments as in tests/sc16_baseband.py: the shortest stream, a
multiple of 8 samples, whose last call gives the 1:50 stage SEGMENTS_WANTED streamed segments per stream
(tests/host/test_iq8_baseband_plan.cpp evaluates the real split of every call)."""
import functools

import numpy as np

import orc
import sc16_baseband as sb
from sc16_baseband import CASES, pm_segments, case, base_name, B, SHARED_OFFSET, PS_OFFSETS, PM_D, PM_NT, PM_LAGS, WAVE_SLOTS, SEGMENTS_WANTED   # noqa: F401

SC8, CU8, SC16, CF32 = "sc8", "cu8", "sc16", "cf32"
BIAS0 = np.float32(127.5)                    # the default of qrl_demod_set_cu8_scale
BIAS1 = np.float32(127.4)                    # set with the second scale
# (samples, format, step) of the calls in front of the last one; step 0: (scale0, BIAS0), step 1: (scale1, BIAS1)
SCHEDULE = [(22000, SC8, 0), (100, CU8, 0), (10002, SC8, 0), (2, CU8, 0), (20000, CF32, 0),
            (8192, CU8, 1), (4000, SC16, 1), (8000, SC8, 1)]
SAMPLE_BYTES = {SC8: 2, CU8: 2, SC16: 4, CF32: 8}


def _stream_length():
    """the shortest stream (a multiple of 8 samples) whose last call is surely cut into SEGMENTS_WANTED segments per stream (the bound of
    tests/sc16_baseband.py on the outputs in front of the first aligned segment and behind the last whole block)"""
    head = sum(k for k, _, _ in SCHEDULE)
    assert head % 8 == 0
    tail = 8
    while pm_segments(tail // PM_D - (2 * PM_LAGS + 31), B, WAVE_SLOTS, PM_LAGS)[1] < SEGMENTS_WANTED:
        tail += 8
    return head + tail


N_PM = _stream_length()
assert N_PM % 8 == 0 and abs(N_PM - (1 << 17)) < (1 << 17) // 8


def length(name):
    """samples per stream of a receiver: N_PM where tests/sc16_baseband.py has its own N_PM, else what it has (400000; None: what the signal gives)"""
    n = case(base_name(name))["n"]
    return N_PM if n == sb.N_PM else n


def calls(n):
    """[(start, samples, format, step)] for a stream of n samples (n % 8 == 0): SCHEDULE, then one cu8 call with the rest"""
    out, pos = [], 0
    for k, fmt, step in SCHEDULE:
        out.append((pos, k, fmt, step))
        pos += k
    assert n % 8 == 0 and n - pos >= 50000 and pos % 8 == 0
    out.append((pos, n - pos, CU8, 1))
    iq8 = [(s, k, f) for s, k, f, _ in out if f in (SC8, CU8)]
    assert {f for _, _, f in iq8} == {SC8, CU8}
    assert any(k % 8 and k > 100 for _, k, _ in iq8) and any(k == 2 for _, k, _ in iq8) and any(k == 100 for _, k, _ in iq8)
    assert any(s % 8 for s, _, _ in iq8) and all(s % 2 == 0 for s, _, _ in iq8)
    assert all(s % 4 == 0 for s, _, f, _ in out if f == SC16) and all(s % 2 == 0 for s, _, f, _ in out if f == CF32)
    assert {f for _, _, f, _ in out} == {SC8, CU8, SC16, CF32}
    return out


def placement(n, start, fmt):
    """Where the GPU tests take a call's samples from, given 16-byte aligned tensors: ("plain", start) = a slice of the stream's tensor (pitch n
    samples); ("shift2" / "shift4" / "shift6", start + shift) = a slice of a copy of the 8-bit stream with that many samples of padding in front
    (pitch n + 8) for the 8-bit calls that start at a sample = 6 / 4 / 2 (mod 8).  Returns (tensor, first sample in it, pitch in samples, byte
    address of that sample modulo 16)."""
    sb_ = SAMPLE_BYTES[fmt]
    if sb_ == 2 and start % 8:
        shift = 8 - start % 8
        return "shift%d" % shift, start + shift, n + 8, (2 * (start + shift)) % 16
    return "plain", start, n, (sb_ * start) % 16


@functools.lru_cache(maxsize=None)
def _floats(name, per_stream):
    """([B, n] complex64, offsets): the three streams of a receiver, each shifted to its carrier offset, cut to the case's length (a multiple of 8)"""
    offsets = PS_OFFSETS if per_stream else [SHARED_OFFSET] * B
    xs = [sb._shift(sb._stream(base_name(name), b), offsets[b]) for b in range(B)]      # (the signals are shared with tests/sc16_baseband.py)
    n = (length(name) or min(x.size for x in xs)) & ~7
    assert all(x.size >= n for x in xs), (name, [x.size for x in xs], n)
    if "1:50" in case(name)["reader"]:
        assert n >= N_PM, (name, n)      # the last call gives the streaming kernel SEGMENTS_WANTED segments per stream
    x = np.stack([x[:n] for x in xs]).astype(np.complex64)
    x.setflags(write=False)
    return x, tuple(offsets)


@functools.lru_cache(maxsize=None)
def levels(name, per_stream):
    """((gain0, scale0), (gain1, scale1)) of a receiver, float32: what the two steps of the schedule quantise and convert with"""
    x, _ = _floats(name, per_stream)
    peak = float(np.abs(x.view(np.float32)).max())
    g0 = 2.0 ** np.floor(np.log2(127.0 / peak))
    assert 63.5 < peak * g0 <= 127.0
    g1 = g0 * (0.75 if peak * g0 >= 96.0 else 1.25)
    for g in (g0, g1):
        assert 64.0 <= peak * g <= 127.0, (name, peak * g)       # the largest component lands between 64 and 127 counts
    s0, s1 = np.float32(1.0 / g0), np.float32(1.0 / g1)
    assert np.frexp(float(s0))[0] == 0.5 and np.frexp(float(s1))[0] != 0.5     # a power of two, then none
    return (np.float32(g0), s0), (np.float32(g1), s1)


def step_settings(name, per_stream, step):
    """(sc8 / cu8 scale, cu8 bias, int16 scale) the handle is given for the calls of a step"""
    _, scale = levels(name, per_stream)[step]
    return float(scale), float(BIAS1 if step else BIAS0), float(np.float32(scale / np.float32(256.0)))


@functools.lru_cache(maxsize=None)
def inputs(name, per_stream):
    """(sc8 [B, 2 n] int8, cu8 [B, 2 n] uint8, sc16 [B, 2 n] int16, converted [B, n] complex64, offsets) of a receiver.  Every sample is
    quantised in all three integer formats with the gain of the call it belongs to; `converted` is what the oracle (and a cf32 call) is fed:
    per sample the conversion of the format its call has -- sc8 float32(v) * scale, cu8 (float32(u) - bias) * scale, int16
    float32(v) * (scale / 256) -- and for the samples of a cf32 call the sc8 conversion."""
    x, offsets = _floats(name, per_stream)
    f = np.ascontiguousarray(x).view(np.float32)
    n = x.shape[1]
    v8, u8, v16, conv = np.empty(f.shape, np.int8), np.empty(f.shape, np.uint8), np.empty(f.shape, np.int16), np.empty(f.shape, np.float32)
    lv = levels(name, per_stream)
    for start, k, fmt, step in calls(n):
        gain, scale = lv[step]
        bias = BIAS1 if step else BIAS0
        sl = slice(2 * start, 2 * (start + k))
        a = np.rint(f[:, sl] * gain)
        u = np.rint(f[:, sl] * gain + bias)
        w = np.rint(f[:, sl] * (gain * np.float32(256.0)))
        assert np.abs(a).max() <= 127 and u.min() >= 0 and u.max() <= 255 and np.abs(w).max() <= 32767      # nothing saturates
        v8[:, sl], u8[:, sl], v16[:, sl] = a.astype(np.int8), u.astype(np.uint8), w.astype(np.int16)
        if fmt == CU8:
            conv[:, sl] = (u8[:, sl].astype(np.float32) - bias) * scale
        elif fmt == SC16:
            conv[:, sl] = v16[:, sl].astype(np.float32) * np.float32(scale / np.float32(256.0))
        else:
            conv[:, sl] = v8[:, sl].astype(np.float32) * scale
    assert 64 <= int(np.abs(v8.astype(np.int32)).max()) <= 127
    for a in (v8, u8, v16, conv):
        a.setflags(write=False)
    return v8, u8, v16, conv.view(np.complex64), offsets


def check_refs(name, out):
    """the conditions tests/sc16_baseband.py's refs() asserts, on this file's oracle outputs: more than 100 filtered items, at least 16 bits on
    every bit port, and a WORKING squelch -- open on exactly streams 0 and 2"""
    c = case(base_name(name))
    alive = 0
    for r in out:
        assert r["filtered"].size > 100, name
        if "bits_a" in c["ports"]:
            assert all(r[p].size >= 16 for p in c["ports"] if p.startswith("bits")), (name, {p: r[p].size for p in c["ports"]})
        alive += "audio" in c["ports"] and r["audio"].size > 200
    if "audio" in c["ports"]:
        assert alive == 2 and out[1]["audio"].size == 0, (name, [r["audio"].size for r in out])


@functools.lru_cache(maxsize=None)
def refs(name, per_stream):
    """the oracle's outputs per stream on the converted floats, with the conditions that make a comparison against them mean something"""
    c = case(base_name(name))
    _, _, _, x, offsets = inputs(name, per_stream)
    out = [c["oracle"](orc.frontend(x[b], 1000000, offsets[b])) for b in range(B)]      # (one after another: the oracle's receiver controls are process-wide)
    check_refs(name, out)
    return out


@functools.lru_cache(maxsize=None)
def whole(name, bias=float(BIAS1)):
    """(sc8 [B, 2 n] int8, cu8 [B, 2 n] uint8, scale, offsets): a receiver's streams (shared offset) quantised with ONE gain, the step-0 one, for
    the callers that keep one setting for the whole stream (the _host entry points, the C++ facade); cu8 with the given bias"""
    x, offsets = _floats(name, False)
    gain, scale = levels(name, False)[0]
    f = np.ascontiguousarray(x).view(np.float32)
    a, u = np.rint(f * gain), np.rint(f * gain + np.float32(bias))
    assert 64 <= np.abs(a).max() <= 127 and u.min() >= 0 and u.max() <= 255      # nothing saturates
    return a.astype(np.int8), u.astype(np.uint8), scale, offsets


def whole_converted(name, fmt, bias=float(BIAS1)):
    """the floats the oracle is fed for whole(): sc8 float32(v) * scale, cu8 (float32(u) - bias) * scale"""
    v8, u8, scale, _ = whole(name, bias)
    f = v8.astype(np.float32) * scale if fmt == SC8 else (u8.astype(np.float32) - np.float32(bias)) * scale
    return f.view(np.complex64)
