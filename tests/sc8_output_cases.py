"""What the sc8 output tests share (test_gpu_sc8_output.py, test_gpu_sc8_tx_rates.py, test_sc8_output_conditions.py): the conversion rule in numpy,
the saturation cases with the oracle's cf32 output, and the preconditions those cases must meet.  Payloads, case tables and oracle outputs are those
of tests/test_gpu_sc16_output.py (computed once per session and shared with it)."""
import functools

import numpy as np

import orc
import sig
import test_gpu_sc16_output as S16

B = S16.B
QPSK250K, GMSK10K, NBFM5000, USB2500 = S16.QPSK250K, S16.GMSK10K, S16.NBFM5000, S16.USB2500


def conv8(x, scale=127.0):
    """complex64 [n] -> (int8 [n, 2], clipped components): r = rint(x * scale), one rounded float32 multiply; saturated to [-128, 127]; NaN -> 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    v = np.where(np.isnan(r), np.float32(0), np.clip(r, -128, 127)).astype(np.int8).reshape(-1, 2)
    return v, int(np.count_nonzero((r > 127) | (r < -128)))


def clip_flags(x, scale=127.0):
    """bool [n, 2]: the components conv8 counts"""
    r = np.rint(np.ascontiguousarray(x, np.complex64).view(np.float32) * np.float32(scale))
    return ((r > 127) | (r < -128)).reshape(-1, 2)


def _freeze(parts):
    for p in parts:
        for x in p:
            x.setflags(write=False)
    return parts


# ---- saturation cases: (cuts, input [B, n], oracle output per call and stream, scale) --------------------------------------------------
MOD_SAT_CUTS = [67, 5, 40]
AMOD_SAT_CUTS = [324, 8, 100]
SILENT_SCALE = 1000.0     # USB at gain 1 peaks near 0.19: x 1000 is past 127 in the loud streams


@functools.lru_cache(maxsize=None)
def mod_saturation():
    """QPSK250K at 4 Msps, +25 kHz, bb_gain 4 (multiply_const_cc(4) is exact in f32: the oracle's gain-1 modulator output x 4 is the gain-4 one)"""
    data = S16._bytes(400, sum(MOD_SAT_CUTS))
    refs = [S16.back_end(orc.mod_qpsk(data[b]) * np.float32(4.0), 4000000, 25000.0) for b in range(B)]
    e = np.cumsum([0] + MOD_SAT_CUTS) * 128                       # 32 samples per byte at 1 Msps, x 4
    return data, _freeze([[x[e[i]:e[i + 1]] for x in refs] for i in range(3)])


@functools.lru_cache(maxsize=None)
def amod_saturation():
    """NBFM at 1 Msps with bb_gain 3: k_tx_interp_c as the analogue chain's terminal kernel"""
    audio = S16._audio(401, sum(AMOD_SAT_CUTS))
    refs = [orc.mod_nbfm(audio[b], filter_width=5000, bb_gain=3.0) for b in range(B)]
    e = np.cumsum([0] + AMOD_SAT_CUTS) * 125
    return audio, _freeze([[x[e[i]:e[i + 1]] for x in refs] for i in range(3)])


@functools.lru_cache(maxsize=None)
def silent_stream():
    """USB at 1 Msps under scale SILENT_SCALE with stream 1 silent: its samples are zero and it clips nowhere, beside two streams that clip"""
    audio = S16._audio(402, 2048)
    audio[1] = 0.0
    return audio, _freeze([[orc.mod_ssb(audio[b], sb=0) for b in range(B)]])[0]


def saturation_preconditions(refs, scale=127.0):
    """in every stream some components clip and some do not, some samples clip in both components, and both rails are reached"""
    flags = [clip_flags(x, scale) for x in refs]
    for b, f in enumerate(flags):
        assert f.any() and not f.all(), "stream %d: %d of %d components clip" % (b, f.sum(), f.size)
        assert f.all(axis=1).any(), "stream %d: no sample clips in both components" % b
    allv = np.concatenate([conv8(x, scale)[0].ravel() for x in refs])
    assert (allv == 127).any() and (allv == -128).any()
    assert len({int(f.sum()) for f in flags}) >= 2, "the streams' counts must differ"


def silent_preconditions(refs):
    counts = [conv8(x, SILENT_SCALE)[1] for x in refs]
    assert counts[1] == 0 and not refs[1].view(np.float32).any(), "stream 1 is silent"
    assert counts[0] > 0 and counts[2] > 0, counts
    assert conv8(refs[0], 127.0)[1] == 0, "only the scale makes it clip"


# the terminal kernels the three cases above do not reach, at bb_gain 4 (test_gpu_sc16_output._clip_case names the single-carrier store by its int16 launch)
OTHER_KERNELS = {"k_tx_interp_sym": "k_tx_interp_sym", "k_tx_interp": "k_tx_interp", "k_tx_rot": "k_tx_rot", "k_an_fir_ccc": "k_an_fir_ccc",
                 "k_pfb_synth": "k_pfb_synth", "k_ring_store_fmt": "k_ring_store_sc16"}


@functools.lru_cache(maxsize=None)
def clip_case(name):
    make, x, refs = S16._clip_case(OTHER_KERNELS[name])
    return make, x, _freeze([refs])[0]


def clip_case_preconditions(refs):
    for b, x in enumerate(refs):
        f = clip_flags(x)
        assert f.any() and not f.all(), "stream %d: %d of %d components clip" % (b, f.sum(), f.size)
    assert refs[0].size % 256, "the last workgroup must be ragged"


# ---- loopback in the format: TX sc8 at 8 Msps (GMSK-10k) -> the same int8 samples into the receiver at 8 Msps ---------------------------
LOOP_RATE, LOOP_OFFSET, LOOP_FRAMES = 8000000, 25000.0, 2
LOOP_SYNC, LOOP_PAYLOAD_BITS = sig.MODES["gmsk10k"][2], 8 * sig.MODES["gmsk10k"][3]


@functools.lru_cache(maxsize=None)
def loopback():
    """(bytes [B, n], payloads per stream, the transmitter's int8 samples per stream [count, 2], the receiver oracle's ports per stream for the floats
    (float)v / 128).  Every stream carries frames of its own; a tail of idle bytes flushes the filters and the Viterbi decoders."""
    rng = np.random.default_rng(88)
    rows, payloads = [], []
    for _ in range(B):
        d, p = sig.frames("gmsk10k", LOOP_FRAMES, rng)
        rows.append(np.concatenate([d, np.full(24, 0xAA, np.uint8)]))
        payloads.append(p)
    data = np.stack(rows)
    codes = [conv8(S16.back_end(orc.mod_gmsk(data[b], sps=10, filter_width=20000), LOOP_RATE, LOOP_OFFSET))[0] for b in range(B)]
    rx = [orc.demod_gmsk(orc.frontend((codes[b].astype(np.float32) * np.float32(1.0 / 128)).view(np.complex64).ravel(), LOOP_RATE, LOOP_OFFSET),
                         sps=1, filter_width=20000) for b in range(B)]
    data.setflags(write=False)
    for c in codes:
        c.setflags(write=False)
    return data, payloads, codes, rx


def recovered(bits_a, bits_b, payloads):
    """every sent payload comes out of one of the receiver's two bit ports"""
    found = sig.find_frames(bits_a, LOOP_SYNC, LOOP_PAYLOAD_BITS) + sig.find_frames(bits_b, LOOP_SYNC, LOOP_PAYLOAD_BITS)
    return all(p in found for p in payloads)
