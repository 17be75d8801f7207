"""Pins for the CPU oracle (oracle/liborc.so).  The reference ships no tests or vectors (SURVEY.md 4,
8c: "parity unpinned"), so the oracle is pinned by (i) the constants the reference's own call sites
imply (tap counts of Appendix B computed from the firdes formulas, FEC polynomials, LFSR, sync words),
(ii) upstream table rows quoted in SURVEY.md A.7/A.8 and (iii) mod -> channel -> demod loopback
known-answer tests through the reference's chain topologies."""
import math

import numpy as np
import pytest

import front_end_rates as fer
import orc
import sig

BH = orc.WIN_BH


# ---- (i) filter-design constants implied by the reference's firdes calls
@pytest.mark.parametrize("args,ntaps", [
    ((1, 1e6, 10e3, 10e3, BH), 419),        # gr_demod_2fsk.cpp:82-88 (sps 10)
    ((1, 1e6, 20e3, 20e3, BH), 209),        # gr_demod_2fsk.cpp (sps 5)
    ((2, 2e6, 40e3, 40e3, BH), 209),        # gr_demod_gmsk.cpp:80-83 (sps 1)
    ((1, 20e3, 2e3, 2e3, BH), 41),          # gr_demod_2fsk.cpp:91-92
    ((1, 20e3, 2e3, 2e3, orc.WIN_HAMMING), 25),   # gr_demod_2fsk.cpp:84-87
    ((1, 80e3, 20e3, 20e3, BH), 17),        # gr_demod_gmsk.cpp:84-85
    ((1, 80e3, 20e3, 20e3, orc.WIN_HAMMING), 9),  # gr_demod_gmsk.cpp:96-98
    ((1, 2e6, 480e3, 100e3, BH), 83),       # gr_demod_base.cpp:1333-1336 @2 Msps
    ((1, 10e6, 480e3, 100e3, BH), 419),
    ((1, 25e6, 480e3, 100e3, BH), 1045),
    ((1, 100e6, 480e3, 100e3, BH), 4181),
    ((1, 20e3, 3000, 1500, BH), 55),        # gr_demod_4fsk.cpp:108-109 (4FSK2KFM: fw 3000, tw fw/2)
    ((1, 500e3, 125e3, 62500, BH), 33),     # gr_demod_4fsk.cpp:108-109 (4FSK100K)
    ((1, 1e6, 250e3, 250e3, BH), 17),       # gr_demod_4fsk.cpp:100-101 (sps 2: 1:2 resampler)
    ((1.0, 20e3, 2000, 100, BH), 837),      # gr_demod_4fsk.cpp:103-105 _symbol_filter (non-FM branch)
    ((1, 240e3, 8000, 3500, BH), 287),      # gr_demod_mmdvm_multi.cpp:64-65 (legacy freq-xlating receiver)
    ((1, 24e3, 8000, 3500, BH), 29),        # gr_demod_mmdvm_multi.cpp:73-74
    ((4, 4e6, 480e3, 20e3, BH), 837),       # gr_mod_base.cpp:249-250 @4 Msps (209 per phase)
])
def test_low_pass_tap_counts(args, ntaps):
    t = orc.low_pass(*args)
    assert t.size == ntaps
    assert np.allclose(t, t[::-1], atol=0, rtol=0)            # linear phase
    assert abs(float(np.sum(t.astype(np.float64))) - args[0]) < 2e-6 * args[0]   # DC gain = gain


@pytest.mark.parametrize("args,ntaps", [
    ((1, 1e6, 250e3, 50e3, 60, BH), 55),       # gr_demod_qpsk.cpp:92-96
    ((1, 250e3, 5e3, 2e3, 60, BH), 341),       # gr_demod_mmdvm_multi2.cpp:98
    ((1, 600e3, 5e3, 2e3, 60, BH), 819),       # gr_demod_mmdvm_multi2.cpp:60-61
    ((1, 24e3, 5e3, 2e3, 60, BH), 33),         # gr_demod_mmdvm_multi2.cpp:62-63
    ((3, 3e6, 5e3, 2e3, 60, BH), 4091),        # gr_demod_dmr.cpp:55-58
    ((12, 3e6, 5e3, 2e3, 60, BH), 4091),       # gr_demod_mmdvm.cpp:43-44 (12/125 resampler)
    ((25, 600e3, 5e3, 2e3, 60, BH), 819),      # gr_mod_mmdvm_multi2.cpp:50-51 (25/24 resampler)
    ((10, 250e3, 5e3, 2e3, 60, BH), 341),      # gr_mod_mmdvm_multi2.cpp:88-89 (synthesizer prototype)
    ((125, 3e6, 5e3, 2e3, 60, BH), 4091),      # gr_mod_mmdvm.cpp:43-44 (125/12 resampler)
    ((1, 1e6, 5e3, 1e3, 60, BH), 2727),        # gr_demod_qpsk.cpp:92-96 for QPSK2K (target 10 ksps)
    ((1, 1e6, 20e3, 4e3, 60, BH), 681),        # gr_demod_qpsk.cpp:92-96 for QPSK20K (target 40 ksps)
])
def test_low_pass_2_tap_counts(args, ntaps):
    # firdes::compute_ntaps_windes is fred harris' rule N = A*fs/(22*tw) made odd (the same rule as
    # compute_ntaps with A given explicitly); SURVEY.md A.1 quotes Kaiser's optfir estimate instead,
    # which is not what firdes::low_pass_2 calls -- see DESIGN.md "Oracle deviations from SURVEY.md".
    assert orc.low_pass_2(*args).size == ntaps


def test_complex_band_pass_is_shifted_low_pass():
    up = orc.complex_band_pass(1, 20e3, -2e3, 0, 2e3, BH)   # gr_demod_2fsk.cpp:94-95
    lo = orc.complex_band_pass(1, 20e3, 0, 2e3, 2e3, BH)
    assert up.size == lo.size == 41
    assert np.allclose(up, np.conj(lo), atol=1e-7)
    # pass band centre: -1 kHz for "upper", +1 kHz for "lower" (SURVEY.md 7.3-9 polarity quirk)
    n = np.arange(41)
    assert abs(np.sum(up * np.exp(2j * np.pi * 1e3 * n / 20e3))) > 0.9
    assert abs(np.sum(up * np.exp(-2j * np.pi * 1e3 * n / 20e3))) < 0.3


def test_rrc_and_gaussian_normalisation():
    r = orc.root_raised_cosine(1, 24000, 4800, 0.2, 125)
    assert r.size == 125 and abs(r.sum() - 1) < 1e-5 and np.allclose(r, r[::-1], atol=1e-7)
    assert orc.root_raised_cosine(2, 2, 1, 0.35, 22).size == 23   # gr_demod_qpsk.cpp:100-103 (made odd)
    g = orc.gaussian(10, 10, 0.3, 40)
    assert abs(g.sum() - 10) < 1e-4
    assert orc.root_raised_cosine(1.5, 20000, 2000, 0.2, 251).size == 251    # gr_demod_4fsk.cpp:130-133
    assert orc.root_raised_cosine(10, 10, 1, 0.35, 150).size == 151          # gr_demod_bpsk.cpp:64-66 (made odd)
    assert orc.root_raised_cosine(500, 500, 1, 0.35, 5500).size == 5501      # gr_mod_bpsk.cpp:52-54
    assert orc.complex_band_pass(1, 20e3, -4000, -2000, 4000, BH).size == 21  # gr_demod_4fsk.cpp:112-113


# ---- (ii) upstream table rows
def test_mmse_table_rows():
    t = orc.table("mmse", 129 * 8).reshape(129, 8)
    row1 = [-1.54700e-04, 8.53777e-04, -2.76968e-03, 7.89295e-03, 9.98534e-01, -5.41054e-03, 1.24642e-03, -1.98993e-04]
    row64 = [-6.77751e-03, 3.94578e-02, -1.42658e-01, 6.09836e-01, 6.09836e-01, -1.42658e-01, 3.94578e-02, -6.77751e-03]
    assert np.allclose(t[1], row1, rtol=0, atol=6e-7)
    assert np.allclose(t[64], row64, rtol=0, atol=6e-7)
    e0 = np.zeros(8); e0[4] = 1
    e128 = np.zeros(8); e128[3] = 1
    assert np.array_equal(t[0], e0.astype(np.float32)) and np.array_equal(t[128], e128.astype(np.float32))
    # mirror symmetry of the design: row(128-k) is row k reversed
    assert np.allclose(t[128 - 5], t[5][::-1], atol=2e-6)


def test_atan_table_and_fast_atan2():
    t = orc.table("atan", 257)
    assert t[0] == 0 and t[256] == t[255] and abs(t[255] - math.pi / 4) < 1e-7
    assert np.allclose(t[:256], np.arctan(np.arange(256) / 255.0), atol=1e-7)
    rng = np.random.default_rng(1)
    for y, x in rng.standard_normal((200, 2)):
        assert abs(orc.lib.orc_fast_atan2f(y, x) - math.atan2(y, x)) < 2e-5
    assert orc.lib.orc_fast_atan2f(0.0, 0.0) == 0.0


def test_tanh_table():
    t = orc.table("tanh", 256)
    assert np.allclose(t, np.tanh((np.arange(256) - 128) / 64.0), atol=1e-6)


def test_deterministic_sincos_accuracy():
    for x in np.linspace(-7, 7, 401):
        s, c = orc.sincosf(float(x))
        assert abs(s - math.sin(x)) < 3e-7 and abs(c - math.cos(x)) < 3e-7
    for a in (0, 1 << 62, 1 << 63, 3 << 62, 12345678901234567):
        s, c = orc.sincos_turn(a)
        th = 2 * math.pi * a / 2.0 ** 64
        assert abs(s - math.sin(th)) < 3e-7 and abs(c - math.cos(th)) < 3e-7


# ---- FEC / LFSR constants of the reference call sites (gr_demod_2fsk.cpp:78-80,120-127)
def test_cc_encoder_polys_109_79():
    # impulse response of the K=7 r=1/2 encoder gives the generator polynomials (MSB = newest bit)
    imp = np.zeros(7, np.uint8); imp[0] = 1
    out = orc.cc_encode_k7(imp).reshape(-1, 2)
    g0 = int("".join(str(b) for b in out[:, 0]), 2)
    g1 = int("".join(str(b) for b in out[:, 1]), 2)
    assert {g0, g1} == {109, 79} or {int(bin(g0)[2:].zfill(7)[::-1], 2), int(bin(g1)[2:].zfill(7)[::-1], 2)} == {109, 79}


def test_viterbi_roundtrip_and_error_correction():
    rng = np.random.default_rng(4)
    bits = rng.integers(0, 2, 80 * 12, dtype=np.uint8)
    coded = orc.cc_encode_k7(bits)
    soft = np.where(coded > 0, 255, 0).astype(np.uint8)
    dec = orc.cc_decode_k7(soft)
    assert dec.size == 80 * 11            # last block waits for its 12-symbol look-ahead (A.9)
    assert np.array_equal(dec, bits[:dec.size])
    noisy = soft.copy()
    for k in range(10, noisy.size - 40, 37):   # isolated hard errors are corrected
        noisy[k] = 255 - noisy[k]
    assert np.array_equal(orc.cc_decode_k7(noisy), bits[:dec.size])
    # soft values: weak symbols around 128 still decode
    weak = np.where(coded > 0, 150, 106).astype(np.uint8)
    assert np.array_equal(orc.cc_decode_k7(weak), bits[:dec.size])


def test_code_is_inversion_transparent_with_descrambler():
    # odd-weight polys + even-term descrambler => a global inversion cancels
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 80 * 6, dtype=np.uint8)
    scr = orc.scramble(bits)
    coded = orc.cc_encode_k7(scr)
    a = orc.descramble(orc.cc_decode_k7(np.where(coded > 0, 255, 0).astype(np.uint8)))
    b = orc.descramble(orc.cc_decode_k7(np.where(coded > 0, 0, 255).astype(np.uint8)))
    n = a.size
    # scrambler_bb emits sr&1, i.e. its input delayed by len+1 = 8 bits (lfsr.h next_bit_scramble)
    assert np.array_equal(a[16:], bits[8:n - 8])
    assert np.array_equal(b[24:], bits[16:n - 8])


def test_scrambler_descrambler_self_synchronising():
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 2, 500, dtype=np.uint8)
    s = orc.scramble(bits)
    assert not np.array_equal(s, bits)
    d = orc.descramble(s)
    assert np.array_equal(d[8:], bits[:-8])      # additive scrambler output lags its input by 8 bits
    d2 = orc.descramble(s[100:])                 # joins mid-stream: resynchronises after 8 bits
    assert np.array_equal(d2[8:], bits[100:-8])


# ---- block semantics
def test_decimator_matches_definition_and_chain_split():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    h = orc.low_pass(1, 1e6, 10e3, 10e3, BH)
    y = orc.decim_fir_ccf(x, h, 50)
    full = np.convolve(x.astype(np.complex128), h.astype(np.float64))[: x.size]
    want = full[::50]
    assert y.size == want.size == 100
    assert np.max(np.abs(y - want)) < 2e-6 * np.max(np.abs(want))


def _definition_error(y, x, h, decim):
    full = np.convolve(x.astype(np.complex128), h.astype(np.float64))[: x.size]
    want = full[::decim]
    assert y.size == want.size
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    return np.max(np.abs(y - want)) / rms


@pytest.mark.parametrize("fs,decim", [(25000000, 25), (50000000, 50), (100000000, 100)])
def test_m16_contract_matches_float64_definition(fs, decim):
    """The MFMA summation order (four fmaf chains per output over zero-padded quarters) stays inside the 1e-5 of RMS the
    north star allows against the float64 definition of the decimating FIR, for the three front-end geometries."""
    rng = np.random.default_rng(70 + decim)
    h = orc.low_pass(1, fs, 480e3, 100e3, BH)
    x = (rng.standard_normal(40 * decim + h.size) + 1j * rng.standard_normal(40 * decim + h.size)).astype(np.complex64)
    assert orc.lib.orc_decim_uses_m16(h.size, decim)
    assert _definition_error(orc.decim_fir_ccf_m16(x, h, decim), x, h, decim) < 1e-5


@pytest.mark.parametrize("decim,nt_scale", [(50, 1.0), (33, 1.0), (52, 0.9)])
def test_pm_contract_matches_float64_definition(decim, nt_scale):
    """Phase-major order of k_decim_pm (per block one fmaf chain over the D phases = the f32 matrix pipe's k order, then the J block
    terms in the lane-row order of the matrix result) against the float64 definition; also the rule that selects it."""
    rng = np.random.default_rng(90 + decim)
    h = orc.low_pass(1, 1e6, 10e3 / nt_scale, 10e3 / nt_scale, BH)
    x = (rng.standard_normal(60 * decim + h.size) + 1j * rng.standard_normal(60 * decim + h.size)).astype(np.complex64)
    assert orc.lib.orc_decim_uses_pm(h.size, decim) and not orc.lib.orc_decim_uses_pl(h.size, decim)
    y = orc.decim_fir_ccf_pm(x, h, decim)
    assert _definition_error(y, x, h, decim) < 1e-5
    assert np.array_equal(orc.decim_auto(x, h, decim).view(np.float32), y.view(np.float32))


def test_pl_contract_two_samples_per_lane_matches_float64_definition():
    """A 96:1 front end (4 013 taps at 96 Msps): 48 lane slots of two neighbouring samples each (k_decim_plx<2, 1, 42>; 100:1 itself
    moved to the phase-major matrix kernel in round 3)."""
    rng = np.random.default_rng(191)
    h = orc.low_pass(1, 96e6, 480e3, 100e3, BH)
    x = (rng.standard_normal(40 * 96 + h.size) + 1j * rng.standard_normal(40 * 96 + h.size)).astype(np.complex64)
    assert orc.lib.orc_decim_uses_pl(h.size, 96) and not orc.lib.orc_decim_uses_pm(h.size, 96) and (h.size + 95) // 96 == 42
    y = orc.decim_fir_ccf_pl(x, h, 96)
    assert _definition_error(y, x, h, 96) < 1e-5
    assert np.array_equal(orc.decim_auto(x, h, 96).view(np.float32), y.view(np.float32))


@pytest.mark.parametrize("fs,decim", [(10e6, 10), (20e6, 20), (25e6, 25), (50e6, 50), (100e6, 100)])
def test_pm_contract_three_lag_tiles_matches_float64_definition(fs, decim):
    """The device-rate front ends (41.8 D taps = 42 block lags = three tiles of the matrix result, delay line over the groups)."""
    rng = np.random.default_rng(300 + decim)
    h = orc.low_pass(1, fs, 480e3, 100e3, BH)
    x = (rng.standard_normal(70 * decim + h.size) + 1j * rng.standard_normal(70 * decim + h.size)).astype(np.complex64)
    assert orc.lib.orc_decim_uses_pm(h.size, decim) and (h.size + decim - 1) // decim == 42
    y = orc.decim_fir_ccf_pm(x, h, decim)
    assert _definition_error(y, x, h, decim) < 1e-5
    assert np.array_equal(orc.decim_auto(x, h, decim).view(np.float32), y.view(np.float32))
    # absolute grouping: a stream that starts 16 blocks later gives the same bits once the window is inside
    y2 = orc.decim_fir_ccf_pm(x[16 * decim:], h, decim)
    k = 43
    assert np.array_equal(y[16 + k:].view(np.float32), y2[k:].view(np.float32))


def test_rules_leave_the_other_front_ends_on_m16():
    for fs, d in ((8e6, 8), (16e6, 16), (32e6, 32), (40e6, 40), (64e6, 64)):
        nt = orc.low_pass(1, fs, 480e3, 100e3, BH).size
        assert not orc.lib.orc_decim_uses_pl(nt, d) and not orc.lib.orc_decim_uses_pm(nt, d) and orc.lib.orc_decim_uses_m16(nt, d)


def _front_end_contract(D):
    """the oracle's rules in orc_decim_auto's order, as the kernel name of front_end_rates"""
    nt = orc.frontend_taps(D * 1000000).size
    u = orc.lib
    return fer.PM if u.orc_decim_uses_pm(nt, D) else fer.PL if u.orc_decim_uses_pl(nt, D) else fer.M16 if u.orc_decim_uses_m16(nt, D) else fer.GENERIC


def test_front_end_partition_is_pinned_for_every_accepted_rate():
    """Which contract defines which device rate, 2 .. 183 Msps, against the table written out in front_end_rates.py (docs/KERNELS.md 17):
    a change of a selection rule shows here before the GPU test's kernel-name check does.  Also what the table's comments claim: 42 taps
    per phase for every D, the pm kernel's slab counts, and the generic tile's LDS bound that ends the range at 183."""
    wrong = [(D, _front_end_contract(D), fer.front_end_class(D)) for D in range(fer.FIRST_D, fer.LAST_D + 1)
             if _front_end_contract(D) != fer.front_end_class(D)]
    assert not wrong, wrong
    for D in range(fer.FIRST_D, fer.LAST_D + 1):
        h = orc.frontend_taps(D * 1000000)
        assert np.array_equal(h, orc.low_pass(1, D * 1e6, 480e3, 100e3, BH))
        assert (h.size + D - 1) // D == 42, (D, h.size)
        if fer.front_end_class(D) == fer.PM:
            assert (D + 3) // 4 in fer.PM_NS
    assert sorted({(D + 3) // 4 for D in range(fer.FIRST_D, fer.LAST_D + 1) if fer.front_end_class(D) == fer.PM}) == list(fer.PM_NS)
    assert fer.generic_lds_bytes(fer.LAST_D) <= 160 * 1024 < fer.generic_lds_bytes(fer.LAST_D + 1)
    assert _front_end_contract(fer.LAST_D + 1) == fer.GENERIC and _front_end_contract(200) == fer.GENERIC   # no other kernel takes what the generic one refuses


def test_every_front_end_rate_matches_float64_definition():
    """orc_decim_auto with the front-end filter of every D = 2 .. 183 (whatever contract the rules pick for it) against the float64
    definition of the decimating FIR: 1e-5 of the output RMS, the project's bound for a summation order.  40 D + ntaps noise samples,
    one fixed seed per D.  And auto IS the contract the partition names, bit for bit."""
    by_class = {fer.GENERIC: orc.decim_fir_ccf, fer.M16: orc.decim_fir_ccf_m16, fer.PM: orc.decim_fir_ccf_pm, fer.PL: orc.decim_fir_ccf_pl}
    worst, over, other = (0.0, 0), [], []
    for D in range(fer.FIRST_D, fer.LAST_D + 1):
        rng = np.random.default_rng(5000 + D)
        h = orc.frontend_taps(D * 1000000)
        n = 40 * D + h.size
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        y = orc.decim_auto(x, h, D)
        e = _definition_error(y, x, h, D)
        worst = max(worst, (e, D))
        if not e < 1e-5:
            over.append((D, e))
        if not np.array_equal(y.view(np.uint32), by_class[fer.front_end_class(D)](x, h, D).view(np.uint32)):
            other.append(D)
    print("worst definition error %.3g of RMS at D = %d" % worst)
    assert not over, over
    assert not other, other


def test_cpu_baseline_simd_decimator_matches_definition():
    """The AVX2 dot-product decimator the bench times as CPU baseline (not a checker) computes the same filter."""
    rng = np.random.default_rng(17)
    for decim, h in ((50, orc.low_pass(1, 1e6, 10e3, 10e3, BH)), (25, orc.low_pass(1, 25e6, 480e3, 100e3, BH))):
        x = (rng.standard_normal(30 * decim + 2 * h.size) + 1j * rng.standard_normal(30 * decim + 2 * h.size)).astype(np.complex64)
        assert _definition_error(orc.decim_fir_ccf_simd(x, h, decim), x, h, decim) < 1e-5


def test_pm_contract_depends_on_the_absolute_output_index_only():
    """Output m only depends on the samples of its window and on m mod 16 (the absolute 16-block groups of the matrix result): a
    stream that starts whole groups later gives the same bits once the window is inside the stream -- the property chunked /
    segmented evaluation relies on (the engine indexes outputs absolutely).  A shift by a non-multiple of 16 blocks regroups the
    block terms: same value to rounding, different bits."""
    rng = np.random.default_rng(5)
    h = orc.low_pass(1, 1e6, 10e3, 10e3, BH)
    x = (rng.standard_normal(6000) + 1j * rng.standard_normal(6000)).astype(np.complex64)
    y = orc.decim_fir_ccf_pm(x, h, 50)
    y2 = orc.decim_fir_ccf_pm(x[800:], h, 50)
    k = (h.size + 49) // 50 + 1
    assert np.array_equal(y[16 + k:].view(np.float32), y2[k:].view(np.float32))
    y3 = orc.decim_fir_ccf_pm(x[500:], h, 50)
    assert np.max(np.abs(y[10 + k:] - y3[k:])) < 1e-6 * np.max(np.abs(y))


def test_pl_contract_is_position_independent():
    """(two-samples-per-lane geometry, the 100:1 front end) Output m only depends on the samples of its window."""
    rng = np.random.default_rng(5)
    h = orc.low_pass(1, 96e6, 480e3, 100e3, BH)
    x = (rng.standard_normal(12000) + 1j * rng.standard_normal(12000)).astype(np.complex64)
    y = orc.decim_fir_ccf_pl(x, h, 96)
    y2 = orc.decim_fir_ccf_pl(x[960:], h, 96)
    k = (h.size + 95) // 96 + 1
    assert np.array_equal(y[10 + k:].view(np.float32), y2[k:].view(np.float32))


def test_rational_resampler_matches_zero_stuffing_definition():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(3000) + 1j * rng.standard_normal(3000)).astype(np.complex64)
    h = orc.low_pass(2, 2e6, 40e3, 40e3, BH)
    y = orc.resamp_ccf(x, h, 2, 25)
    up = np.zeros(2 * x.size, np.complex128); up[::2] = x
    full = np.convolve(up, h.astype(np.float64))[: up.size]
    want = full[::25]
    assert y.size == want.size
    assert np.max(np.abs(y - want)) < 2e-6 * np.max(np.abs(want))


def test_rotator_is_exact_nco():
    x = np.ones(4096, np.complex64)
    inc = orc.phase_inc_to_turn(2 * math.pi * -25000.0 / 4e6)
    y = orc.rotator(x, inc)
    n = np.arange(x.size)
    assert np.max(np.abs(y - np.exp(-2j * np.pi * 25000.0 * n / 4e6))) < 5e-7
    assert np.max(np.abs(np.abs(y) - 1)) < 3e-7     # no amplitude drift (VOLK renormalises every 512)


# ---- (iii) loopback KATs through the reference's chain topologies
def _frames_ok(mode, bits, payloads):
    sync, nbits = {"gmsk10k": (bytes([0xED, 0x89]), 384), "qpsk250k": (bytes([0xDE, 0x98, 0xAA]), 1516 * 8)}.get(
        mode, (bytes([0xB5]), 32))
    fr = sig.find_frames(bits, sync, nbits)
    if mode == "gmsk10k":
        return sum((bytes([0xAA]) + p) in fr for p in payloads)
    return sum(p in fr for p in payloads)


@pytest.mark.parametrize("mode,rate", [("2fsk1k", 1000000), ("2fsk1kfm", 1000000), ("gmsk1k", 1000000),
                                       ("gmsk10k", 1000000), ("gmsk10k", 4000000), ("qpsk250k", 1000000)])
def test_loopback_recovers_every_frame(mode, rate):
    y, payloads = sig.make_stream(mode, nframes=3, device_rate=rate, rx_offset_hz=25000.0, seed=5)
    fe = orc.frontend(y, rate, 25000.0 if rate >= 2000000 else 0.0)
    if mode.startswith("2fsk"):
        r = orc.demod_2fsk(fe, sps=10, filter_width=2500 if mode.endswith("fm") else 2000, fm=mode.endswith("fm"))
    elif mode == "gmsk10k":
        r = orc.demod_gmsk(fe, sps=1, filter_width=20000)
    elif mode == "gmsk1k":
        r = orc.demod_gmsk(fe, sps=10, filter_width=2000)
    else:
        r = orc.demod_qpsk(fe)
    got = max(_frames_ok(mode, r[k], payloads) for k in ("bits_a", "bits_b") if r[k].size)
    assert got == len(payloads)
    # port geometry of the hier blocks (gr_demod_2fsk.cpp:19-37): rates 20k/2k/1k etc.
    assert r["filtered"].size > 0 and r["constellation"].size > 0
    if mode != "qpsk250k":
        assert abs(r["bits_a"].size - r["bits_b"].size) <= 80


def test_two_branch_alignment_exactly_one_branch_locks():
    """gr_demod_2fsk.cpp:158-164: the second decoder sees the soft stream delayed by one symbol; only
    one of the two alignments is the true pairing of coded bits."""
    y, payloads = sig.make_stream("gmsk10k", nframes=3, seed=9)
    r = orc.demod_gmsk(y, sps=1, filter_width=20000)
    ok = [_frames_ok("gmsk10k", r[k], payloads) for k in ("bits_a", "bits_b")]
    assert sorted(ok) == [0, 3]


# ---- multi-carrier MMDVM RX (gr_demod_mmdvm_multi2.cpp:98): channel orientation and FM scaling
@pytest.mark.parametrize("M", [10, 64])
def test_pfb_channelizer_single_tone_lands_in_its_channel(M):
    """A.13: channel c is centred at +c*fs/M (c > M/2: negative offsets), consistent with the reference's port map
    {0,1,2,3,9,8,7} = {0,+25,+50,+75,-25,-50,-75 kHz} (docs/README_MMDVM_operation.md:136-157)."""
    fs = 25000.0 * M
    taps = orc.chan_proto_taps(M)
    assert taps.size == {10: 341, 64: 2181}[M]
    t = np.arange(M * 3000)
    for c in (0, 1, 3, M - 1, M // 2 + 1):
        f = c * 25000.0 if c <= M // 2 else (c - M) * 25000.0
        x = np.exp(2j * np.pi * (f + 300.0) * t / fs).astype(np.complex64)
        p = np.mean(np.abs(orc.pfb_channelizer(x, taps, M)[:, 200:]) ** 2, axis=1)
        assert int(np.argmax(p)) == c and abs(p[c] - 1.0) < 1e-3 and np.sort(p)[-2] < 1e-9


def test_mmdvm_chain_fm_deviation_scaling():
    """quadrature_demod gain 24000/(2 pi 12500) and float_to_short(32767): a +-2 kHz deviation reads +-5242 counts"""
    M, fs = 10, 250000.0
    t = np.arange(M * 30000)
    dev, fm = 2000.0, 400.0
    ph = 2 * np.pi * (2 * 25000.0) * t / fs + (dev / fm) * np.sin(2 * np.pi * fm * t / fs)
    o = orc.demod_mmdvm_multi((0.5 * np.exp(1j * ph)).astype(np.complex64), M)
    assert o.shape == (10, 28800)
    peak = np.abs(o[2, 2000:].astype(np.int32)).max()
    assert abs(peak - 32767 * dev / 12500.0) < 40
    assert np.abs(o[5, 2000:].astype(np.int32)).max() > 20000   # an empty channel is discriminator noise, full scale


def test_dmr_4fsk_oracle_recovers_dibits():
    """gr_demod_dmr chain (3/125 resampler, discriminator, RRC, M&M symbol sync on the 4-level constellation, phase
    modulator + slicer + map{3,1,2,0}) returns the transmitted dibits of a DMR-shaped 4FSK burst."""
    x, dib = sig.make_4fsk(nsym=500, seed=7)
    r = orc.demod_dmr(x)
    assert r["filtered"].size == orc.lib.orc_decim_count(x.size, 3, 125)
    got = r["bits_a"].reshape(-1, 2)
    got = got[:, 0] * 2 + got[:, 1]
    assert max(np.mean(got[k:k + 400] == dib[:400]) for k in range(40)) == 1.0
    assert np.allclose(np.abs(r["constellation"][50:]), 1.0, atol=1e-6)


# ---- native 4FSK (FM variants) and BPSK chains (gr_demod_4fsk.cpp, gr_demod_bpsk.cpp): the oracle's modulator through a
# seeded channel into the oracle's demodulator returns the frames
NEW_MODES = {
    "4fsk2k": (bytes([0xED, 0x89, 0xAA]), 56, lambda fe: orc.demod_4fsk(fe, sps=5, filter_width=4000, fm=False)),
    "4fsk2kfm": (bytes([0xED, 0x89, 0xAA]), 56, lambda fe: orc.demod_4fsk(fe, sps=5, filter_width=3000, fm=True)),
    "4fsk1kfm": (bytes([0xB5]), 32, lambda fe: orc.demod_4fsk(fe, sps=10, filter_width=2000, fm=True)),
    "4fsk10kfm": (bytes([0xED, 0x89, 0xAA]), 47 * 8, lambda fe: orc.demod_4fsk(fe, sps=1, filter_width=20000, fm=True)),
    "4fsk100k": (bytes([0xDE, 0x98, 0xAA]), 1516 * 8, lambda fe: orc.demod_4fsk(fe, sps=2, filter_width=125000, fm=True)),
    "bpsk1k": (bytes([0xB5]), 32, lambda fe: orc.demod_bpsk(fe, sps=10)),
    "bpsk2k": (bytes([0xED, 0x89, 0xAA]), 56, lambda fe: orc.demod_bpsk(fe, sps=5)),
}


@pytest.mark.parametrize("mode", sorted(NEW_MODES))
def test_loopback_4fsk_bpsk(mode):
    sync, nbits, dem = NEW_MODES[mode]
    nframes = 6 if mode.startswith("bpsk") else 3
    y, payloads = sig.make_stream(mode, nframes=nframes, device_rate=1000000, seed=6)
    y = np.concatenate([y, np.zeros(30000, np.complex64)])   # flush the filters and the 80-bit Viterbi frames
    r = dem(orc.frontend(y, 1000000, 0.0))
    got = 0
    for k in ("bits_a", "bits_b"):
        if r[k].size:
            fr = sig.find_frames(r[k], sync, nbits)
            got = max(got, sum(p in fr for p in payloads))
            if mode.startswith("bpsk"):   # BPSK has a 180 degree ambiguity; the convolutional code + descrambler are inversion transparent
                fr = sig.find_frames(1 - r[k], sync, nbits)
                got = max(got, sum(p in fr for p in payloads))
    # BPSK: agc2 (rate 0.1), FLL and Costas acquire during the first frame after the 8-byte preamble
    assert got >= len(payloads) - (1 if mode.startswith("bpsk") else 0), (mode, got)
    assert r["filtered"].size > 0 and r["constellation"].size > 0


MODES_40K_10KFM = {
    # mode: (oracle receiver, frames that may be lost)
    "2fsk2k": (lambda fe: orc.demod_2fsk(fe, sps=5, filter_width=4000, fm=False), 0),
    "gmsk2k": (lambda fe: orc.demod_gmsk(fe, sps=5, filter_width=4000), 0),
    # the FM variants: the 351- / 501-tap RRC and the loops are still settling behind the 8-byte preamble, the first frame is lost
    "2fsk2kfm": (lambda fe: orc.demod_2fsk(fe, sps=5, filter_width=4000, fm=True), 1),
    "2fsk10kfm": (lambda fe: orc.demod_2fsk(fe, sps=1, filter_width=25000, fm=True), 1),
}


@pytest.mark.parametrize("impair", [None, sig.SPEC], ids=["default", "survey8d"])
@pytest.mark.parametrize("seed,nframes", [(3, 3), (5, 5), (104, 3)])
@pytest.mark.parametrize("mode", sorted(MODES_40K_10KFM))
def test_loopback_2fsk_gmsk_40k_and_10kfm(mode, seed, nframes, impair):
    """The stimulus of the 40 ksps 2FSK / GMSK receivers and of 2FSK-10k FM (sig.MODES) is one the oracle alone decodes, in the default channel and
    in SURVEY 8(d)'s: what makes the device loopback of tests/test_gpu_parity.py::test_loopback_frames_recovered_40k_and_10kfm a statement"""
    dem, may_lose = MODES_40K_10KFM[mode]
    y, payloads = sig.make_stream(mode, nframes, device_rate=1000000, rx_offset_hz=0.0, seed=seed, impair=impair)
    r = dem(orc.frontend(y, 1000000, 0.0))
    nbits = (sig.MODES[mode][3] + 1) * 8
    got = max(sum((b"\xAA" + p) in sig.find_frames(r[k], b"\xED\x89", nbits) for p in payloads) for k in ("bits_a", "bits_b"))
    assert got >= nframes - may_lose, (mode, seed, got)
    assert r["filtered"].size > 0 and r["constellation"].size > 0


def test_4level_slicer_follows_constellation_rect_sectors():
    """symbol_sync_ff on a constant input: the decision is the sector (int)(x + 2) clamped to [0, 3], so exact zeros
    (the start-up transient) slice to +0.5, not -0.5"""
    import ctypes as C
    x = np.zeros(64, np.float32)
    out = np.zeros(64, np.float32)
    n = orc.lib.orc_symbol_sync_ff(x.ctypes.data_as(C.c_void_p), x.size, 1, 5.0, 0.0314, 1.0, 0.2869, 0.05, 2,
                                   out.ctypes.data_as(C.c_void_p))
    assert n > 5 and np.all(out[:n] == 0.0)


def test_rssi_tag_block_levels():
    """rssi_tag_block.cpp:43-68: one tag per 300 samples, 10 log10(sqrt(mean |x|^4)) = 20 log10(amplitude) for a constant envelope"""
    x = (0.1 * np.exp(2j * np.pi * 0.01 * np.arange(1000))).astype(np.complex64)
    db = orc.rssi_tag(x, cal=3.0)
    assert db.size == 3
    assert np.allclose(db, 20 * np.log10(0.1) + 3.0, atol=1e-3)


def test_mmdvm_single_carrier_chain():
    """gr_demod_mmdvm: 250 ksps -> 24 ksps, FM discriminator scaled so that +-10 kHz gives +-full scale / (2 pi) * 2 pi..."""
    fs, dev = 250000, 2500.0
    n = np.arange(fs // 2)
    x = (0.2 * np.exp(2j * np.pi * dev * n / fs)).astype(np.complex64)
    out, rssi = orc.demod_mmdvm(x)
    assert abs(out.size - n.size * 12 // 125) <= 1
    # quadrature_demod gain 24000 / (2 pi 10000): a constant +2.5 kHz offset reads 0.25 -> 0.25 * 32767
    assert abs(np.median(out[2000:]) - 0.25 * 32767) < 40
    assert rssi.size == out.size // 300 and np.allclose(rssi[5:], 20 * np.log10(0.2), atol=0.05)


def test_deframer_oracle_frames_and_state_carry():
    """gr_deframer_bb: sync bits + bit_buf_len frame bits; split calls give the same output as one call"""
    rng = np.random.default_rng(3)
    payload = rng.integers(0, 2, 32, dtype=np.uint8)
    b5 = np.array([(0xB5 >> (7 - k)) & 1 for k in range(8)], np.uint8)
    bits = np.concatenate([np.zeros(11, np.uint8), b5, payload, np.zeros(9, np.uint8), b5, payload[::-1], np.zeros(5, np.uint8)])
    out = orc.deframer(2, bits)
    assert np.array_equal(out, np.concatenate([b5, payload, b5, payload[::-1]]))
    st = np.zeros(3, np.uint32)
    parts = [orc.deframer(2, bits[a:b], st) for a, b in ((0, 15), (15, 16), (16, 60), (60, bits.size))]
    assert np.array_equal(np.concatenate(parts), out)
    # 24-bit word on a type-1 deframer: 24 sync bits + 64 frame bits
    w = np.array([(0x4C8A2B >> (23 - k)) & 1 for k in range(24)], np.uint8)
    fr = rng.integers(0, 2, 64, dtype=np.uint8)
    out = orc.deframer(1, np.concatenate([np.ones(3, np.uint8), w, fr, np.ones(10, np.uint8)]))
    assert np.array_equal(out[:24], w) and np.array_equal(out[24:88], fr)


def test_channelizer_plus_4fsk_tail_recovers_dibits():
    """BASELINE config 4 on the oracle: a 4FSK carrier planted on channel 2 of a 10 x 25 kHz band comes back as its dibits"""
    M, n, fs = 10, 60000, 250000.0
    rng = np.random.default_rng(1)
    iq = (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x, d = sig.make_4fsk(nsym=int(n / fs * 4800) - 2, seed=5, amp=0.4, noise=0.0, fs=fs)
    m = min(n, x.size)
    iq[:m] += (x[:m] * np.exp(2j * np.pi * 2 * 25000 * np.arange(m) / fs)).astype(np.complex64)
    out, dib = orc.demod_mmdvm_multi_4fsk(iq, M)
    g = dib[2].reshape(-1, 2)
    g = g[:, 0] * 2 + g[:, 1]
    assert max(np.mean(g[k:k + 800] == d[:800]) for k in range(60)) > 0.99


def test_legacy_freq_xlating_bank_channel_map():
    """gr_demod_mmdvm_multi.cpp:89-95: channel i listens at ct * separation, ct = i (i <= 3) or 3 - i; +2.5 kHz reads 0.2 full scale"""
    fs, n = 240000.0, 48000
    t = np.arange(n)
    for ch, ct in ((0, 0), (2, 2), (5, -2)):
        x = (0.3 * np.exp(2j * np.pi * (ct * 25000.0 + 2500.0) * t / fs)).astype(np.complex64)
        out, rssi = orc.demod_mmdvm_xlating(x, 7)
        assert abs(np.median(out[ch, 500:]) - 0.2 * 32767) < 30
        assert abs(rssi[ch][1] - 20 * np.log10(0.3)) < 0.1


def test_modem_sync_oracle_frames_by_class():
    """gr_modem::synchronize: 1k modes find 0xB5 + 4 bytes; 10k modes 0xED89 + (reserved + 47) bytes; QPSK-250k 0xDE98AA + 1516"""
    rng = np.random.default_rng(2)
    for mode, modem, ft, off in (("2fsk1k", 18, 0xB5, 0), ("gmsk10k", 22, 0xED89, 1), ("qpsk250k", 26, 0xDE98AA, 0)):
        data, payloads = sig.frames(mode, 3, rng)
        bits = np.unpackbits(data)
        ms = orc.ModemSync(modem)
        fr = ms.feed(bits[:777]) + ms.feed(bits[777:])
        assert [f for f, _ in fr] == [ft] * 3 and [p[off:] for _, p in fr] == payloads


def test_modem_sync_oracle_m17_words():
    """gr_modem::findSync for ModemTypeM17 (gr_modem.cpp:1187-1210, frame geometry :309-313): LSF 0x55F7 and stream 0xFF5D as 16-bit
    words, EOT 0x555D555D only as the full 32-bit word; every frame is 46 bytes, nothing is adjusted per frame type."""
    rng = np.random.default_rng(40)
    parts, want = [], []
    for word, nb in ((0x55F7, 16), (0xFF5D, 16), (0x555D555D, 32), (0xFF5D, 16)):
        payload = rng.integers(0, 256, 46, dtype=np.uint8)
        parts += [np.zeros(9, np.uint8), np.array([(word >> (nb - 1 - k)) & 1 for k in range(nb)], np.uint8), np.unpackbits(payload)]
        want.append((word, bytes(payload)))
    bits = np.concatenate(parts + [np.zeros(5, np.uint8)])
    ms = orc.ModemSync(40)
    fr = ms.feed(bits[:500]) + ms.feed(bits[500:])
    assert fr == want


def test_mmdvm_tx_synthesizer_loops_back_through_the_channelizer():
    """gr_mod_mmdvm_multi2 restatement -> gr_demod_mmdvm_multi2 restatement: channel c's tone returns on port {0,1,2,3,9,8,7}[c]"""
    N, n = 7, 24000
    t = np.arange(n)
    x = np.stack([(8000 * np.sin(2 * np.pi * (300 + 100 * c) * t / 24000)).astype(np.int16) for c in range(N)])
    y = orc.mod_mmdvm_multi(x)
    assert y.size == 250000 and 0.2 < np.sqrt(np.mean(np.abs(y) ** 2)) < 0.4
    out = orc.demod_mmdvm_multi(y, 10)
    for c in (0, 3, 4, 6):
        p = c if c <= 3 else 10 - (c - 3)
        r = out[p, 3000:3000 + 16384].astype(np.float64)
        f = np.abs(np.fft.rfft(r * np.hanning(r.size)))
        assert abs(np.argmax(f) * 24000 / r.size - (300 + 100 * c)) < 3.0
        assert 0.8 * 8000 < np.percentile(np.abs(r), 99) < 1.1 * 8000


def test_clock_recovery_mm_locks_to_symbol_rate():
    """clock_recovery_mm_cc(omega 10, 2.5e-5, 0.5, 0.05, 0.001) on a 10 samples/symbol BPSK waveform: one output per symbol,
    omega stays inside +-0.1 %, outputs sit on the +-1 decision points"""
    import ctypes as C
    rng = np.random.default_rng(4)
    sym = rng.integers(0, 2, 600) * 2.0 - 1.0
    h = orc.root_raised_cosine(10, 10, 1, 0.35, 110)
    x = np.zeros(sym.size * 10)
    x[::10] = sym
    x = np.convolve(np.convolve(x, h), h / 10.0).astype(np.complex64)
    out = np.zeros(x.size // 9 + 16, np.complex64)
    n = orc.lib.orc_clock_recovery_mm_cc(x.ctypes.data_as(C.c_void_p), x.size, 10.0, 2.5e-5, 0.5, 0.05, 0.001, out.ctypes.data_as(C.c_void_p))
    assert abs(n - x.size / 10) <= 2
    tail = out[100:n - 30].real
    assert np.median(np.abs(np.abs(tail) - 1.0)) < 0.05 and abs(np.abs(tail).mean() - 1.0) < 0.05


def test_m17_chain_recovers_dibits():
    """gr_demod_m17 in the oracle: an M17-shaped 4FSK burst (RRC 0.5, +-2400 / +-800 Hz) comes back as its
    dibits once the clock loop has settled."""
    x, dib = sig.make_4fsk(nsym=500, seed=9, alpha=0.5, dev=2400.0)
    r = orc.demod_m17(x)
    got = r["bits_a"].reshape(-1, 2)
    got = got[:, 0] * 2 + got[:, 1]
    assert max(np.mean(got[k + 60:k + 420] == dib[60:420]) for k in range(60)) == 1.0
    assert abs(r["filtered"].size - x.size * 3 / 125) <= 1 and r["constellation"].size * 2 == r["bits_a"].size


# ---- DSSS "BPSK 8" (gr_demod_dsss): definition checks of the restatement
def test_dsss_matched_filter_taps_are_the_reversed_barker_code_through_the_rrc():
    t = orc.dsss_taps(25)
    assert t.size == 13 * 25 + 11 * 25
    code = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1], np.float64)[::-1] * 2 - 1
    cs = np.zeros(13 * 25 + 2 * 275)
    cs[275:275 + 325] = np.repeat(code, 25)
    rrc = orc.root_raised_cosine(1, 25, 1.0, 0.35, 275).astype(np.float64)
    want = np.convolve(cs, rrc)[rrc.size - 1:rrc.size - 1 + 600]
    assert np.max(np.abs(t - want)) < 1e-5


def test_dsss_decoder_picks_the_correlation_peak_of_each_code_period():
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 2, 40)
    code = np.array([1, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1])
    chips = np.concatenate([code if b == 0 else 1 - code for b in bits]) * 2.0 - 1
    up = np.zeros(chips.size * 25)
    up[::25] = chips
    x = np.convolve(up, orc.root_raised_cosine(25, 25, 1, 0.35, 275).astype(np.float64))[:up.size]
    y = orc.dsss_decoder((x * np.exp(0.7j)).astype(np.complex64))
    assert y.size >= 38
    d = np.real(y * np.exp(-0.7j))
    # one output per code period, sign = the spread bit (bit 0 -> code -> positive correlation); the block's latency is two periods
    got = (d[3:39] < 0).astype(int)
    assert any(np.array_equal(got[:30], bits[k:k + 30]) for k in range(6)), (got, bits)
    assert np.all(np.abs(d[3:39]) > 0.5 * np.abs(d[3:39]).max())


def test_dsss_chain_recovers_the_information_bits():
    bits = np.random.default_rng(3).integers(0, 2, 120, dtype=np.uint8)
    r = orc.demod_dsss(sig.make_dsss(bits))
    want = "".join(map(str, bits[:60]))
    assert any(want in "".join(map(str, r[p])) for p in ("bits_a", "bits_b"))


# ---- analogue voice receivers (orc_analog.c): definition checks of the restated blocks
def test_pwr_squelch_gates_and_ramps():
    x = np.concatenate([np.ones(10), np.zeros(5000), np.ones(10)]).astype(np.complex64)
    y = orc.pwr_squelch_cc(x, db=-140.0, alpha=0.01, ramp=4, gate=True)
    # attack: the item that opens the gate leaves with envelope 0, then 0.5 - cos(pi k / 4) / 2
    assert np.allclose(y[:5].real, [0.0, 0.5 - np.cos(np.pi / 4) / 2, 0.5, 0.5 + np.cos(np.pi / 4) / 2, 1.0], atol=1e-7)
    # the single-pole power estimate (alpha 0.01) needs ln(p0 / 1e-14) / 0.01 items to fall below -140 dB; then 4 items of decay, then nothing
    p = 0.0
    for _ in range(10):
        p = 0.01 * 1.0 + 0.99 * p
    k = 0
    while p >= 1e-14:
        p *= 0.99
        k += 1
    # (the item that trips the threshold still leaves at full level, then ramp - 1 decaying items; the last one lands on envelope 0 = muted)
    assert y.size == 10 + (k - 1) + 4 + 10
    ungated = orc.pwr_squelch_cc(x, db=-140.0, alpha=0.01, ramp=4, gate=False)
    assert ungated.size == x.size


def test_deemphasis_taps_and_iir_against_scipy():
    from scipy.signal import lfilter
    a, b = orc.deemph_taps(20000)
    fs, tau = 20000.0, 50e-6
    w_ca = 2 * fs * float(np.tan(np.float32(1 / tau / (2 * fs))))
    k = -w_ca / (2 * fs)
    assert np.allclose(a, [1.0, -(1 + k) / (1 - k)], rtol=1e-6) and np.allclose(b, [-k / (1 - k)] * 2, rtol=1e-6)
    assert abs(sum(b) / sum(a) - 1.0) < 1e-9          # unity gain at DC


@pytest.mark.parametrize("kind,fw", [("nbfm", 5000), ("nbfm", 2500), ("am", 5000), ("wbfm", 75000)])
def test_analog_chain_recovers_the_modulating_tone(kind, fw):
    x, _ = sig.make_analog(kind, n=600000, seed=1)
    r = orc.demod_analog(x, kind, filter_width=fw)
    assert r["filtered"].size == (120000 if kind == "wbfm" else 12000)
    a = r["audio"][800:4000].astype(np.float64)
    spec = np.abs(np.fft.rfft(a * np.hanning(a.size)))
    assert abs((np.argmax(spec[5:]) + 5) * 8000.0 / a.size - 713.0) < 5.0


def test_analog_idle_channel_is_gated_away():
    x, _ = sig.make_analog("nbfm", n=400000, seed=1, gap=(100000, 300000))
    y, _ = sig.make_analog("nbfm", n=400000, seed=1)
    assert orc.demod_analog(x, "nbfm")["audio"].size < orc.demod_analog(y, "nbfm")["audio"].size


# ---- SSB receiver: cessb clipper / stretcher definitions and the chain
def test_cessb_clipper_limits_the_magnitude_and_keeps_the_phase():
    lib = orc.lib
    rng = np.random.default_rng(1)
    x = ((rng.standard_normal(500) + 1j * rng.standard_normal(500)) * 0.8).astype(np.complex64)
    y = np.zeros_like(x)
    lib.orc_cessb_clipper(x.ctypes.data_as(orc.C.c_void_p), orc.C.c_size_t(x.size), orc.C.c_float(0.95), y.ctypes.data_as(orc.C.c_void_p))
    assert np.all(np.abs(y) <= 0.95 * (1 + 1e-5))
    small = np.abs(x) < 0.9
    assert np.allclose(y[small], x[small], atol=2e-3)                       # (fast_atan2f is a 2e-3 rad LUT)
    assert np.allclose(np.angle(y * np.conj(x)), 0.0, atol=2e-3)


def test_cessb_stretcher_emits_whole_chunks_and_divides_by_the_five_point_envelope():
    lib = orc.lib
    lib.orc_cessb_stretcher.restype = orc.C.c_size_t
    rng = np.random.default_rng(2)
    x = ((rng.standard_normal(3000) + 1j * rng.standard_normal(3000)) * 0.3).astype(np.complex64)
    y = np.zeros_like(x)
    n = lib.orc_cessb_stretcher(x.ctypes.data_as(orc.C.c_void_p), orc.C.c_size_t(x.size), y.ctypes.data_as(orc.C.c_void_p))
    assert n == 2048                                                        # 1024 floor((3000 - 2) / 1024)
    assert lib.orc_cessb_stretcher(x.ctypes.data_as(orc.C.c_void_p), orc.C.c_size_t(1025), y.ctypes.data_as(orc.C.c_void_p)) == 0
    mag = np.abs(np.concatenate([np.zeros(2, np.complex64), x]))
    env = np.max(np.stack([mag[k:k + 2048] for k in range(5)]), axis=0)     # |x[k-2 .. k+2]|
    h = (np.maximum(env * np.float32(1 / (np.sqrt(0.5) / 2)), 1.0) - 1.0) * 2.0 + 1.0
    lib.orc_cessb_stretcher(x.ctypes.data_as(orc.C.c_void_p), orc.C.c_size_t(x.size), y.ctypes.data_as(orc.C.c_void_p))
    assert np.allclose(y[:2048], x[:2048] / h, rtol=1e-5, atol=1e-7)


def test_band_pass_2_has_unity_gain_at_the_band_centre():
    t = orc.band_pass_2(1, 8000, 200, 2700, 200, 90, orc.WIN_BH)
    H = np.abs(np.fft.rfft(t, 16384))
    f = np.fft.rfftfreq(16384, 1 / 8000)
    assert abs(H[np.argmin(abs(f - 1450))] - 1.0) < 1e-4 and H[np.argmin(abs(f - 3300))] < 1e-4 and H[0] < 2e-3


@pytest.mark.parametrize("lsb", [False, True])
def test_ssb_chain_recovers_the_tones_and_rejects_the_other_sideband(lsb):
    x = sig.make_ssb(n=800000, seed=1, lsb=lsb)
    a = orc.demod_ssb(x, sb=int(lsb))["audio"]
    assert a.size == 6144
    seg = a[1024:5120].astype(np.float64)
    spec = np.abs(np.fft.rfft(seg * np.hanning(seg.size)))
    assert abs(np.argmax(spec) * 8000.0 / seg.size - 713.0) < 4.0
    other = orc.demod_ssb(x, sb=int(not lsb))["audio"][1024:5120]
    assert np.sqrt(np.mean(other.astype(np.float64) ** 2)) < 0.02 * np.sqrt(np.mean(seg ** 2))


def test_literal_c4_freq_xlating_bank_equals_the_pfb_form():
    """BASELINE configs[3] literal (64 freq-xlating FIRs 1:64 with the PFB prototype, orc_demod_mmdvm_xlating_bank_4fsk) and the PFB
    form (orc_demod_mmdvm_multi_4fsk) are the same filter bank summed in different orders: on a channel that carries a signal the
    int16 FM outputs agree to 1 LSB and the 4FSK dibits are identical; planted dibits come back."""
    import sig
    N, n = 64, 64 * 2500
    fs = 25000.0 * N
    rng = np.random.default_rng(64)
    iq = (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    t = np.arange(n)
    planted = {}
    for c, seed in ((3, 5), (40, 6)):
        x, d = sig.make_4fsk(nsym=int(n / fs * 4800) - 2, seed=seed, amp=0.4, noise=0.0, fs=fs)
        f0 = c * 25000.0 if c <= N // 2 else (c - N) * 25000.0
        m = min(n, x.size)
        iq[:m] += (x[:m] * np.exp(2j * np.pi * f0 * t[:m] / fs)).astype(np.complex64)
        planted[c] = d
    a16, _, adib = orc.demod_mmdvm_xlating_bank_4fsk(iq, N)
    p16, pdib = orc.demod_mmdvm_multi_4fsk(iq, N)
    assert a16.shape == p16.shape
    for c, d in planted.items():
        assert np.abs(a16[c, 100:-5].astype(int) - p16[c, 100:-5].astype(int)).max() <= 1
        assert np.array_equal(adib[c], pdib[c])
        g = adib[c].reshape(-1, 2)
        g = g[:, 0] * 2 + g[:, 1]
        assert max(np.mean(g[k:k + 400] == d[:400]) for k in range(60)) > 0.99


def test_conjugate_pair_contract_of_the_2fsk_discriminator_filters():
    """gr_demod_2fsk's upper / lower band-pass filters (gr_demod_2fsk.cpp:86-89) are a conjugate pair bit for bit; the product runs the
    shared real-tap chains once (orc_fir_ccc_conj_pair, kernels_ff.hip).  Definition test: both outputs within 1e-5 of RMS of the float64
    filters, and within float rounding of two independent orc_fir_ccc; a pair that is NOT conjugate takes the generic path exactly."""
    rng = np.random.default_rng(5)
    x = ((rng.standard_normal(4000) + 1j * rng.standard_normal(4000)) * 0.3).astype(np.complex64)
    for fs, w in ((20000, 2000), (20000, 2500), (200000, 20000)):
        up = orc.complex_band_pass(1, fs, -w, 0, w, orc.WIN_BH)
        lo = orc.complex_band_pass(1, fs, 0, w, w, orc.WIN_BH)
        assert np.array_equal(lo.view(np.uint32), np.conj(up).view(np.uint32))          # the premise
        ou, ol = orc.fir_ccc_conj_pair(x, up, lo)
        for got, taps in ((ou, up), (ol, lo)):
            want = np.convolve(x.astype(np.complex128), taps.astype(np.complex128))[: x.size]
            rms = np.sqrt(np.mean(np.abs(want) ** 2))
            assert np.max(np.abs(got - want)) < 1e-5 * rms
            assert np.max(np.abs(got - orc.fir_ccc(x, taps))) < 4e-6 * rms
    lo2 = lo.copy(); lo2[3] += np.float32(1e-3)
    ou, ol = orc.fir_ccc_conj_pair(x, up, lo2)
    assert np.array_equal(ou.view(np.uint32), orc.fir_ccc(x, up).view(np.uint32))
    assert np.array_equal(ol.view(np.uint32), orc.fir_ccc(x, lo2).view(np.uint32))
