"""What the sc8 output tests on the device take for granted, asserted on the CPU from the oracle alone (tests/sc8_output_cases.py): the saturation
cases clip where the tests need it, the rates of test_gpu_sc8_tx_rates.py reach both back-end interpolators and the edges of a phase tile, and the
8-bit stream of the loopback decodes."""
import numpy as np

import sc8_output_cases as K
import test_gpu_tx_rates as R
from test_gpu_sc8_tx_rates import RATES


def test_saturation_cases_clip_partly_in_every_stream_and_twice_in_some_samples():
    for parts in (K.mod_saturation()[1], K.amod_saturation()[1]):
        K.saturation_preconditions(parts[0])
        K.saturation_preconditions(parts[2])


def test_one_stream_of_the_silent_case_clips_nowhere():
    K.silent_preconditions(K.silent_stream()[1])


def test_every_other_terminal_kernel_clips_in_a_ragged_last_workgroup():
    for name in K.OTHER_KERNELS:
        K.clip_case_preconditions(K.clip_case(name)[2])


def test_rates_reach_both_interpolators_and_the_tile_edges():
    assert R.MFMA_MIN_RATE == 4000000 and [r < R.MFMA_MIN_RATE for r in RATES] == [True, True, False, False, False]
    assert 33 % 32 == 1 and -(-183 // 32) == 6 and 183 % 32 == 23       # a second tile of one phase; six tiles, the last of 23 phases
    per_call = [32 * c for c in R.CUTS]                               # samples at 1 Msps; the interpolator walks blocks of 128 from the call's first
    assert [n % 128 // 32 for n in per_call] == [1, 3, 3, 0] and per_call[-1] > 128
    K.saturation_preconditions(R._ref(RATES[0], 4.0))


def test_the_quantised_loopback_stream_decodes():
    data, payloads, codes, rx = K.loopback()
    assert codes[0].shape[0] % 8 == 0, "the receiver takes calls of a multiple of 8 samples"
    for b in range(K.B):
        assert 100 < np.abs(codes[b].astype(np.int32)).max() <= 127 and K.conv8(codes[b].astype(np.float32).view(np.complex64).ravel(), 1.0)[1] == 0
        assert len(payloads[b]) == K.LOOP_FRAMES and K.recovered(rx[b]["bits_a"], rx[b]["bits_b"], payloads[b]), "stream %d does not decode in the oracle" % b
    assert len({p for ps in payloads for p in ps}) == K.B * K.LOOP_FRAMES
