"""The oracle's back-end interpolator (orc_tx_interp) at the device rates above 64 Msps against its float64 definition, and the public
header's statement of the transmitters' rate range (2 .. 183 Msps, as on the receivers)."""
import os
import re

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rate", [65000000, 100000000, 183000000])
def test_tx_interp_matches_float64_definition(rate):
    """rational_resampler_ccf(I, 1, low_pass(I, rate, 480k, 20k, BH)): zero-stuffing by I, then the FIR with the same float32 taps, in float64.
    The project's rule for a summation contract: the largest error is at most 1e-5 of the output's RMS."""
    I = rate // 1000000
    rng = np.random.default_rng(I)
    x = (rng.standard_normal(500) + 1j * rng.standard_normal(500)).astype(np.complex64)
    h = orc.low_pass(I, rate, 480000, 20000, orc.WIN_BH)
    assert h.size // I == 209 and (h.size + I - 1) // I <= 210       # 209 taps per phase, 210 for the first nt % I phases
    y = orc.tx_interp(x, rate)
    assert y.size == x.size * I
    up = np.zeros(x.size * I, np.complex128)
    up[::I] = x
    ref = np.convolve(up, h.astype(np.float64))[:y.size]
    err = np.abs(y - ref).max() / np.sqrt(np.mean(np.abs(ref) ** 2))
    print("rate %d: %d taps, largest error %.2e of the output RMS" % (rate, h.size, err))
    assert err <= 1e-5


def test_header_names_the_transmitters_rate_range():
    """both device_samp_rate comments (qrl_mod_config, qrl_amod_config) name 183e6 and no longer 64e6"""
    text = open(os.path.join(ROOT, "include", "qrl_hip.h")).read()
    for struct in ("qrl_mod_config", "qrl_amod_config"):
        m = re.search(r"typedef struct(?: %s)? \{([^}]*)\} %s;" % (struct, struct), text)
        assert m, struct
        body = m.group(1)
        assert "device_samp_rate" in body
        assert "183e6" in body, "%s: device_samp_rate does not name 183e6" % struct
        assert "64e6" not in body, "%s still names 64e6" % struct
