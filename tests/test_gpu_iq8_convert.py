"""The 8-bit conversion helper of engine.hpp alone on the device (tests/host/iq8_probe.hip, built with the product's flags from the product's
header) over all 65 536 input words, for sc8 and for cu8 under the parameter pairs of tests/test_iq8_definition.py: bit for bit the numpy rule
(u.astype(f32) - f32(bias)) * f32(scale), which for sc8 is v.astype(f32) * f32(scale)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_iq8_definition import PAIRS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "host", "libqrl_iq8_probe.so")
IN_SC8, IN_CU8 = 2, 3
F = np.float32


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "iq8_probe"])
    lib = C.CDLL(PROBE)
    lib.qrl_probe_iq8_to_f2.restype = C.c_int
    lib.qrl_probe_iq8_to_f2.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    return lib


def _run(lib, fmt, bias, scale):
    w = np.arange(65536, dtype=np.uint16)
    re, im = np.empty(65536, F), np.empty(65536, F)
    err = lib.qrl_probe_iq8_to_f2(w.ctypes.data, w.size, fmt, C.c_float(bias), C.c_float(scale), re.ctypes.data, im.ctypes.data)
    assert err == 0, "HIP error %d" % err
    return w, re, im


def _same(dev, ref, what):
    bad = np.flatnonzero(dev.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, "%s: %d of 65536 words differ, first word 0x%04x: device %r, numpy %r" % (what, bad.size, bad[0], dev[bad[0]], ref[bad[0]])


@pytest.mark.parametrize("scale", [p[0] for p in PAIRS])
def test_sc8_words(probe, scale):
    """the library hands the unsigned path the bias 128 for sc8: (float)(uint8)(v ^ 0x80) - 128 is (float)v"""
    w, re, im = _run(probe, IN_SC8, 128.0, scale)
    lo, hi = (w & 0xff).astype(np.uint8).view(np.int8), (w >> 8).astype(np.uint8).view(np.int8)
    _same(re, lo.astype(F) * F(scale), "sc8 I at scale %r" % scale)
    _same(im, hi.astype(F) * F(scale), "sc8 Q at scale %r" % scale)


@pytest.mark.parametrize("scale,bias", PAIRS)
def test_cu8_words(probe, scale, bias):
    w, re, im = _run(probe, IN_CU8, bias, scale)
    lo, hi = (w & 0xff).astype(np.uint8), (w >> 8).astype(np.uint8)
    _same(re, (lo.astype(F) - F(bias)) * F(scale), "cu8 I at (%r, %r)" % (scale, bias))
    _same(im, (hi.astype(F) - F(bias)) * F(scale), "cu8 Q at (%r, %r)" % (scale, bias))
