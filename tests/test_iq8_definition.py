"""The 8-bit sample formats' arithmetic, on the CPU and exhaustive over the 256 codes.

sc8: x = (float)v * scale.  cu8: x = ((float)u - bias) * scale: one exact conversion, one f32 subtract, one rounded f32 multiply.  The device runs
one path for both -- u = byte ^ 0x80 for sc8 with the bias 128 -- which rests on an identity checked here bit for bit.  The numpy float32 rule the
GPU tests compare against is held to the float64 value of the contract: the subtract is one correctly rounded f32 operation (exact for two of the
three pairs), and the product is the correctly rounded product of THAT float and the scale."""
import numpy as np

F = np.float32
# (scale, bias): the defaults; what gr-osmosdr's RTL source is remembered to use (products that round); an arbitrary scale on the raw codes
PAIRS = [(float(F(1.0 / 128.0)), float(F(127.5))), (float(F(1.0 / 127.0)), float(F(127.4))), (float(F(0.0123)), 0.0)]
CODES_U = np.arange(256, dtype=np.uint8)
CODES_S = CODES_U.view(np.int8)


def test_signed_through_unsigned_identity():
    """(float)(uint8)(v ^ 0x80) - 128.0f == (float)v bit for bit, for every int8 v"""
    u = (CODES_S.view(np.uint8) ^ np.uint8(0x80))
    got = u.astype(F) - F(128.0)
    want = CODES_S.astype(F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.any(np.signbit(got[want == 0]))            # 128 - 128 is +0, as (float)0 is


def _rule(u, scale, bias):
    return (u.astype(F) - F(bias)) * F(scale)


def _ulp(x):
    return np.spacing(np.abs(x).astype(F)).astype(np.float64)


def test_numpy_rule_is_the_rounded_float64_value():
    """within one float32 rounding of (u - bias) * scale in float64 (bias and scale the float32 parameters); and step by step: the difference is the
    float32 nearest to the exact difference, the product the float32 nearest to the exact product of that difference and the scale"""
    for scale, bias in PAIRS:
        got = _rule(CODES_U, scale, bias)
        u64, b64, s64 = CODES_U.astype(np.float64), float(F(bias)), float(F(scale))
        exact = (u64 - b64) * s64                            # |u - bias| < 2^8, 24-bit operands: exact in float64 up to one rounding of the product
        assert np.all(np.abs(got.astype(np.float64) - exact) <= _ulp(got)), (scale, bias)
        diff = (u64 - b64).astype(F)                         # correctly rounded by the float64 -> float32 conversion (the float64 difference is exact)
        assert np.array_equal((CODES_U.astype(F) - F(bias)).view(np.uint32), diff.view(np.uint32)), (scale, bias)
        prod = (diff.astype(np.float64) * s64).astype(F)     # two 24-bit significands: the float64 product is exact, its conversion the correct rounding
        assert np.array_equal(got.view(np.uint32), prod.view(np.uint32)), (scale, bias)


def test_the_second_pair_makes_the_multiply_round():
    """(1 / 127, 127.4f): the products are not all exact -- without that the rounding of the multiply would not be exercised"""
    scale, bias = PAIRS[1]
    diff = CODES_U.astype(F) - F(bias)
    exact = diff.astype(np.float64) * float(F(scale))
    assert np.any(exact != _rule(CODES_U, scale, bias).astype(np.float64))
    # and the default pair is exact throughout: a power-of-two scale on half-integers
    scale0, bias0 = PAIRS[0]
    assert np.array_equal(_rule(CODES_U, scale0, bias0).astype(np.float64), (CODES_U.astype(np.float64) - 127.5) / 128.0)


def test_sc8_rule_is_the_unsigned_rule_at_bias_128():
    for scale, _ in PAIRS:
        a = CODES_S.astype(F) * F(scale)
        b = _rule(CODES_S.view(np.uint8) ^ np.uint8(0x80), scale, 128.0)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
