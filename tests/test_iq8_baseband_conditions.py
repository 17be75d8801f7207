"""The conditions under which tests/test_gpu_iq8_baseband.py means something, from the oracle alone (CPU): every one of the thirteen receivers
of tests/sc16_baseband.py, quantised to 8 bits as tests/iq8_baseband.py does it -- the largest component between 64 and 127 counts, nothing
saturated, the scale the inverse of the gain -- still gives the oracle, on the converted floats, what tests/sc16_baseband.py's refs() asks for:
more than 100 filtered items, at least 16 bits on every bit port, the squelch open on exactly streams 0 and 2."""
import numpy as np
import pytest

import iq8_baseband as ib


def test_all_thirteen_readers_are_there():
    assert len(ib.CASES) == 13 and ib.CASES is __import__("sc16_baseband").CASES
    assert sum("1:50" in ib.case(name)["reader"] for name in ib.CASES) >= 4


@pytest.mark.parametrize("per_stream", [False, True], ids=["shared_offset", "per_stream_offsets"])
@pytest.mark.parametrize("name", sorted(n for n in ib.CASES if "like" not in ib.CASES[n]))
def test_quantisation_uses_the_top_bit_and_saturates_nothing(name, per_stream):
    v8, u8, v16, conv, _ = ib.inputs(name, per_stream)
    n = v8.shape[1] // 2
    assert n % 8 == 0 and conv.shape == (ib.B, n)
    peak = int(np.abs(v8.astype(np.int32)).max())
    assert 64 <= peak <= 127, peak
    assert int(u8.min()) >= 0 and int(u8.max()) <= 254 and int(np.abs(v16.astype(np.int32)).max()) <= 127 * 256 + 128
    (g0, s0), (g1, s1) = ib.levels(name, per_stream)
    assert s0 == np.float32(1.0 / g0) and s1 == np.float32(1.0 / g1)
    # the conversion the ABI defines, call by call, is what the oracle is fed
    f = conv.view(np.float32)
    for start, k, fmt, step in ib.calls(n):
        scale, bias, scale16 = ib.step_settings(name, per_stream, step)
        sl = slice(2 * start, 2 * (start + k))
        if fmt == ib.CU8:
            want = (u8[:, sl].astype(np.float32) - np.float32(bias)) * np.float32(scale)
        elif fmt == ib.SC16:
            want = v16[:, sl].astype(np.float32) * np.float32(scale16)
        else:
            want = ((v8[:, sl].view(np.uint8) ^ np.uint8(0x80)).astype(np.float32) - np.float32(128.0)) * np.float32(scale)     # the device's path for sc8
        assert np.array_equal(f[:, sl].view(np.uint32), want.view(np.uint32)), (start, fmt)


@pytest.mark.parametrize("name", sorted(n for n in ib.CASES if "like" not in ib.CASES[n]))
def test_oracle_on_the_converted_floats_meets_the_conditions(name):
    """(refs() asserts them; the per-stream variant differs in the carrier offsets only and is asserted by the GPU test before it compares)"""
    out = ib.refs(name, False)
    ib.check_refs(name, out)
    assert len(out) == ib.B
