"""The device math primitives, each alone, against their oracle twins bit for bit (signed zeros included) over the input sets of
tests/devmath_points.py.  The device side is tests/host/devmath_probe.hip: devmath.hpp, engine.hpp and qrl_contracts.h as the kernels include
them, under the product's compiler flags, one entry per primitive.  Where the oracle gives a NaN the device must give one (payload not compared);
nothing else is allowed for.  tests/test_devmath_definition.py holds the oracle's side to float64 definitions on the same sets."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devmath_points as P
import orc
import qradiolink_amd as q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "host", "libqrl_devmath_probe.so")
F = np.float32
U = np.uint32
_p, _sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "devmath_probe"])
    lib = C.CDLL(PROBE)
    for name, args in {
        "sincos_rad": (_p, _sz, _p, _p), "sincos_turn": (_p, _sz, _p, _p), "fast_atan2": (_p, _p, _sz, _p, _p), "tanh_lut": (_p, _sz, _p, _p),
        "clip": (_p, _p, _sz, _p), "ted_error": (_p, _sz, _p, _p), "phase_wrap": (_p, _sz, _p), "det_log2": (_p, _sz, _p), "det_log10": (_p, _sz, _p),
        "f2_to_sc16": (_p, _p, _sz, C.c_float, _p, _p), "sc16_to_f2": (_p, _sz, C.c_float, _p, _p),
        "sc16_store_divergent": (_p, _p, _p, _p, C.c_uint32, C.c_uint32, _p, _p, _p),
    }.items():
        f = getattr(lib, "qrl_probe_" + name)
        f.restype, f.argtypes = C.c_int, list(args)
    return lib


def _ptr(a):
    return a.ctypes.data_as(_p)


def _call(lib, name, *args):
    keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
    err = getattr(lib, "qrl_probe_" + name)(*[_ptr(a) if isinstance(a, np.ndarray) else a for a in keep])
    assert err == 0, "%s: HIP error %d" % (name, err)


def _hex(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        a = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return "0x%0*x" % (2 * a.dtype.itemsize, int(a))


def assert_same_bits(what, dev, ref, *inputs):
    """dev == ref bit for bit; a NaN of the reference asks for a NaN of the device.  A failure shows the first offenders in hex."""
    dev, ref = np.ascontiguousarray(dev), np.ascontiguousarray(ref)
    assert dev.shape == ref.shape and dev.dtype == ref.dtype
    if ref.dtype.kind == "f":
        ok = (dev.view(U) == ref.view(U)) | (np.isnan(ref) & np.isnan(dev))
    else:
        ok = dev == ref
    if ok.all():
        return
    bad = np.flatnonzero(~ok.ravel())
    lines = ["%s: %d of %d points differ" % (what, bad.size, ok.size)]
    for i in bad[:8]:
        ins = ", ".join(_hex(np.asarray(a).ravel()[i]) for a in inputs)
        lines.append("  [%d] in (%s): device %s, oracle %s" % (i, ins, _hex(dev.ravel()[i]), _hex(ref.ravel()[i])))
    pytest.fail("\n".join(lines), pytrace=False)


def test_sincos_rad(probe):
    x = P.sincos_rad()
    c, s = np.empty_like(x), np.empty_like(x)
    _call(probe, "sincos_rad", x, x.size, c, s)
    rc, rs = orc.probe_sincosf(x)
    assert_same_bits("sincos_rad cos", c, rc, x)
    assert_same_bits("sincos_rad sin", s, rs, x)


def test_sincos_turn(probe):
    a = P.sincos_turn()
    c, s = np.empty(a.size, F), np.empty(a.size, F)
    _call(probe, "sincos_turn", a, a.size, c, s)
    rc, rs = orc.probe_sincos_turn(a)
    assert_same_bits("sincos_turn cos", c, rc, a)
    assert_same_bits("sincos_turn sin", s, rs, a)


def test_fast_atan2(probe):
    table = q.table("atan")
    assert np.array_equal(table.view(U), orc.table("atan", 257).view(U))
    y, x, _ = P.atan2()
    o = np.empty_like(y)
    _call(probe, "fast_atan2", y, x, y.size, table, o)
    assert_same_bits("fast_atan2", o, orc.probe_fast_atan2f(y, x), y, x)
    # both arguments infinite, or a NaN: the host's (int)NaN is undefined, so there is no oracle value; the device gives a NaN or an angle
    y, x = P.atan2_undefined_on_host()
    o = np.full(y.size, 99.0, F)
    _call(probe, "fast_atan2", y, x, y.size, table, o)
    assert np.all(np.isnan(o) | (np.abs(o) <= F(np.pi))), o


def test_tanh_lut(probe):
    table = q.table("tanh")
    assert np.array_equal(table.view(U), orc.table("tanh", 256).view(U))
    x = P.tanh()
    o = np.empty_like(x)
    _call(probe, "tanh_lut", x, x.size, table, o)
    assert_same_bits("tanh_lut", o, orc.probe_tanhf_lut(x), x)
    nan = P.f32([0x7fc00000, 0xffc00000, 0x7f800001])      # (int)NaN again: the device stays inside the table or gives +-1
    o = np.full(nan.size, 99.0, F)
    _call(probe, "tanh_lut", nan, nan.size, table, o)
    assert np.all(np.isin(o, np.concatenate([table, F([1.0, -1.0])]))), o


def test_clip(probe):
    x, lim = P.clip()
    o = np.empty_like(x)
    _call(probe, "clip", x, lim, x.size, o)
    assert_same_bits("branchless_clip", o, orc.probe_clip(x, lim), x, lim)


def test_ted_error(probe):
    u = P.ted_u()
    ff, cc = np.empty_like(u), np.empty_like(u)
    _call(probe, "ted_error", u, u.size, ff, cc)
    rff, rcc = orc.probe_ted_error(u)
    assert_same_bits("QRL_TED_MODMM_FF", ff, rff, u)
    assert_same_bits("QRL_TED_MODMM_CC", cc, rcc, u)


def test_phase_wrap(probe):
    x = P.phase_wrap()
    o = np.empty_like(x)
    _call(probe, "phase_wrap", x, x.size, o)
    assert_same_bits("phase_wrap", o, orc.probe_phase_wrap(x), x)


def test_det_log2(probe):
    x = P.det_log()
    o = np.empty_like(x)
    _call(probe, "det_log2", x, x.size, o)
    assert_same_bits("det_log2f", o, orc.probe_det_log2f(x), x)


def test_det_log10(probe):
    x = P.det_log()
    o = np.empty_like(x)
    _call(probe, "det_log10", x, x.size, o)
    assert_same_bits("det_log10f", o, orc.probe_det_log10f(x), x)


@pytest.mark.parametrize("scale", [float(s) for s in P.SC16_SCALES])
def test_f2_to_sc16(probe, scale):
    vi, vq = P.f2_to_sc16(scale)
    w, nclip = np.empty(vi.size, U), np.empty(vi.size, U)
    _call(probe, "f2_to_sc16", vi, vq, vi.size, C.c_float(scale), w, nclip)
    # the word: the oracle's float_to_short on each component (NaN -> 0 compared like everything else), I in the low half
    assert_same_bits("f2_to_sc16 word", w, P.sc16_pack(orc.probe_f2s(vi, scale), orc.probe_f2s(vq, scale)), vi, vq)
    # nclip has no twin in the oracle: the integer rule of devmath_points.sc16_rule, which test_devmath_definition.py holds the oracle's f2s to
    want = P.sc16_rule(vi, scale)[1].astype(U) + P.sc16_rule(vq, scale)[1].astype(U)
    assert_same_bits("f2_to_sc16 nclip", nclip, want, vi, vq)


@pytest.mark.parametrize("scale", [float(s) for s in P.SC16_IN_SCALES])
def test_sc16_to_f2(probe, scale):
    w = P.sc16_words()
    oi, oq = np.empty(w.size, F), np.empty(w.size, F)
    _call(probe, "sc16_to_f2", w, w.size, C.c_float(scale), oi, oq)
    # (float)v * scale: one exact conversion, one rounded multiply -- the floats the sc16 chain tests hand the oracle
    lo = (w & 0xffff).astype(np.uint16).view(np.int16).astype(F)
    hi = (w >> 16).astype(np.uint16).view(np.int16).astype(F)
    with np.errstate(under="ignore"):
        assert_same_bits("sc16_to_f2 I", oi, lo * F(scale), w)
        assert_same_bits("sc16_to_f2 Q", oq, hi * F(scale), w)


def test_sc16_store_divergent(probe):
    d = P.sc16_store_divergent()
    vi, vq, valid, branch, n, batch = d["vi"], d["vq"], d["valid"], d["branch"], d["n"], d["batch"]
    out = np.full((batch, n), P.STORE_SENTINEL, U)
    clip = np.full(batch, P.STORE_CLIP_START, U)
    _call(probe, "sc16_store_divergent", vi, vq, valid, branch, n, batch, P.STORE_SCALES, out, clip)
    calls = branch < 4                                       # lanes that reach a sc16_store at all
    live = calls & (valid != 0)
    sc = np.where(calls, P.STORE_SCALES[np.minimum(branch, 3)], F(1.0))
    word = P.sc16_pack(orc.probe_f2s(vi.ravel(), sc.ravel()), orc.probe_f2s(vq.ravel(), sc.ravel())).reshape(batch, n)
    assert_same_bits("sc16_store words", out, np.where(live, word, P.STORE_SENTINEL), vi, vq, valid, branch)
    ncl = P.sc16_rule(vi, sc)[1].astype(np.int64) + P.sc16_rule(vq, sc)[1].astype(np.int64)
    want = (int(P.STORE_CLIP_START) + np.where(live, ncl, 0).sum(axis=1)).astype(U)      # the plain sum over the valid lanes
    assert want.min() > P.STORE_CLIP_START + 50
    assert_same_bits("sc16_store clip counters", clip, want, np.arange(batch))
