"""The oracle's math primitives against float64 definitions, over the input sets of tests/devmath_points.py (CPU only).
tests/test_gpu_devmath.py holds the device's twins to the oracle bit for bit on the same sets; this file anchors the other end, and asserts
from the oracle alone that the sets reach the paths they are aimed at.  Every bound is against the float64 definition, never the device.
Measured figures (this set, gcc -O3 -ffp-contract=off) stand next to the bounds that come from them."""
import numpy as np
import pytest

import devmath_points as P
import orc

F = np.float32
TWO_PI = 2 * np.pi


def _ulp(v):
    """unit in the last place of the float32 nearest v (float64)"""
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(F)).astype(np.float64)


# ---- sincos ---------------------------------------------------------------------------------------------------------------------
# |x| <= 10: the 3e-7 of test_oracle.py.  10 < |x| <= 1e5: measured maximum 8.93e-8 (the two-term Cody-Waite constant is exact to 1e-15 a quarter
# turn, and fmaf keeps k * PIO2_HI unrounded, so the reduction does not degrade up there); twice that is asserted.
SINCOS_NEAR_BOUND = 3e-7
SINCOS_FAR_MEASURED = 8.93e-8


def test_sincosf_against_float64():
    x = P.sincos_rad()
    c, s = orc.probe_sincosf(x)
    xd = x.astype(np.float64)
    err = np.maximum(np.abs(c - np.cos(xd)), np.abs(s - np.sin(xd)))
    near = np.abs(xd) <= 10
    print("sincosf: n %d, max err %.4g on |x| <= 10, %.4g beyond (to %g)" % (x.size, err[near].max(), err[~near].max(), np.abs(xd).max()))
    assert np.abs(xd).max() == P.SINCOS_FAR and (~near).sum() > 100000
    assert err[near].max() < SINCOS_NEAR_BOUND
    assert err[~near].max() < 2 * SINCOS_FAR_MEASURED
    c0, s0 = orc.probe_sincosf(F([0.0, -0.0]))
    assert c0.tolist() == [1.0, 1.0] and s0.tolist() == [0.0, 0.0]


def test_sincosf_set_reaches_every_quadrant_and_both_signs_of_k():
    x = P.sincos_rad()
    k = np.rint(x.astype(np.float64) * (2 / np.pi)).astype(np.int64)
    for sign in (1, -1):
        for q in range(4):
            assert np.any((np.sign(k) == sign) & ((k & 3) == q)), (sign, q)
    assert k.max() > 60000 and k.min() < -60000 and np.abs(k).max() < 2 ** 31
    # the rintf ties: points on both sides of odd multiples of pi/4, 4 ulps around each up to |k| = 128
    odd = F(np.arange(1, 128, 2) * (np.pi / 4))
    xs = np.sort(x)
    for v in odd:
        i = np.searchsorted(xs, v)
        assert xs[i - 4] < v <= xs[i + 3] and xs[i + 3] - xs[i - 4] <= 8 * np.spacing(v)


def test_sincos_turn_against_float64():
    a = P.sincos_turn()
    c, s = orc.probe_sincos_turn(a)
    th = TWO_PI * (a.astype(np.float64) / 2.0 ** 64)      # the low 32 bits move the angle by at most 1.5e-9 rad
    err = max(np.abs(c - np.cos(th)).max(), np.abs(s - np.sin(th)).max())
    print("sincos_turn: n %d, max err %.4g" % (a.size, err))
    assert err < SINCOS_NEAR_BOUND
    top = (a >> np.uint64(32)).astype(np.int64)
    q = ((top + 0x20000000) >> 30) & 3
    assert set(q) == {0, 1, 2, 3}
    for m in range(8):                                     # both sides of every multiple of 2^29, low half zero and all-ones
        for low in (0, 0xffffffff):
            sel = top[(a & np.uint64(0xffffffff)) == np.uint64(low)]
            d = (sel - (m << 29) + (1 << 31)) % (1 << 32) - (1 << 31)
            assert {-1, 0, 1} <= set(d[np.abs(d) <= 8]), (m, low)


# ---- fast_atan2 -----------------------------------------------------------------------------------------------------------------
# The whole set keeps the 2e-5 of test_oracle.py.  On the aimed points (the small-z threshold, 4 ulps around every breakpoint) the measured
# maximum is 3.02e-7; twice that is asserted.  fast_atan2f takes y = -0 for positive (y >= 0), so (-0, -1) gives +pi where atan2 gives -pi:
# the same direction, and the error is the distance on the circle.
ATAN2_BOUND = 2e-5
ATAN2_AIMED_MEASURED = 3.02e-7


def _circle(d):
    return np.abs((d + np.pi) % TWO_PI - np.pi)


def test_fast_atan2f_against_float64():
    y, x, n_aimed = P.atan2()
    o = orc.probe_fast_atan2f(y, x)
    err = _circle(o.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    origin = (y == 0) & (x == 0)                           # fast_atan2f(+-0, +-0) is +0 whatever the signs (atan2 gives 0 or +-pi)
    assert origin.sum() == 4 and np.all(o[origin].view(np.uint32) == 0)
    err[origin] = 0
    print("fast_atan2f: n %d, max err %.4g; aimed n %d, max err %.4g" % (y.size, err.max(), n_aimed, err[:n_aimed].max()))
    assert not np.any(np.isnan(o)) and np.all(np.abs(o) <= F(np.pi))
    assert err.max() < ATAN2_BOUND
    assert err[:n_aimed].max() < 2 * ATAN2_AIMED_MEASURED


def test_fast_atan2f_set_reaches_both_branches_every_index_and_the_threshold():
    y, x, _ = P.atan2()
    ya, xa = np.abs(y), np.abs(x)
    ok = (ya > 0) | (xa > 0)
    with np.errstate(all="ignore"):
        z = np.where(ya < xa, ya / xa, xa / ya)[ok]        # float32 division, as the function does it
    table = z.astype(np.float64) >= 0.003921569
    assert table.any() and (~table).any()
    index = (z[table] * F(255.0)).astype(np.int64) & 0xff
    # every index the table branch can take: 0.003921569 lies above 1 / 255, so z * 255 >= 1 on that branch: index 0 cannot occur
    # and T[0] is never read (shown here from the first float of the branch); index 255 (z = 1) reads T[256]
    assert P.f32(P.ATAN_THRESHOLD_BITS) * F(255.0) >= 1
    assert set(index) == set(range(1, 256))
    zb = z.view(np.uint32)
    for b in (P.ATAN_THRESHOLD_BITS - 1, P.ATAN_THRESHOLD_BITS):      # the last float under the threshold and the first one at or over it
        assert np.any(zb == b)
    assert np.float64(P.f32(P.ATAN_THRESHOLD_BITS - 1)) < 0.003921569 <= np.float64(P.f32(P.ATAN_THRESHOLD_BITS))
    for first in (True, False):                            # both branches under all four sign pairs
        for sy in (False, True):
            for sx in (False, True):
                assert np.any(((xa > ya) == first) & (np.signbit(y) == sy) & (np.signbit(x) == sx) & (ya != xa))
    assert np.any((ya == xa) & ok)
    with np.errstate(invalid="ignore"):
        a255 = z * F(255.0)
    frac = a255 - np.floor(a255)                           # z * 255 just under and just over an integer
    assert np.any((frac > 0) & (frac < 1e-4)) and np.any(frac > 1 - 1e-4) and np.any((frac == 0) & (a255 >= 1))


# ---- tanh_lut -------------------------------------------------------------------------------------------------------------------
def test_tanhf_lut_against_float64():
    x = P.tanh()
    o = orc.probe_tanhf_lut(x)
    xd = x.astype(np.float64)
    # the table holds tanh((i - 128) / 64) to 8 decimals and x falls in a step 1/64 wide: |error| <= 1/64 (slope <= 1) + 5e-9 inside (-2, 2]
    inside = (xd > -2) & (xd <= 2)
    assert np.abs(o[inside] - np.tanh(xd[inside])).max() <= 1 / 64 + 1e-8
    assert np.all(o[xd > 2] == 1.0) and np.all(o[xd <= -2] == -1.0)
    index = np.clip((F(128.0) + F(64.0) * x[inside]).astype(np.int64), 0, 255)
    assert set(index) == set(range(256))                   # every entry of the table is read
    assert np.array_equal(o[inside], orc.table("tanh", 256)[index])
    assert np.any(x == F(2.0)) and np.any(x == np.nextafter(F(2.0), F(3.0))) and np.any(x == np.nextafter(F(2.0), F(0.0)))
    assert np.any(x == F(-2.0)) and np.any(np.isposinf(x)) and np.any(np.isneginf(x))


# ---- clip / TED error -----------------------------------------------------------------------------------------------------------
def _clip_bound(x, lim):
    """0.5 (|x + L| - |x - L|) in float32: the two sums each round by at most half an ulp of |x| + L, their difference by half an ulp of
    itself (<= 2 L <= 2 (|x| + L)), the halving is exact: in all at most 1.5 ulp(|x| + L) -- which is why a huge x clips to 0, as upstream's does"""
    return 1.5 * _ulp(np.abs(x) + lim)


def test_branchless_clip_against_float64():
    x, lim = P.clip()
    o = orc.probe_clip(x, lim).astype(np.float64)
    xd, ld = x.astype(np.float64), lim.astype(np.float64)
    fin = np.isfinite(xd) & np.isfinite(_ulp(np.abs(xd) + ld))
    ref = np.clip(xd, -ld, ld)
    assert np.all(np.abs(o[fin] - ref[fin]) <= _clip_bound(xd[fin], ld[fin]))
    assert np.all(np.isnan(o[np.isinf(xd)]))               # inf - inf
    exact = fin & (np.abs(xd) >= 2.0 ** -20 * ld) & (np.abs(xd) <= 3 * ld) & (ld == 1.0)
    assert exact.sum() > 3000 and np.abs(o[exact] - ref[exact]).max() <= 2.0 ** -23
    for l in P.CLIP_LIMITS:                                # both sides of both limits, ties and zeros are in the set
        v = x[lim == l]
        assert np.any(v == l) and np.any(v == np.nextafter(l, F(np.inf))) and np.any(v == np.nextafter(l, F(0)))
        assert np.any(v == -l) and np.any(v == 0) and np.any(np.isinf(v))


def test_ted_error_against_float64():
    u = P.ted_u()
    ff, cc = orc.probe_ted_error(u)
    ud = u.astype(np.float64)
    fin = np.isfinite(ud)
    # the contract of include/qrl_contracts.h: symbol_sync_ff halves before the clip, symbol_sync_cc does not halve
    assert np.all(np.abs(ff[fin] - np.clip(ud[fin] / 2, -1, 1)) <= _clip_bound(ud[fin] / 2, 1.0))
    assert np.all(np.abs(cc[fin] - np.clip(ud[fin], -1, 1)) <= _clip_bound(ud[fin], 1.0))
    assert np.all(np.isnan(ff[~fin])) and np.all(np.isnan(cc[~fin]))
    assert np.any(np.abs(ud) > 2) and np.any((np.abs(ud) > 1) & (np.abs(ud) < 2)) and np.any(np.abs(ud) < 1)
    assert np.array_equal(ff.view(np.uint32), orc.probe_clip(u / F(2.0), np.ones(u.size, F)).view(np.uint32))


# ---- phase_wrap -----------------------------------------------------------------------------------------------------------------
def test_phase_wrap_against_float64():
    x = P.phase_wrap()
    o = orc.probe_phase_wrap(x).astype(np.float64)
    xd = x.astype(np.float64)
    lim = np.float64(F(TWO_PI))
    inside = np.abs(xd) <= lim
    assert np.array_equal(o[inside], xd[inside])           # in range (the float limits included): untouched
    assert np.all(np.abs(o) <= lim)
    turns = np.rint((xd - o) / TWO_PI)
    # a whole number of turns, each one rounded to float once (half an ulp of a value no larger than |x|)
    assert np.all(np.abs(xd - turns * TWO_PI - o) <= np.abs(turns) * 0.5 * _ulp(xd) + 1e-12)
    # and no turn too many: one turn back is out of range again
    out = ~inside
    back = o[out] + np.sign(xd[out]) * TWO_PI
    assert np.all(np.abs(back) > lim - 0.5 * _ulp(xd[out]) * np.abs(turns[out]) - 1e-6)
    assert np.all(np.abs(turns[out]) >= 1) and set(np.abs(turns).astype(int)) >= {0, 1, 2, 3}


def test_phase_wrap_set_lays_out_the_waves():
    x = P.phase_wrap()
    lim = F(TWO_PI)
    full = x[: x.size // P.WAVE * P.WAVE].reshape(-1, P.WAVE)
    out = np.abs(full) > lim
    count = out.sum(axis=1)
    assert np.sum(count == 0) >= 256 and np.sum(count == P.WAVE) >= 24
    for lane in (0, 31, 32, 63):
        assert np.sum((count == 1) & out[:, lane]) >= 24, lane
    turns = np.floor(np.abs(full.astype(np.float64)) / TWO_PI)
    assert np.any([len(set(t[o])) >= 3 and not o.all() for t, o in zip(turns, out)])      # lanes of one wave that need 0, 1, 2, 3 turns
    for k in (1, 2):                                        # the floats on either side of +-2 pi and +-4 pi
        v = F(k * TWO_PI)
        for s in (F(1), F(-1)):
            assert np.any(x == s * v) and np.any(x == s * np.nextafter(v, F(np.inf))) and np.any(x == s * np.nextafter(v, F(0)))
    assert x.size % P.WAVE != 0 and np.abs(x).max() <= 8 * np.pi + 1e-4


# ---- det_log2f / det_log10f -----------------------------------------------------------------------------------------------------
# Measured on this set (2.1 million points): maximum error 0.500000 ulp of the float result for both, no point beyond half an ulp that float64
# can tell from a tie.  The cap on the share beyond half an ulp is 1e-4; "beyond" leaves float64's own error in log2 / log10 out (1e-9 ulp of a float).
LOG_HALF_ULP_SHARE = 1e-4


@pytest.mark.parametrize("name", ["log2", "log10"])
def test_det_log_against_float64(name):
    f, g = {"log2": (orc.probe_det_log2f, np.log2), "log10": (orc.probe_det_log10f, np.log10)}[name]
    x = P.det_log()
    o = f(x)
    pos = (x > 0) & np.isfinite(x)
    t = g(x[pos].astype(np.float64))
    eu = np.abs(o[pos].astype(np.float64) - t) / _ulp(t)
    share = np.mean(eu > 0.5 + 1e-8)
    print("det_%sf: n %d, max err %.6f ulp, share beyond half an ulp %.3g" % (name, pos.sum(), eu.max(), share))
    assert eu.max() <= 1.0
    assert share < LOG_HALF_ULP_SHARE
    # the ends of the domain
    zero, big = (-127.0, 127.0) if name == "log2" else (-np.inf, np.inf)
    assert np.all(o[x == 0] == zero) and np.all(o[np.isposinf(x)] == big)
    assert np.all(np.isnan(o[(x < 0) | np.isnan(x)]))
    assert np.sum(x == 0) == 2 and np.any(x < 0) and np.any(np.isneginf(x)) and np.any(np.isnan(x))


def test_det_log_set_takes_the_subnormal_path_and_the_fold():
    x = P.det_log()
    b = x.view(np.uint32)
    pos = (x > 0) & np.isfinite(x)
    sub = pos & (b < 0x00800000)
    assert sub.sum() > 1000 and np.any(b == 1) and np.any(b == 0x007fffff) and np.any(b == 0x00800000) and np.any(b == 0x7f7fffff)
    mant = b[pos & ~sub] & 0x7fffff
    assert np.mean(mant > P.LOG_FOLD_MANTISSA) > 0.3 and np.mean(mant <= P.LOG_FOLD_MANTISSA) > 0.3
    for e in range(1, 255):                                 # every exponent: the fold mantissa itself and its two neighbours
        for d in (-1, 0, 1):
            assert np.any(b == (e << 23) + P.LOG_FOLD_MANTISSA + d), (e, d)
    scaled = (x[sub] * F(2.0 ** 64)).view(np.uint32) & 0x7fffff      # where the fold sits after the subnormal rescale
    assert np.any(scaled > P.LOG_FOLD_MANTISSA) and np.any(scaled <= P.LOG_FOLD_MANTISSA)
    assert np.any(np.abs(scaled.astype(np.int64) - P.LOG_FOLD_MANTISSA) <= 16)


# ---- the sc16 rules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [float(s) for s in P.SC16_SCALES])
def test_f2s_against_the_integer_rule(scale):
    vi, vq = P.f2_to_sc16(scale)
    for v in (vi, vq):
        want, clipped = P.sc16_rule(v, scale)
        assert np.array_equal(orc.probe_f2s(v, scale), want)
    want, clipped = P.sc16_rule(vi, scale)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (vi * F(scale)).astype(np.float64)
        fin = np.isfinite(p)
        tie = fin & (np.abs(p - np.floor(p) - 0.5) == 0) & (np.abs(p) < 40000)
    print("f2s at scale %g: n %d, %.2f %% saturate, %d ties" % (scale, vi.size, 100 * clipped.mean(), tie.sum()))
    assert clipped.mean() >= 0.01                           # at least 1 % of the points saturate
    assert np.any(want == 32767) and np.any(want == -32768)
    assert np.any(np.isnan(vi)) and np.any(np.isposinf(vi)) and np.any(np.isneginf(vi))
    assert want[np.isnan(vi)].tolist() == [0] and not clipped[np.isnan(vi)].any()
    if scale < 1e30:
        assert tie.sum() >= 500                             # rounding ties exist, and go to the even neighbour
        assert np.all(clipped[tie] | (want[tie].astype(np.int64) % 2 == 0))
        # the saturation edges: 32767.5 rounds to 32768 and clips, -32768.5 rounds to -32768 and does not
        if scale in (1.0, 32768.0):
            e = F([32767.5, -32768.5, 32767.0, -32768.0, 32768.5]) / F(scale)
            q, c = P.sc16_rule(e, scale)
            assert q.tolist() == [32767, -32768, 32767, -32768, 32767] and c.tolist() == [True, False, False, False, True]
            assert np.all(np.isin(e, vi))
            assert np.array_equal(orc.probe_f2s(e, scale), q)


@pytest.mark.parametrize("scale", [float(s) for s in P.SC16_IN_SCALES])
def test_sc16_to_f2_rule_is_one_rounded_multiply(scale):
    """the input conversion has no twin in the oracle: the chain tests feed the oracle (float)v * scale made by numpy, and that product is what the
    device is held to.  Here: numpy's float32 product is the correctly rounded one (against float64, which holds the exact product)"""
    w = P.sc16_words()
    lo = (w & 0xffff).astype(np.uint16).view(np.int16)
    hi = (w >> 16).astype(np.uint16).view(np.int16)
    assert set(lo[:65536].tolist()) == set(range(-32768, 32768)) and set(hi[65536:].tolist()) == set(range(-32768, 32768))
    s = F(scale)
    with np.errstate(under="ignore"):
        for v in (lo, hi):
            got = v.astype(F) * s
            exact = v.astype(np.float64) * np.float64(s)
            assert np.array_equal(got, exact.astype(F))
    if scale < 1e-40:
        tiny = np.abs(lo.astype(F) * s)
        assert np.any((tiny > 0) & (tiny < F(1.17549435e-38)))      # subnormal results


def test_sc16_store_set_fills_every_branch():
    d = P.sc16_store_divergent()
    vi, vq, valid, branch = d["vi"], d["vq"], d["valid"], d["branch"]
    sc = np.where(branch < 4, P.STORE_SCALES[np.minimum(branch, 3)], F(1.0))
    ci, cq = P.sc16_rule(vi, sc)[1], P.sc16_rule(vq, sc)[1]
    clips = ci | cq
    live = (branch < 4) & (valid != 0)
    for k in range(4):                                      # every branch holds clipped and unclipped valid lanes, in one and in both components
        m = live & (branch == k)
        assert np.any(m & clips) and np.any(m & ~clips) and np.any(m & ci & cq) and np.any(m & (ci ^ cq)), k
        assert np.any((branch == k) & (valid == 0) & clips), k      # and clipping lanes that must not count
    share = clips[branch < 4].mean()
    assert 0.05 < share < 0.2, share
    assert np.any(branch == P.STORE_EARLY_EXIT) and np.any(valid == 0)
    assert not clips[0, 0:64].any()                         # a wave with no clip at all
    w1 = slice(64, 128)
    assert clips[0, w1].any() and not (clips[0, w1] & (valid[0, w1] != 0)).any()      # a wave where only invalid lanes clip
    waves = branch[:, : d["n"] // 64 * 64].reshape(d["batch"], -1, 64)
    assert np.any([len(set(w[w < 4])) == 4 for row in waves for w in row])      # all four branches inside one wave
    assert d["n"] % 64 != 0 and d["n"] > 256 and d["batch"] > 1
