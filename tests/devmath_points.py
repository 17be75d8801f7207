"""Input sets of the math-primitive tests (tests/test_gpu_devmath.py: device == oracle bit for bit; tests/test_devmath_definition.py:
oracle against float64 definitions, and the conditions a set has to meet).  Seeded; every set joins a dense sweep with points aimed at
the edges of the function (quadrant changes, table breakpoints, thresholds, ties, saturation, specials); at most 2^24 points each.
Each function returns the same arrays on every call of a process (cached) and nobody writes into them."""
import functools

import numpy as np

F = np.float32
U = np.uint32
SIGN = U(0x80000000)
INF = F(np.inf)
NAN = F(np.nan)
MAX_POINTS = 1 << 24


def f32(bits):
    return np.asarray(bits, U).view(F)


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def ulps(x, span):
    """every float within +-span units in the last place of each x (x finite; steps walk through 0 into the other sign)"""
    b = bits(np.atleast_1d(x)).astype(np.int64)
    key = np.where(b & 0x80000000, -(b & 0x7fffffff), b)            # monotone integer line of the floats
    key = (key[:, None] + np.arange(-span, span + 1)[None, :]).ravel()
    out = np.where(key < 0, (-key) | 0x80000000, key).astype(U)
    return out.view(F)


def both_signs(x):
    x = np.ascontiguousarray(x, F)
    return np.concatenate([x, -x])


def _done(a):
    a = np.ascontiguousarray(a)
    assert a.shape[-1] <= MAX_POINTS
    a.setflags(write=False)
    return a


cache = functools.lru_cache(maxsize=None)

SUBNORMALS = f32([1, 2, 0x00400000, 0x007fffff])
PI = np.pi


# ---- sincos_rad -----------------------------------------------------------------------------------------------------------------
SINCOS_DENSE = 16.0      # the stride sweep covers [-16, 16]
SINCOS_FAR = 1.0e5       # the log-spaced sweep ends here: 63 662 quarter turns, far below 2^31


@cache
def sincos_rad():
    dense = f32(np.arange(0, 0x41800000 + 1, 1021, dtype=np.int64))                           # every 1021st float of [0, 16]
    quarter = ulps(F(np.arange(1, 129) * (PI / 4)), 4)                                         # quadrant changes (odd k) and rintf ties
    far = np.geomspace(SINCOS_DENSE, SINCOS_FAR, 200000).astype(F)
    far_q = ulps(F(np.rint(np.geomspace(129, 2 * SINCOS_FAR / PI - 2, 4000)) * (PI / 4)), 2)   # and quarter-turn multiples out there
    x = both_signs(np.concatenate([dense, quarter, far, far_q, SUBNORMALS, F([0.0, SINCOS_DENSE, SINCOS_FAR])]))
    return _done(x)


# ---- sincos_turn ----------------------------------------------------------------------------------------------------------------
@cache
def sincos_turn():
    rng = np.random.default_rng(0x7012)
    top = np.arange(0, 1 << 32, 2039, dtype=np.uint64)
    low = rng.integers(0, 1 << 32, top.size, dtype=np.uint64)
    edge = ((np.arange(8, dtype=np.int64) << 29)[:, None] + np.arange(-8, 9)[None, :]).ravel() & 0xffffffff
    edge = edge.astype(np.uint64)
    a = np.concatenate([(top << np.uint64(32)) | low, edge << np.uint64(32), (edge << np.uint64(32)) | np.uint64(0xffffffff)])
    return _done(a)


# ---- fast_atan2 -----------------------------------------------------------------------------------------------------------------
ATAN_THRESHOLD_BITS = 0x3B808082          # the first float >= 0.003921569
# atan2() = (y, x, n_aimed): the first n_aimed points are the threshold and breakpoint ones


def _atan_pairs(z, big):
    """all sign pairs and both branches of (small, big) with small / big == z exactly (big a power of two)"""
    z = np.ascontiguousarray(z, F)
    small = z * F(big)
    bigv = np.full(z.size, big, F)
    ys, xs = [], []
    for sy in (1, -1):
        for sx in (1, -1):
            ys += [F(sy) * small, F(sy) * bigv]
            xs += [F(sx) * bigv, F(sx) * small]
    return np.concatenate(ys), np.concatenate(xs)


@cache
def atan2():
    rng = np.random.default_rng(0xA7A2)
    thr = f32(np.arange(0x3B808070, 0x3B808090 + 1))
    brk = ulps(F(np.arange(1, 256) / 255.0), 4)
    brk = brk[brk <= 1.0]
    ya, xa = zip(*[_atan_pairs(np.concatenate([thr, brk]), big) for big in (1.0, 0.125, 4096.0)])
    ya, xa = np.concatenate(ya), np.concatenate(xa)
    n_aimed = ya.size
    # dense: ratios swept through [0, 1] by bit pattern, under a random power-of-two magnitude, all signs and both branches
    z = f32(np.arange(0x33000000, 0x3F800000 + 1, 4093, dtype=np.int64))
    yd, xd = _atan_pairs(z, 1.0)
    mag = np.exp2(rng.integers(-20, 21, yd.size)).astype(F)
    yd, xd = yd * mag, xd * mag
    # random pairs whose quotient is rounded
    n = 1 << 20
    yr = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 13, n))).astype(F)
    xr = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 13, n))).astype(F)
    # |x| == |y|
    e = np.abs(rng.standard_normal(64)).astype(F)
    ye = np.concatenate([e, e, -e, -e])
    xe = np.concatenate([e, -e, e, -e])
    # signed zeros, one argument zero or infinite, subnormal over subnormal, very large over very small
    s = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0)]
    for v in (1.0, -1.0, 3.0e38, -1.0e-40):
        s += [(0.0, v), (-0.0, v), (v, 0.0), (v, -0.0), (np.inf, v), (-np.inf, v), (v, np.inf), (v, -np.inf)]
    sub = [float(v) for v in SUBNORMALS] + [-float(SUBNORMALS[1])]
    s += [(a, b) for a in sub for b in sub]
    s += [(a, b) for a in (3.0e38, -3.0e38, 1.0e30) for b in (1.0e-38, -1.0e-38, 1.0e-45)]
    s += [(b, a) for a in (3.0e38, -3.0e38, 1.0e30) for b in (1.0e-38, -1.0e-38, 1.0e-45)]
    ysp, xsp = np.array(s, F).T
    y = np.concatenate([ya, yd, yr, ye, ysp])
    x = np.concatenate([xa, xd, xr, xe, xsp])
    assert not np.any(np.isnan(y) | np.isnan(x) | (np.isinf(y) & np.isinf(x)))
    return _done(y), _done(x), n_aimed


@cache
def atan2_undefined_on_host():
    """both arguments infinite, or a NaN: (int)NaN is undefined on the host, so these stay out of the comparison"""
    v = [np.inf, -np.inf, np.nan, 0.0, -1.0, 2.5]
    s = [(a, b) for a in v for b in v if (np.isinf(a) and np.isinf(b)) or np.isnan(a) or np.isnan(b)]
    y, x = np.array(s, F).T
    return _done(y), _done(x)


# ---- tanh_lut -------------------------------------------------------------------------------------------------------------------
@cache
def tanh():
    steps = ulps(F((np.arange(-8, 265) - 128) / 64.0), 4)                        # 128 + 64 x an integer, index -8 .. 264
    dense = both_signs(f32(np.arange(0, 0x40200000 + 1, 509, dtype=np.int64)))   # every 509th float of [-2.5, 2.5]
    edge = both_signs(np.concatenate([ulps(F([2.0]), 8), F([np.inf, 1.0e30, 3.0, 0.0]), SUBNORMALS]))
    return _done(np.concatenate([steps, dense, edge]))


# ---- clip / ted_error -----------------------------------------------------------------------------------------------------------
CLIP_LIMITS = F([1.0, 0.5, 3.7, 1.0e-3, 0.011, 1.0e30])


def _around_limit(lim):
    lim = F(lim)
    near = np.concatenate([ulps(F([lim, lim / F(2), lim * F(2), lim * F(3)]), 4), F([0.0, lim * F(1.0e-8), lim * F(1.0e8)])])
    sweep = (np.linspace(-3, 3, 4001) * float(lim)).astype(F)
    return np.concatenate([both_signs(near), sweep, both_signs(SUBNORMALS), F([np.inf, -np.inf, 3.0e38, -3.0e38, 1.0e20])])


@cache
def clip():
    xs = [_around_limit(l) for l in CLIP_LIMITS]
    x = np.concatenate(xs)
    lim = np.concatenate([np.full(v.size, l, F) for v, l in zip(xs, CLIP_LIMITS)])
    return _done(x), _done(lim)


@cache
def ted_u():
    rng = np.random.default_rng(0x7ED)
    u = np.concatenate([_around_limit(1.0), _around_limit(2.0), (rng.standard_normal(1 << 16) * 1.5).astype(F)])
    return _done(u)


# ---- phase_wrap -----------------------------------------------------------------------------------------------------------------
WAVE = 64


@cache
def phase_wrap():
    """waves of 64 consecutive values; the layout decides which lanes of a wave are out of [-2 pi, 2 pi]"""
    rng = np.random.default_rng(0xFA5E)
    two_pi = float(F(2 * PI))

    def inside(n):
        return rng.uniform(-two_pi, two_pi, n).astype(F)

    def outside(n, turns):
        """out of range by `turns` loop turns (an array or a number), either sign"""
        mag = two_pi * np.asarray(turns, np.float64) + rng.uniform(0.05, two_pi - 0.05, n)
        return (mag * rng.choice([-1.0, 1.0], n)).astype(F)

    waves = []
    waves += list(rng.uniform(-8 * PI, 8 * PI, (2048, WAVE)).astype(F))                      # anything in [-8 pi, 8 pi]
    waves += list(inside(256 * WAVE).reshape(256, WAVE))                                     # no lane out of range: the uniform early exit
    for lane in (0, 31, 32, 63):                                                              # exactly one lane out of range
        for turns in (1, 2, 3):
            for _ in range(8):
                w = inside(WAVE)
                w[lane] = outside(1, turns)[0]
                waves.append(w)
    for turns in (1, 2, 3):                                                                   # all lanes out of range
        waves += [outside(WAVE, turns) for _ in range(8)]
    for _ in range(32):                                                                       # a different number of turns per lane, 0 included
        t = rng.integers(0, 4, WAVE)
        waves.append(np.where(t == 0, inside(WAVE), outside(WAVE, np.maximum(t, 1) - 0.0)).astype(F))
    edges = both_signs(np.concatenate([ulps(F([2 * PI, 4 * PI, 6 * PI, 8 * PI]), 4), F([0.0])]))   # either side of the limits
    for k in range(0, edges.size, 4):                                                         # four edge values in an in-range wave ...
        w = inside(WAVE)
        w[rng.choice(WAVE, 4, replace=False)] = np.resize(edges[k:k + 4], 4)
        waves.append(w)
    waves.append(np.resize(edges, WAVE))                                                      # ... and waves of nothing else
    waves.append(np.resize(edges[::-1], WAVE))
    x = np.concatenate(waves)
    tail = inside(37)                                                                         # a ragged last wave, one lane out of range
    tail[5] = F(-7.5)
    return _done(np.concatenate([x, tail]))


# ---- det_log2 / det_log10 -------------------------------------------------------------------------------------------------------
LOG_FOLD_MANTISSA = 0x3504F3      # 1.41421354f = 0x3FB504F3
LOG_STRIDE = 1021


@cache
def det_log():
    dense = f32(np.arange(1, 0x7f800000, LOG_STRIDE, dtype=np.int64))                          # positive patterns, subnormals included
    d = np.arange(-8, 9)
    fold = f32(((np.arange(1, 255, dtype=np.int64) << 23)[:, None] + LOG_FOLD_MANTISSA + d[None, :]).ravel())
    sub_fold = f32((((0x800000 | LOG_FOLD_MANTISSA) >> np.arange(1, 20, dtype=np.int64))[:, None] + d[None, :]).ravel())   # the fold after the 2^64 rescale
    near_one = ulps(F([1.0, 2.0, 0.5]), 16)
    edge = f32([1, 2, 0x007fffff, 0x00800000, 0x00800001, 0x7f7fffff, 0x7f7ffffe])
    special = F([0.0, -0.0, -1.0, -1.0e-40, -3.0e38, np.inf, -np.inf, np.nan])
    return _done(np.concatenate([dense, fold, sub_fold, near_one, edge, special]))


# ---- f2_to_sc16 -----------------------------------------------------------------------------------------------------------------
SC16_SCALES = F([32767.0, 32768.0, 1.0, 3.0e38])      # the last one overflows: any |v| > 1.14 becomes inf


@cache
def f2_to_sc16(scale):
    """(vi, vq) for one scale: products on and around rounding ties, the saturation edges, specials, a random body of which some clip"""
    scale = F(scale)
    rng = np.random.default_rng(0x5C16)
    k = np.unique(np.concatenate([np.arange(-32772, 32773, 97), np.arange(-32772, -32760), np.arange(32760, 32773), np.arange(-6, 7)]))
    with np.errstate(over="ignore", under="ignore"):
        ties = ulps((k + 0.5).astype(F) / scale, 1)                                     # exact for the power-of-two scales, next to the tie for 32767
        edges = ulps(F([32767.5, -32767.5, 32768.5, -32768.5, 32767.0, -32768.0]) / scale, 2)
        body = (rng.standard_normal(1 << 18) * 0.55).astype(F) * (F(32768.0) / scale)   # about 7 % of the components past full scale
    special = F([np.inf, -np.inf, np.nan, -0.0, 0.0, 3.0e38, -3.0e38, 1.0e-45, -1.0e-45])
    vi = np.concatenate([ties, edges, special, body])
    vq = vi[rng.permutation(vi.size)]
    return _done(vi), _done(vq)


# ---- sc16_to_f2 -----------------------------------------------------------------------------------------------------------------
SC16_IN_SCALES = F([1.0 / 32768.0, 1.0, 2.0e-42, 3.3e-5])      # 2e-42 is subnormal itself and gives subnormal samples


@cache
def sc16_words():
    """every int16 value in the low half and in the high half, the other half shuffled"""
    rng = np.random.default_rng(0x16)
    v = np.arange(1 << 16, dtype=U)
    w = np.concatenate([v | (rng.permutation(v) << U(16)), rng.permutation(v) | (v << U(16))])
    return _done(w)


# ---- sc16_store under divergence ------------------------------------------------------------------------------------------------
STORE_SENTINEL = U(0xDEADBEEF)
STORE_CLIP_START = U(7)              # the counters do not start at zero: the kernel adds
STORE_SCALES = F([32767.0, 32768.0, 30000.0, 34000.0])      # one per branch
STORE_EARLY_EXIT = np.uint8(255)


@cache
def sc16_store_divergent():
    """dict of vi, vq [batch][n] float32, valid, branch [batch][n] uint8, n, batch.  n = 1000: four workgroups a row, the last wave ragged"""
    rng = np.random.default_rng(0xD1CE)
    batch, n = 3, 1000
    vi = (rng.standard_normal((batch, n)) * 0.55).astype(F)      # about a tenth of the lanes clip in one or both components
    vq = (rng.standard_normal((batch, n)) * 0.55).astype(F)
    both = rng.random((batch, n)) < 0.02
    vi[both] = F(1.5); vq[both] = F(-1.7)
    valid = (rng.random((batch, n)) < 0.8).astype(np.uint8)
    branch = rng.integers(0, 4, (batch, n)).astype(np.uint8)
    branch[rng.random((batch, n)) < 0.1] = STORE_EARLY_EXIT
    vi[0, 0:64] *= F(0.1); vq[0, 0:64] *= F(0.1)                 # row 0, wave 0: no lane clips
    w1 = slice(64, 128)                                          # row 0, wave 1: only invalid lanes clip
    vi[0, 70:90] = F(2.0)
    clips = (np.abs(vi[0, w1]) > 0.9) | (np.abs(vq[0, w1]) > 0.9)
    valid[0, w1] = np.where(clips, 0, 1)
    branch[0, 70:90] = np.arange(20) % 4
    branch[1, 128:192] = 2                                       # row 1, wave 2: one branch takes the whole wave
    valid[1, 192:256] = 0                                        # row 1, wave 3: no lane valid
    d = dict(vi=vi, vq=vq, valid=valid, branch=branch)
    for a in d.values():
        a.setflags(write=False)
    d.update(n=n, batch=batch)
    return d


def sc16_rule(v, scale):
    """the sc16 rule restated on integers: (int16 value, clipped flag) of r = rint(v * scale), the product one rounded float32 multiply.
    NaN gives 0 and does not count as clipped; +-inf saturates and counts."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = (np.ascontiguousarray(v, F) * np.asarray(scale, F)).astype(F)
    r = np.rint(p.astype(np.float64))                            # round half to even; exact in float64
    nan = np.isnan(r)
    clipped = ~nan & ((r > 32767) | (r < -32768))
    q = np.where(nan, 0.0, np.clip(r, -32768, 32767)).astype(np.int64)
    return q.astype(np.int16), clipped


def sc16_pack(i16, q16):
    return (np.asarray(i16, np.int16).view(np.uint16).astype(U)) | (np.asarray(q16, np.int16).view(np.uint16).astype(U) << U(16))
