"""f2_to_sc8 and sc8_store of devmath.hpp alone (tests/host/sc8_out_probe.hip, built with the product's flags) against the rule in numpy:
r = rint(x * scale), the product one rounded float32 multiply, saturated to [-128, 127], NaN -> 0; a component counts as clipped when r > 127 or
r < -128.  Aimed products (ties, the edges of the range, non-finite values), a dense sweep, the clip sums under divergence, and the word-sharing
rule: a sample is one 2-byte store, whoever owns the other half of its 32-bit word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devmath_points as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "host", "libqrl_sc8_out_probe.so")
F = np.float32
_p, _sz, _u = C.c_void_p, C.c_size_t, C.c_uint32
SENTINEL = np.uint16(0x5A5A)
STORE_SCALES = F([127.0, 128.0, 118.0, 132.0])      # one per branch


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "sc8_out_probe"])
    lib = C.CDLL(PROBE)
    for name, args in {"f2_to_sc8": (_p, _p, _sz, C.c_float, _p, _p), "sc8_store_divergent": (_p, _p, _p, _p, _u, _u, _p, _p, _p),
                       "sc8_store_alternate": (_p, _p, _u, C.c_float, _p, _u, _u)}.items():
        f = getattr(lib, "qrl_probe_" + name)
        f.restype, f.argtypes = C.c_int, list(args)
    return lib


def _call(lib, name, *args):
    keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
    err = getattr(lib, "qrl_probe_" + name)(*[a.ctypes.data_as(_p) if isinstance(a, np.ndarray) else a for a in keep])
    assert err == 0, "%s: error %d" % (name, err)


def sc8_rule(v, scale):
    """(int8 value, clipped flag) per component"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = (np.ascontiguousarray(v, F) * np.asarray(scale, F)).astype(F)
    r = np.rint(p.astype(np.float64))                            # round half to even; exact in float64
    nan = np.isnan(r)
    clipped = ~nan & ((r > 127) | (r < -128))
    return np.where(nan, 0.0, np.clip(r, -128, 127)).astype(np.int64).astype(np.int8), clipped


def sc8_pack(i8, q8):
    return np.asarray(i8, np.int8).view(np.uint8).astype(np.uint16) | (np.asarray(q8, np.int8).view(np.uint8).astype(np.uint16) << np.uint16(8))


def _convert(probe, vi, vq, scale):
    w, nclip = np.zeros(vi.size, np.uint16), np.zeros(vi.size, np.uint32)
    _call(probe, "f2_to_sc8", vi, vq, vi.size, C.c_float(scale), w, nclip)
    return w, nclip


def _check(probe, v, scale):
    """every point as I beside a harmless Q, and as Q beside a harmless I"""
    v = np.ascontiguousarray(v, F)
    other = np.resize(F([0.25, -3.0, 100.0, -100.0]), v.size) / F(scale)
    for vi, vq in ((v, other), (other, v)):
        w, nclip = _convert(probe, vi, vq, scale)
        (ri, ci), (rq, cq) = sc8_rule(vi, scale), sc8_rule(vq, scale)
        bad = np.flatnonzero((w != sc8_pack(ri, rq)) | (nclip != ci.astype(np.uint32) + cq))
        assert bad.size == 0, "scale %r, first offenders (I, Q, word, nclip): %s" % (
            scale, [(float(vi[k]), float(vq[k]), hex(int(w[k])), int(nclip[k])) for k in bad[:8]])
    return sc8_rule(v, scale)


def test_aimed_products(probe):
    """scale 1: the product is the point itself"""
    ties = F([k + 0.5 for k in range(-130, 130)])                # even and odd k of both signs
    edges = F([127.49, -127.49, 127.5, -127.5, 128.49, -128.49, -128.5, 129.0, -129.0, 127.0, -128.0, 128.0])
    odd = F([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 1e30, -1e30, 3.4e38])
    r, c = _check(probe, np.concatenate([ties, edges, odd]), 1.0)
    # the rule itself at the points the contract names
    pts = np.concatenate([ties, edges, odd])
    table = dict(zip(pts.tolist(), zip(r.tolist(), c.tolist())))

    def at(x):
        return table[float(F(x))]
    assert at(0.5) == (0, False) and at(1.5) == (2, False) and at(2.5) == (2, False) and at(-0.5) == (0, False) and at(-1.5) == (-2, False)
    assert at(127.49) == (127, False) and at(127.5) == (127, True) and at(-127.5) == (-128, False)
    assert at(128.49) == (127, True) and at(-128.49) == (-128, False)
    assert at(-128.5) == (-128, False), "-128.5 rounds to -128: not a clip"
    assert at(129.0) == (127, True) and at(-129.0) == (-128, True)
    assert at(np.inf) == (127, True) and at(-np.inf) == (-128, True) and at(1e30) == (127, True)
    k = int(np.flatnonzero(np.isnan(pts))[0])
    assert (int(r[k]), bool(c[k])) == (0, False), "NaN gives 0 and is not counted"


@pytest.mark.parametrize("scale", [127.0, 1.0, -100.0, 0.3])
def test_dense_sweep(probe, scale):
    """products over [-130, 130] at a spacing of 1 / 256 (exact at scale 1), and a random set across it"""
    grid = np.arange(-130 * 256, 130 * 256 + 1, dtype=np.float64) / 256
    rng = np.random.default_rng(8)
    _check(probe, np.concatenate([(grid / scale).astype(F), (rng.uniform(-130, 130, 20000) / scale).astype(F)]), scale)


def test_both_components_clipped(probe):
    vi, vq = F([1.5, -1.5, 1.5, 0.5, np.inf]), F([-1.7, 1.7, 0.5, -1.7, -np.inf])
    w, nclip = _convert(probe, vi, vq, 127.0)
    assert nclip.tolist() == [2, 2, 1, 1, 2]
    assert np.array_equal(w, sc8_pack(sc8_rule(vi, 127.0)[0], sc8_rule(vq, 127.0)[0]))


def test_sc8_store_divergent(probe):
    """lanes that left early, up to four branches of one wave that all store, waves in which nothing (stored) clips, samples clipped twice"""
    d = P.sc16_store_divergent()
    vi, vq, valid, branch, n, batch = d["vi"], d["vq"], d["valid"], d["branch"], d["n"], d["batch"]
    calls = branch < 4                                           # lanes that reach a sc8_store at all
    live = calls & (valid != 0)
    sc = STORE_SCALES[np.minimum(branch, 3)]
    (ri, ci), (rq, cq) = sc8_rule(vi, sc), sc8_rule(vq, sc)
    ncl = np.where(live, ci.astype(np.int64) + cq, 0)
    # what the data must hold for the test to mean something
    assert (~calls).any() and (ncl == 2).any() and (ncl == 1).any()
    assert ncl[0, 0:64].sum() == 0 and live[0, 0:64].any(), "row 0, wave 0: stores, no clip, no atomic"
    assert ncl[0, 64:128].sum() == 0 and (ci | cq)[0, 64:128].any(), "row 0, wave 1: only lanes that do not store would clip"
    assert np.unique(branch[0, 70:90]).tolist() == [0, 1, 2, 3], "four branches of one wave store"
    assert not live[1, 192:256].any(), "row 1, wave 3: no lane stores"
    out = np.full((batch, n), SENTINEL, np.uint16)
    clip = np.full(batch, 7, np.uint32)                          # the counters do not start at zero: the kernel adds
    _call(probe, "sc8_store_divergent", vi, vq, valid, branch, n, batch, STORE_SCALES, out, clip)
    assert np.array_equal(out, np.where(live, sc8_pack(ri, rq), SENTINEL))
    assert clip.tolist() == (7 + ncl.sum(axis=1)).tolist()


@pytest.mark.parametrize("first", [8, 9], ids=["row-at-0-mod-4", "row-at-2-mod-4"])
@pytest.mark.parametrize("n", [1, 2, 129, 300])
def test_two_waves_share_every_word(probe, first, n):
    """two waves write the even and the odd samples of one row: every sample comes out as its owner wrote it, the sentinel stays on both sides"""
    rng = np.random.default_rng(100 * first + n)
    vi, vq = rng.uniform(-1.2, 1.2, n).astype(F), rng.uniform(-1.2, 1.2, n).astype(F)
    total = first + n + 9
    buf = np.full(total, SENTINEL, np.uint16)
    _call(probe, "sc8_store_alternate", vi, vq, n, C.c_float(127.0), buf, total, first)
    want = sc8_pack(sc8_rule(vi, 127.0)[0], sc8_rule(vq, 127.0)[0])
    assert not (want == SENTINEL).all()
    assert np.array_equal(buf[first:first + n], want)
    assert (buf[:first] == SENTINEL).all() and (buf[first + n:] == SENTINEL).all()
