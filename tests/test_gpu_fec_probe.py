"""The K=7 Viterbi decoder + descrambler (k_fec) alone against the oracle, bit for bit, on the soft-symbol sets and ragged call schedules of
tests/fec_points.py.  The device side is tests/host/fec_probe.hip: one call of the product's own qrl::launch_fec per entry, nothing restated.  This
file plays the handle: it keeps the 1024-byte soft ring and the FecState array between calls and writes a call's new symbols at index & mask, as
the symbol synchroniser would.  The reference is orc.descramble(orc.cc_decode_k7(.)) of the stream (branch A) and of [0] + stream (branch B, fec_tail
of oracle/orc_chains.c); tests/test_fec_conditions.py asserts on the CPU what these sets and schedules reach inside the decoder."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import fec_points as P
import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "host", "libqrl_fec_probe.so")
_p = C.c_void_p
GUARD = 0xA5
COUNT_GUARD = 0xDEAD0000
STATE = np.dtype([("consumed", np.uint64), ("start_state", np.uint32), ("last_bits", np.uint32)])   # FecState of engine.hpp
UNUSED_STATE = (0x1234567, 0x55, 0xAA)     # in the second slot of a stream with one branch: never read, never written
CAP = 4 * P.BLOCK_BITS                    # no call of a schedule completes more than four blocks


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "fec_probe"])
    lib = C.CDLL(PROBE)
    lib.qrl_probe_fec.restype = C.c_int
    lib.qrl_probe_fec.argtypes = [_p, C.c_uint32, _p, C.c_uint32, C.c_int, C.c_int, _p, C.c_size_t, _p, _p, _p]
    return lib


@functools.lru_cache(maxsize=None)
def reference(name, branch):
    """(decoded bits, descrambled bits) of the oracle for one unit's whole stream"""
    dec = orc.cc_decode_k7(P.branch_input(name, branch))
    out = orc.descramble(dec)
    assert dec.size == P.NBLOCKS * P.BLOCK_BITS
    return dec, out


def reference_state(name, branch, nblk):
    """FecState after nblk blocks, from the oracle's decoded bits d: last_bits bit t = d[-1 - t] (the descrambler's register, seed 0x7F in front of
    the stream), start_state = the trellis state six steps before the end of the block = the last six decoded bits, newest in bit 0"""
    if nblk == 0:
        return (0, 0, 0xFE)
    d = reference(name, branch)[0][:nblk * P.BLOCK_BITS]
    last = sum(int(d[-1 - t]) << t for t in range(8))
    return (P.BLOCK_SYMS * nblk, last & 63, last)


class Handle:
    """ring, state and the running symbol counts of `names`' streams under one configuration"""

    def __init__(self, lib, config, names):
        self.lib, self.names = lib, names
        self.branches, self.mul = P.CONFIGS[config]
        self.batch = len(names)
        # 255 everywhere, where a handle's ring starts zeroed: the zero symbol in front of branch B's stream has to be the decoder's own doing
        # (engine.hpp: "an item in front of the stream start is zero"), not what happens to lie at ring index -1 & mask
        self.ring = np.full((self.batch, P.RING), 255, np.uint8)
        self.avail = np.zeros(self.batch, np.uint64)
        self.st = np.zeros((self.batch, 2), STATE)
        for b in range(self.batch):
            self.st[b, 0] = (0, 0, 0xFE)
            self.st[b, 1] = (0, 0, 0xFE) if self.branches == 2 else UNUSED_STATE
        self.done = np.zeros((self.batch, self.branches), np.int64)

    def call(self, deliveries, cap=CAP, want_a=True, want_b=True):
        """deliver deliveries[b] items to stream b, decode; returns (bits_a, bits_b, counts, blocks decoded before, after) -- buffers guard-filled"""
        for b, n in enumerate(deliveries):
            i0, i1 = int(self.avail[b]) * self.mul, (int(self.avail[b]) + int(n)) * self.mul
            assert i1 <= P.STREAM_SYMS
            idx = np.arange(i0, i1)
            self.ring[b, idx & P.MASK] = P.soft(self.names[b])[idx]
            self.avail[b] += np.uint64(n)
        bits = [np.full((self.batch, cap), GUARD, np.uint8) if want else None for want in (want_a, want_b)]
        counts = np.full(self.batch * 4, COUNT_GUARD, np.uint32) + np.arange(self.batch * 4, dtype=np.uint32)
        err = self.lib.qrl_probe_fec(self.ring.ctypes.data_as(_p), P.MASK, self.avail.ctypes.data_as(_p), self.mul, self.branches, self.batch,
                                     self.st.ctypes.data_as(_p), cap, *[x.ctypes.data_as(_p) if x is not None else None for x in bits],
                                     counts.ctypes.data_as(_p))
        assert err == 0, "HIP error %d" % err
        before = self.done.copy()
        for b in range(self.batch):
            for r in range(self.branches):
                self.done[b, r] = P.blocks_ready(int(self.avail[b]) * self.mul + r)
        return bits[0], bits[1], counts, before, self.done.copy()

    def check(self, what, bits_a, bits_b, counts, before, after, cap=CAP):
        """bits and counts of one call against the oracle: the blocks that became decodable in it, cut at the cap; nothing else touched"""
        want_counts = np.full(self.batch * 4, COUNT_GUARD, np.uint32) + np.arange(self.batch * 4, dtype=np.uint32)
        for b, name in enumerate(self.names):
            for r in range(self.branches):
                lo, hi = P.BLOCK_BITS * before[b, r], P.BLOCK_BITS * after[b, r]
                n = min(hi - lo, cap)
                want_counts[4 * b + 2 + r] = n
                buf = bits_b if r else bits_a
                if buf is None:
                    continue
                want = np.full(cap, GUARD, np.uint8)
                want[:n] = reference(name, r)[1][lo:lo + n]
                bad = np.flatnonzero(buf[b] != want)
                assert bad.size == 0, "%s: stream %d (%s) branch %s, blocks %d..%d: %d bytes differ, first at %d (device %d, oracle %d)" % (
                    what, b, name, "AB"[r], before[b, r], after[b, r], bad.size, bad[0], buf[b][bad[0]], want[bad[0]])
            if self.branches == 1 and bits_b is not None:
                assert (bits_b[b] == GUARD).all(), "%s: stream %d: branch B written with one branch" % (what, b)
        assert np.array_equal(counts, want_counts), "%s: counts %s, oracle %s" % (what, counts, want_counts)

    def check_state(self, what):
        for b, name in enumerate(self.names):
            for r in range(2):
                want = reference_state(name, r, self.done[b, r]) if r < self.branches else UNUSED_STATE
                assert tuple(int(v) for v in self.st[b, r]) == want, "%s: stream %d (%s) state %d: device %s, oracle %s" % (
                    what, b, name, r, self.st[b, r], want)


@pytest.mark.parametrize("batch", P.BATCHES)
@pytest.mark.parametrize("config", range(len(P.CONFIGS)), ids=["b2m1", "b1m2", "b2m2"])
def test_every_call_of_a_ragged_schedule(probe, config, batch):
    """bits, counts and the state after every call, every stream of the batch another set"""
    h = Handle(probe, config, P.BATCH_SETS[batch])
    for k, d in enumerate(P.schedule(config, batch)):
        what = "call %d (+%s items)" % (k, d.tolist())
        res = h.call(d)
        h.check(what, *res)
        h.check_state(what)
    assert (h.done == P.NBLOCKS).all()


def _two_blocks(mul):
    """a call that completes two blocks of stream 0 on either branch, and none of the others"""
    return (P.BLOCK_SYMS + P.NEED_SYMS + 2) // mul


@pytest.mark.parametrize("cap", [0, 79, 80, 81, 150])
@pytest.mark.parametrize("config", range(len(P.CONFIGS)), ids=["b2m1", "b1m2", "b2m2"])
def test_bits_cap_below_what_a_call_produces(probe, config, cap):
    """a call of two blocks (160 bits) into buffers of `cap` bytes a stream: the prefix is written, nothing at or beyond the cap (the rows of the two
    idle streams behind it stay as they were filled), counts says what was written, the state moves by the two blocks all the same"""
    mul = P.CONFIGS[config][1]
    h = Handle(probe, config, ("weak_code", "coded_noise", "uniform"))
    n = _two_blocks(mul)
    res = h.call([n, 100 // mul, 2], cap=cap)
    assert (res[4][0] == 2).all() and (res[4][1:] == 0).all()
    h.check("capped call", *res, cap=cap)
    h.check_state("capped call")
    res = h.call([P.BLOCK_SYMS // mul, 0, 0])
    assert (res[4][0] == 3).all()
    h.check("call after the capped one", *res)
    h.check_state("call after the capped one")


@pytest.mark.parametrize("want_a,want_b", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("config", range(len(P.CONFIGS)), ids=["b2m1", "b1m2", "b2m2"])
def test_null_bit_buffers(probe, config, want_a, want_b):
    """bits_a and / or bits_b null: counts and state advance as if they were there, and the next call's bits are right"""
    mul = P.CONFIGS[config][1]
    h = Handle(probe, config, ("weak_code", "bursts"))
    res = h.call([_two_blocks(mul), P.NEED_SYMS // mul], want_a=want_a, want_b=want_b)
    assert (res[4][0] == 2).all() and (res[4][1] == 1).all()
    h.check("call with null buffers", *res)
    h.check_state("call with null buffers")
    res = h.call([P.BLOCK_SYMS // mul, (2 * P.BLOCK_SYMS) // mul])
    assert (res[4][0] == 3).all() and (res[4][1] == 3).all()
    h.check("call after it", *res)
    h.check_state("call after it")
