"""Soft-symbol sets, call schedules and an instrumented restatement for the K=7 Viterbi decoder + descrambler run alone
(tests/test_gpu_fec_probe.py on the device, tests/test_fec_conditions.py on the CPU).

Three things live here, none of which knows the device:

* FAMILIES: seeded generators of u8 soft symbols, each aimed at a corner of the decoder's arithmetic (saturating sums, ties,
  the renormalisation threshold, tied end states, block chaining).
* decode(): VOLK's spiral K=7 r=1/2 kernel behind cc_decoder(80, CC_STREAMING), restated once more and INSTRUMENTED: beside the
  bits it reports, per block and step, what the arithmetic went through.  It is separate from appendix_a.cc_decode_k7 (which stays as it is)
  and from the oracle; tests/test_fec_conditions.py holds the oracle to it bit for bit on every set.
* schedule() / simulate(): how a stream is cut into calls, and what a call of the decoder then has to do: which 80-bit blocks of which unit
  become decodable, and which blocks of the two units of a wave meet in one pass of the kernel's block loop.

A UNIT is one trellis: (stream, alignment branch).  Branch A decodes the stream, branch B the stream behind one zero symbol (blocks::delay(1)).
With two branches unit 2b + r is branch r of stream b, with one branch unit b is stream b; units 2w and 2w + 1 share wave w, in the low and the
high half of its registers."""
import functools

import numpy as np

BLOCK_BITS = 80
BLOCK_SYMS = 160          # soft symbols a block consumes
NEED_SYMS = 172           # ... and needs in front of it: 6 trellis steps of look-ahead
STEPS = 86
RING = 1024               # the smallest soft ring a handle makes (engine.cpp: pow2_at_least(symbols of the calls in flight + 512))
MASK = RING - 1
# What a handle with that ring may hold unread (written, not consumed by the decoder): the symbols of the calls in flight, RING - 512, on top
# of what the last decoder call left, which is less than one block's need.  Every schedule below stays inside it.
MAX_CALL_SYMS = RING - 512
MAX_UNREAD = NEED_SYMS - 1 + MAX_CALL_SYMS
NBLOCKS = 40
STREAM_SYMS = BLOCK_SYMS * NBLOCKS + 12 + 38      # 6450: 40 blocks on either branch and a ragged, even remainder

# (branches, avail_mul) of the product: 2FSK / GMSK / BPSK / DSSS, QPSK, 4FSK
CONFIGS = ((2, 1), (1, 2), (2, 2))
BATCHES = (1, 2, 3, 5)


def _parity(v):
    return bin(v).count("1") & 1


# ---------------------------------------------------------------- the sets
def _encode(bits):
    """cc_encoder K=7, polynomials 109 / 79, streaming from state 0: two coded bits per bit"""
    st, out = 0, np.empty(2 * len(bits), np.uint8)
    for i, b in enumerate(bits):
        st = ((st << 1) | int(b)) & 0x7F
        out[2 * i], out[2 * i + 1] = _parity(st & 109), _parity(st & 79)
    return out


def _coded(rng, n):
    return _encode(rng.integers(0, 2, (n + 1) // 2))[:n].astype(np.int64)


def _coded_hard(rng, n):
    return _coded(rng, n) * 255


def _coded_noise(rng, n):
    return np.clip(np.rint(128 + 100 * (2 * _coded(rng, n) - 1) + 40 * rng.standard_normal(n)), 0, 255)


def _uniform(rng, n):
    return rng.integers(0, 256, n)


def _random_hard(rng, n):
    return rng.integers(0, 2, n) * 255


def _const(v):
    return lambda rng, n: np.full(n, v)


def _alternating(rng, n):
    return 127 + (np.arange(n) & 1)


def _near_centre(rng, n):
    return rng.choice(np.array([123, 124, 127, 128, 131, 132]), n)


def _bursts(rng, n):
    x = _coded_hard(rng, n)
    for start in range(100, n - 40, 331):          # off the block length and the call cuts
        x[start:start + 40] = rng.integers(0, 2, 40) * 255
    return x


def _weak_code(rng, n):
    """clean code zero, one or two metric steps (of 4) off the centre: decisions that hang on a tie or on a difference of one"""
    return 128 + (2 * _coded(rng, n) - 1) * 4 * rng.integers(0, 3, n)


FAMILIES = {
    "coded_hard": _coded_hard, "coded_noise": _coded_noise, "uniform": _uniform, "random_hard": _random_hard, "const128": _const(128),
    "const127": _const(127), "alternating": _alternating, "near_centre": _near_centre, "const0": _const(0), "const255": _const(255),
    "bursts": _bursts, "weak_code": _weak_code,
}
# the streams of a batch, in order: every stream of a batch carries another set, and the four batches between them carry every set
BATCH_SETS = {
    1: ("coded_noise",),
    2: ("uniform", "random_hard"),
    3: ("coded_hard", "const128", "near_centre"),
    5: ("alternating", "const127", "const0", "const255", "bursts"),
}
# a twelfth set, beside the eleven of the batches: the first stream of the cap and null-buffer cases of the device test
EXTRA_SETS = ("weak_code",)


# Events alone do not make a wrong decoder show: a renormalisation one step late, a sum left above 255 or a minimum subtracted early move all the
# metrics of a trellis alike, and the decoded bits change only where a saturated sum later decides a survivor on the path that wins.  About one
# random 40-block stream in six has such a place.  These seeds were picked, on the restatement below with its wrong-decoder arguments and never on
# the device, as streams that have them: tests/test_fec_conditions.py asserts what each tells apart.
SEED_SALT = {"uniform": 25, "coded_noise": 19, "random_hard": 23}


def _rng(name):
    return np.random.default_rng([0xFEC, sorted(FAMILIES).index(name)] + ([SEED_SALT[name]] if name in SEED_SALT else []))


@functools.lru_cache(maxsize=None)
def soft(name):
    """the set's STREAM_SYMS soft symbols (u8, read-only)"""
    rng = _rng(name)
    x = np.asarray(FAMILIES[name](rng, STREAM_SYMS)).astype(np.uint8)
    assert x.size == STREAM_SYMS
    x.setflags(write=False)
    return x


def branch_input(name, branch):
    """what branch `branch` of a stream decodes: the stream, or the stream behind one zero symbol"""
    x = soft(name)
    return x if branch == 0 else np.concatenate([np.zeros(1, np.uint8), x])


# ---------------------------------------------------------------- the instrumented restatement
_B0 = np.array([255 if _parity((2 * i) & 109) else 0 for i in range(32)], np.int64)
_B1 = np.array([255 if _parity((2 * i) & 79) else 0 for i in range(32)], np.int64)
# The kernel keeps state -> lane rotating: after step 85 bit j of a state sits in lane bit (85 - j) mod 6, and its search for the first minimum in
# STATE order runs over lanes.  LANE_AT_END[state] is that lane: a tied end state tells the two orders apart only if they disagree on it.
LANE_AT_END = np.array([sum(((s >> j) & 1) << ((85 - j) % 6) for j in range(6)) for s in range(64)])


class Decoded:
    """bits: decoded bits before the descrambler; out: behind it.  Per block and step ([nblk, 86]): one_over / both_over = output states whose
    two candidate sums have one / both above 255, sat_ties / ties = output states whose two CLAMPED sums are equal at 255 / below, y0 = metric[0]
    after the step and before a renormalisation, renorm = it renormalised, rmin = the minimum it subtracted, rspread = maximum - minimum there.
    Per block: start = the chained start state, end = the end state that won, end_tied = how many states hold the minimal end metric,
    end_first_lane = the one of them that sits in the lowest lane at step 85."""


def decode(x, start=0, threshold=210, clamp=True, tie_upper=True, end_in_lane_order=False, also_renorm=None):
    """every whole block of x, the first one from trellis state `start`.  The other arguments turn it into one of the WRONG decoders of the mutation
    check (docs/ORACLE_AND_PINS.md): another renormalisation threshold, sums left unclamped, ties to the lower predecessor, the end state searched in
    lane order, renormalisations at further steps (also_renorm[block, step], as when a wave renormalises both its trellises for either).
    tests/test_fec_conditions.py asserts that the sets tell each of them from the right one in the decoded bits, which counts of events alone do not."""
    x = np.asarray(x, np.uint8).astype(np.int64)
    nblk = (x.size - 12) // BLOCK_SYMS if x.size >= NEED_SYMS else 0
    r = Decoded()
    for k in ("one_over", "both_over", "sat_ties", "ties", "y0", "renorm", "rmin", "rspread"):
        setattr(r, k, np.zeros((nblk, STEPS), np.int64))
    for k in ("start", "end", "end_tied", "end_first_lane"):
        setattr(r, k, np.zeros(nblk, np.int64))
    bits = np.zeros(nblk * BLOCK_BITS, np.uint8)
    for f in range(nblk):
        sym = x[BLOCK_SYMS * f: BLOCK_SYMS * f + NEED_SYMS]
        X = np.full(64, 63, np.int64)
        X[start] = 0
        r.start[f] = start
        dec = np.zeros((STEPS, 64), np.int64)
        lo, up = np.empty(64, np.int64), np.empty(64, np.int64)
        for t in range(STEPS):
            m = (((((_B0 ^ sym[2 * t]) + (_B1 ^ sym[2 * t + 1]) + 1) >> 1) >> 2) & 63)
            # output state 2i: predecessors i (lower) and i + 32 (upper) with m and 63 - m; output state 2i + 1: the other way round
            lo[0::2], up[0::2] = X[:32] + m, X[32:] + (63 - m)
            lo[1::2], up[1::2] = X[:32] + (63 - m), X[32:] + m
            over_lo, over_up = lo > 255, up > 255
            cl, cu = np.minimum(lo, 255), np.minimum(up, 255)
            r.one_over[f, t] = np.count_nonzero(over_lo ^ over_up)
            r.both_over[f, t] = np.count_nonzero(over_lo & over_up)
            r.sat_ties[f, t] = np.count_nonzero((cl == cu) & (cl == 255))
            r.ties[f, t] = np.count_nonzero((cl == cu) & (cl < 255))
            if not clamp:
                cl, cu = lo, up
            dec[t] = cu <= cl if tie_upper else cu < cl      # the upper predecessor wins a tie
            Y = np.minimum(cl, cu)
            r.y0[f, t] = Y[0]
            if Y[0] > threshold or (also_renorm is not None and also_renorm[f, t]):
                r.renorm[f, t], r.rmin[f, t], r.rspread[f, t] = 1, Y.min(), Y.max() - Y.min()
                Y = Y - Y.min()
            X = Y
        tied = np.flatnonzero(X == X.min())
        r.end[f], r.end_tied[f] = tied[0], tied.size
        r.end_first_lane[f] = tied[np.argmin(LANE_AT_END[tied])]
        state = int(r.end_first_lane[f] if end_in_lane_order else tied[0])
        for nb in range(BLOCK_BITS - 1, -1, -1):
            k = int(dec[nb + 6, state])
            state = (state >> 1) | (k << 5)
            bits[BLOCK_BITS * f + nb] = k
            if nb == BLOCK_BITS - 6:
                start = state
    r.bits = bits
    r.out = descramble(bits)
    r.nblk = nblk
    return r


def descramble(bits):
    """descrambler_bb(0x8A, 0x7F, 7): out[k] = d[k] ^ parity(register & 0x8A), the register holding the 8 bits before, seeded 0x7F"""
    sr, out = 0x7F, np.empty(len(bits), np.uint8)
    for i, b in enumerate(bits):
        out[i] = _parity(sr & 0x8A) ^ int(b)
        sr = (sr >> 1) | (int(b) << 7)
    return out


@functools.lru_cache(maxsize=None)
def decoded(name, branch):
    return decode(branch_input(name, branch))


# ---------------------------------------------------------------- call schedules
def blocks_ready(nsyms):
    """blocks a unit can have decoded once it may read nsyms symbols"""
    return 0 if nsyms < NEED_SYMS else (nsyms - 12) // BLOCK_SYMS


def _stream_schedule(rng, mul):
    """per-call deliveries of one stream, in the items `avail` counts (avail_mul soft symbols each).  Pieces of 0, 1 and 171 items among random
    ones; with avail_mul 1 a call that ends on 160 k + 171 symbols (branch B, one symbol ahead, has a block and branch A has not) and a call of one
    symbol behind it (now A has one and B has not); a call of the largest size behind a remainder of 170 symbols, which completes four blocks."""
    cap, total = MAX_CALL_SYMS // mul, STREAM_SYMS // mul
    out, have = [], 0

    def walk_to(target):
        nonlocal have
        while have < target:
            u = rng.random()
            n = 0 if u < 0.12 else 1 if u < 0.24 else 171 if u < 0.40 else int(rng.integers(2, 171)) if u < 0.75 else int(rng.integers(172, cap + 1))
            n = min(n, cap, target - have)
            out.append(n)
            have += n

    k1, k2 = int(rng.integers(2, 12)), int(rng.integers(16, 30))
    if mul == 1:
        walk_to(BLOCK_SYMS * k1 + 171)
        out.append(1)
        have += 1
    walk_to((BLOCK_SYMS * k2 + 170) // mul)
    out.append(cap)
    have += cap
    walk_to(total)
    return out


@functools.lru_cache(maxsize=None)
def schedule(config, batch):
    """deliveries[call][stream] in items of `avail`; every stream ends on STREAM_SYMS soft symbols.  The streams' own schedules are brought to one
    length with calls that deliver nothing, at seeded places."""
    mul = CONFIGS[config][1]
    rng = np.random.default_rng([0x5C4ED, config, batch])
    per = [_stream_schedule(rng, mul) for _ in range(batch)]
    ncalls = max(len(p) for p in per) + 1
    d = np.zeros((ncalls, batch), np.int64)
    for b, p in enumerate(per):
        d[np.sort(rng.choice(ncalls, len(p), replace=False)), b] = p
    d.setflags(write=False)
    return d


def unit_sets(config, batch):
    """(set name, branch) of every unit of a case, in unit order"""
    branches = CONFIGS[config][0]
    return [(name, r) for name in BATCH_SETS[batch] for r in range(branches)]


def simulate(config, deliveries):
    """What each call of the decoder has to do.  Per call: avail (items per stream, as handed to the decoder), done0 / done1 (blocks every unit has
    decoded before / after it), passes (per wave, the kernel's block loop as a list of (block of the low unit or None, block of the high unit or
    None)), unread (per stream: soft symbols written and not consumed by the slowest of its units when the call starts decoding)."""
    branches, mul = CONFIGS[config]
    deliveries = np.asarray(deliveries)
    batch = deliveries.shape[1]
    nunits = batch * branches
    avail = np.zeros(batch, np.int64)
    done = np.zeros(nunits, np.int64)
    calls = []
    for d in deliveries:
        avail = avail + d
        after = np.array([blocks_ready(int(avail[u // branches]) * mul + (u % branches if branches == 2 else 0)) for u in range(nunits)])
        passes = []
        for w in range((nunits + 1) // 2):
            us = [u for u in (2 * w, 2 * w + 1) if u < nunits]
            n = [int(after[u] - done[u]) for u in us] + [0] * (2 - len(us))
            first = [int(done[u]) for u in us] + [0] * (2 - len(us))
            passes.append([tuple(first[q] + i if i < n[q] else None for q in range(2)) for i in range(max(n))])
        unread = np.array([int(avail[b]) * mul - BLOCK_SYMS * int(done[b * branches:(b + 1) * branches].min()) for b in range(batch)])
        calls.append(dict(avail=avail.copy(), done0=done.copy(), done1=after.copy(), passes=passes, unread=unread))
        done = after
    return calls
