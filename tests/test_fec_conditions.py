"""The conditions file of tests/test_gpu_fec_probe.py: what the soft-symbol sets and call schedules of tests/fec_points.py reach inside the
decoder, asserted on the CPU from the instrumented restatement alone (never from the device), and the oracle held to that restatement bit for bit
on every set.  The device test compares k_fec with the oracle on exactly these sets and schedules; this file is why that comparison means something."""
import numpy as np
import pytest

import appendix_a as A
import fec_points as P
import orc

ALL_UNITS = [(name, r) for name in P.FAMILIES for r in (0, 1)]
NCONF = len(P.CONFIGS)


@pytest.mark.parametrize("name,branch", ALL_UNITS)
def test_oracle_equals_the_instrumented_restatement(name, branch):
    x = P.branch_input(name, branch)
    d = P.decoded(name, branch)
    assert d.nblk == P.NBLOCKS and d.out.size == P.NBLOCKS * P.BLOCK_BITS
    dec = orc.cc_decode_k7(x)
    assert np.array_equal(dec, d.bits)
    assert np.array_equal(orc.descramble(dec), d.out)


def test_restatement_equals_appendix_a_on_one_set():
    """the third statement of the same kernel (tests/appendix_a.py, spiral variant), on the set with most of the conditions"""
    x = P.branch_input("coded_noise", 1)
    assert np.array_equal(A.cc_decode_k7(x, variant="spiral"), P.decoded("coded_noise", 1).bits)
    assert np.array_equal(A.descramble(P.decoded("coded_noise", 1).bits), P.decoded("coded_noise", 1).out)


def _n(a):
    return int(np.count_nonzero(a))


# what each set is there for (branch A of it, the stream itself); the figures are those of the restatement with a wide margin below them
BUTTERFLIES = 64 * P.STEPS * P.NBLOCKS


def test_sets_reach_what_they_claim():
    d = {name: P.decoded(name, 0) for name in P.FAMILIES}
    # coded bits at 0 / 255: one-sided saturation all the time, every renormalisation subtracts 0 (the right path stays at metric 0)
    c = d["coded_hard"]
    assert c.one_over.sum() > BUTTERFLIES // 8 and c.both_over.sum() == 0
    assert _n(c.renorm) > 500 and _n(c.renorm & (c.rmin == 0)) == _n(c.renorm)
    # coded + noise: both sums saturated by the hundred, saturated ties, metric[0] on either side of the threshold
    c = d["coded_noise"]
    assert c.both_over.sum() > 300 and c.sat_ties.sum() > 300 and _n(c.y0 == 210) >= 10 and _n(c.y0 == 211) >= 10
    assert _n(c.renorm & (c.rmin > 0)) > 100
    # uniform bytes and random hard symbols: both-saturated butterflies and tied end states
    for name in ("uniform", "random_hard"):
        c = d[name]
        assert c.both_over.sum() > 100 and _n(c.end_tied > 1) >= 1 and _n(c.start != 0) > 30
    # around the centre: a tie at a fifth to a quarter of all output states (most steps have some), all metrics rising together (a renormalisation
    # every seventh step, small spread)
    for name in ("const128", "const127", "alternating", "near_centre"):
        c = d[name]
        assert c.ties.sum() > BUTTERFLIES // 6 and _n(c.ties > 0) > P.STEPS * P.NBLOCKS * 3 // 4 and c.one_over.sum() == 0
        assert _n(c.renorm) == 12 * P.NBLOCKS and c.rspread[c.renorm == 1].max() <= 66 and c.rmin[c.renorm == 1].min() > 100
    assert _n(d["near_centre"].end_tied > 1) > 10 and _n(d["weak_code"].end_tied > 1) > 5
    # constant 0 / 255: saturating trellises that never, or once, renormalise
    assert _n(d["const0"].renorm) == 0 and d["const0"].one_over.sum() > BUTTERFLIES // 8
    assert _n(d["const255"].renorm) == 1 and d["const255"].one_over.sum() > BUTTERFLIES // 8
    # bursts: blocks that start from a chained state other than 0, and both kinds of renormalisation in one stream
    c = d["bursts"]
    assert _n(c.start != 0) > 30 and _n(c.renorm & (c.rmin == 0)) > 100 and _n(c.renorm & (c.rmin > 0)) > 10
    # the burst set differs from clean code in its bits only near the bursts: it recovers
    assert 0 < _n(P.decoded("bursts", 0).bits != _clean_bits_of_bursts()) < 40 * 20


def _clean_bits_of_bursts():
    return P._rng("bursts").integers(0, 2, (P.STREAM_SYMS + 1) // 2)[:P.NBLOCKS * P.BLOCK_BITS]


def _units_of(config):
    return sorted({u for batch in P.BATCHES for u in P.unit_sets(config, batch)})


def test_every_set_runs_in_every_configuration():
    used = [name for batch in P.BATCHES for name in P.BATCH_SETS[batch]]
    assert len(used) == len(set(used)) and set(used) | set(P.EXTRA_SETS) == set(P.FAMILIES)
    for batch in P.BATCHES:
        assert len(P.BATCH_SETS[batch]) == batch
    assert sorted(len(P.unit_sets(c, b)) for c in range(NCONF) for b in P.BATCHES) == [1, 2, 2, 2, 3, 4, 4, 5, 6, 6, 10, 10]


@pytest.mark.parametrize("config", range(NCONF))
def test_conditions_a_to_d_and_f_to_h_in_the_units_of_a_configuration(config):
    ds = [P.decoded(*u) for u in _units_of(config)]
    # (a) a butterfly with both sums above 255 -- which is a tie between two saturated sums -- and a saturated tie with one sum exactly at 255 or both
    assert any(d.both_over.sum() > 0 for d in ds) and any(d.sat_ties.sum() > 0 for d in ds)
    # (b) an unsaturated tie on steps with s mod 6 = 0 .. 5: every one of the six predecessor exchanges decides one
    for q in range(6):
        assert any(d.ties[:, q::6].sum() > 0 for d in ds)
    # (c) metric[0] = 210 (no renormalisation) and = 211 (one)
    assert any(_n((d.y0 == 210) & (d.renorm == 0)) > 0 for d in ds) and any(_n((d.y0 == 211) & (d.renorm == 1)) > 0 for d in ds)
    assert all(_n((d.y0 <= 210) & (d.renorm == 1)) == 0 and _n((d.y0 > 210) & (d.renorm == 0)) == 0 for d in ds)
    # (d) a renormalisation with a non-zero minimum and one with a zero minimum
    assert any(_n((d.renorm == 1) & (d.rmin > 0)) > 0 for d in ds) and any(_n((d.renorm == 1) & (d.rmin == 0)) > 0 for d in ds)
    # (f) a tied end state whose first holder in state order is not the first in the lane order of step 85
    assert any(_n((d.end_tied > 1) & (d.end != d.end_first_lane)) > 0 for d in ds)
    # (g) a block whose chained start state is not 0
    assert any(_n(d.start[1:] != 0) > 0 for d in ds)
    # (h) decoded bits that differ between branch A and branch B of one stream
    if P.CONFIGS[config][0] == 2:
        assert any(_n(P.decoded(name, 0).out != P.decoded(name, 1).out) > 0 for name, r in _units_of(config) if r == 1)


def test_lane_order_at_the_end_is_a_permutation_that_differs_from_state_order():
    assert sorted(P.LANE_AT_END.tolist()) == list(range(64)) and P.LANE_AT_END[0] == 0 and P.LANE_AT_END[1] == 2 and P.LANE_AT_END[2] == 1


def _passes(config, batch):
    """(low unit, high unit, block of low or None, block of high or None) of every pass of the block loop in which both units exist"""
    nunits = len(P.unit_sets(config, batch))
    for call in P.simulate(config, P.schedule(config, batch)):
        for w, wave in enumerate(call["passes"]):
            if 2 * w + 1 < nunits:
                for b0, b1 in wave:
                    yield 2 * w, 2 * w + 1, b0, b1


@pytest.mark.parametrize("config", range(NCONF))
def test_condition_e_one_half_of_a_wave_renormalises_alone(config):
    """(e) a pair of units that share a wave, both decoding a block in the same pass, and a step at which exactly one of them renormalises: the low half
    only and the high half only.  With two branches the pair is the two alignments of one stream, with one branch two different streams."""
    low_only = high_only = 0
    for batch in P.BATCHES:
        units = P.unit_sets(config, batch)
        for u0, u1, b0, b1 in _passes(config, batch):
            if b0 is None or b1 is None:
                continue
            r0, r1 = P.decoded(*units[u0]).renorm[b0], P.decoded(*units[u1]).renorm[b1]
            low_only += _n((r0 == 1) & (r1 == 0))
            high_only += _n((r0 == 0) & (r1 == 1))
    assert low_only > 0 and high_only > 0


def _differs(unit, **wrong):
    """decoded and descrambled bits of a unit's stream that one of the wrong decoders of fec_points.decode gets otherwise"""
    return _n(P.decode(P.branch_input(*unit), **wrong).out != P.decoded(*unit).out)


@pytest.mark.parametrize("config", range(NCONF))
def test_the_sets_tell_the_wrong_decoders_apart(config):
    """Reaching an event is not yet seeing it: most of the decoder's mistakes move all metrics of a trellis alike and leave the bits as they are.  For
    each mutation of the mutation check that is a property of one trellis, a unit of this configuration whose bits the restatement, made wrong in
    that way, decodes otherwise (counts of differing bits measured: 90 / 48 / 116 / 104 on uniform and random_hard A, 92 / 50 on coded_noise B)."""
    units = _units_of(config)
    assert ("uniform", 0) in units and ("random_hard", 0) in units and ("near_centre", 0) in units
    assert _differs(("uniform", 0), threshold=211) > 0                 # renormalisation threshold 211
    assert _differs(("uniform", 0), clamp=False) > 0                   # the upper sum left unclamped
    assert _differs(("uniform", 0), tie_upper=False) > 0 and _differs(("near_centre", 0), tie_upper=False) > 0     # ties to the lower predecessor
    assert _differs(("random_hard", 0), end_in_lane_order=True) > 0 and _differs(("near_centre", 0), end_in_lane_order=True) > 0   # `lend` dropped
    if P.CONFIGS[config][0] == 2:
        assert _differs(("coded_noise", 1), threshold=211) > 0 and _differs(("coded_noise", 1), clamp=False) > 0
        assert _differs(("random_hard", 1), clamp=False) > 0


@pytest.mark.parametrize("config", [c for c in range(NCONF) if P.CONFIGS[c][0] == 2])
def test_a_wave_that_renormalises_both_halves_for_either_decodes_otherwise(config):
    """the fifth mutation is a property of a pair: to first order, a unit that also renormalises at the steps at which its wave partner does, in the
    passes in which both decode a block.  Some unit of every two-branch configuration decodes other bits then (the partner is the other alignment
    of the same stream, whose trellis nears the threshold at the same places).  With one branch the partner is another stream, the early
    renormalisation has to fall on one of a few steps by chance, and no pairing of these sets has one: that mutation is seen by the two-branch cases."""
    hit = 0
    for batch in P.BATCHES:
        units = P.unit_sets(config, batch)
        also = {u: np.zeros((P.NBLOCKS, P.STEPS), np.int64) for u in range(len(units))}
        for u0, u1, b0, b1 in _passes(config, batch):
            if b0 is not None and b1 is not None:
                also[u0][b0], also[u1][b1] = P.decoded(*units[u1]).renorm[b1], P.decoded(*units[u0]).renorm[b0]
        for u, unit in enumerate(units):
            if unit[0] in ("uniform", "coded_noise", "random_hard"):     # (the other sets have no place where it would show; skipped for time)
                hit += _differs(unit, also_renorm=also[u]) > 0
    assert hit > 0


@pytest.mark.parametrize("batch", P.BATCHES)
@pytest.mark.parametrize("config", range(NCONF))
def test_schedule_conditions(config, batch):
    branches, mul = P.CONFIGS[config]
    s = P.schedule(config, batch)
    calls = P.simulate(config, s)
    assert s.shape[1] == batch and (s.sum(axis=0) * mul == P.STREAM_SYMS).all()
    # inside the product's contract for the ring: its smallest size, a call's symbols and the unread symbols no more than a handle's
    assert (s * mul <= P.MAX_CALL_SYMS).all() and max(int(c["unread"].max()) for c in calls) <= P.MAX_UNREAD < P.RING - 1
    # some calls deliver 0 items, some 1, some 171
    for v in (0, 1, 171):
        assert (s == v).any()
    # every unit decodes its 40 blocks; a call that completes exactly one block, one that completes four at once
    per_call = np.array([c["done1"] - c["done0"] for c in calls])
    assert (calls[-1]["done1"] == P.NBLOCKS).all()
    assert (per_call == 1).any() and (per_call == 4).any() and per_call.max() == 4 and (per_call == 0).any()
    # the ring wrapped at least three times
    assert P.STREAM_SYMS // P.RING >= 3
    # passes of the block loop in which one unit of a pair has a block and the other has not, in both orders.  Two alignments of one stream under
    # avail_mul = 2 can never differ: avail * 2 is even, a block boundary + 172 is even, and the one symbol branch B is ahead falls between them.
    low_only = sum(1 for _, _, b0, b1 in _passes(config, batch) if b0 is not None and b1 is None)
    high_only = sum(1 for _, _, b0, b1 in _passes(config, batch) if b0 is None and b1 is not None)
    if len(P.unit_sets(config, batch)) < 2:
        assert low_only == high_only == 0
    elif (branches, mul) == (2, 2):
        assert low_only == high_only == 0
    else:
        assert low_only > 0 and high_only > 0
