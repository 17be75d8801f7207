"""The conditions of tests/test_gpu_reset.py, on the oracle alone: every dirt stream A of tests/reset_streams.py leaves state behind that
changes what the clean stream B gives -- oracle(A | B) behind A's items differs from oracle(B) on EVERY port the GPU test compares, so a handle
whose reset did nothing cannot pass -- and every A ends where it is meant to: off the decimation, the symbol, the decoder's 160-symbol block,
the RSSI block's 2000 and, for the bit-level blocks, inside a frame behind its sync word."""
import numpy as np
import pytest

import reset_streams as rs


def _ids(cases):
    return [c.name for c in cases]


def _dirt_matters(case):
    for b in range(case.nb):
        for port, (carried, alone) in case.carried(b).items():
            if port in case.SILENT:
                assert alone.size == 0 and carried.size == 0, (case, port, b)
                continue
            assert not rs._bits_equal(carried, alone), "%s: A leaves port %s of stream %d as a fresh handle gives it" % (case, port, b)


@pytest.mark.parametrize("case", rs.RX_CASES + rs.ANALOG_CASES, ids=_ids(rs.RX_CASES + rs.ANALOG_CASES))
def test_receiver_dirt_matters_and_ends_off_every_grid(case):
    A, B = case.streams()
    na = A.shape[1]
    assert na % 2 == 0 and B.shape[1] % 2 == 0
    cuts_a, cuts_b = case.cuts()
    assert len(cuts_a) % 2 == 1 and len(cuts_a) >= 3 and sum(cuts_a) == na and sum(cuts_b) == B.shape[1] and len(cuts_b) >= 6
    if getattr(case, "chunk", 0):     # small calls: A laps the decimated rings of a handle with that max_chunk
        assert len(cuts_a) > 3 and max(cuts_a + cuts_b) == case.chunk
        assert all(case.oracle(A[b], b)["filtered"].size > case.ring + 1024 for b in range(case.nb))
    else:
        assert len(cuts_a) == 3
    D = getattr(case, "D", 1)
    if D > 1:
        assert na % D, (na, D)
    n1 = rs.orc.lib.orc_decim_count(na, 1, D) if D > 1 else na          # A's samples at 1 Msps
    if case.decim != 2:           # (an even length cannot avoid the 1:2 stages)
        assert n1 % case.decim, (n1, case.decim)
    if case.sps_1m and case.sps_1m != 2:
        assert n1 % case.sps_1m > 0.5, (n1, case.sps_1m)
    if case.kind == "rx":
        for b in range(case.nb):
            symbols = case.oracle(A[b], b)["constellation"].size
            assert symbols > 0 and symbols % 160, (b, symbols)
    _dirt_matters(case)
    for ref in case.refs():       # a vacuous comparison cannot pass
        assert ref["filtered"].size > 1000
        if case.kind == "analog":
            assert ref["audio"].size >= 1024


TX_CASES = rs.MOD_CASES + rs.AMOD_CASES + rs.SYNTH_CASES


@pytest.mark.parametrize("case", TX_CASES, ids=["%s-%s" % (c.kind, c.name) for c in TX_CASES])
def test_transmitter_dirt_matters(case):
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    assert sum(cuts_a) == A.shape[-1] and sum(cuts_b) == B.shape[-1] and len(cuts_b) >= 2
    assert len(cuts_a) == 3 or case.name == "dsss"        # (one byte of DSSS is a million samples)
    if getattr(case, "mode", None) == "nbfm":             # calls of whole groups of four audio items: an odd number of groups
        assert A.shape[-1] % 8 == 4
    elif getattr(case, "block", 1) == 1 and len(cuts_a) == 3:
        assert A.shape[-1] % 2 == 1
    _dirt_matters(case)
    if getattr(case, "zero_run", None):                   # the queued run would change B if the reset kept it
        for b in range(case.nb):
            assert not rs._bits_equal(case.oracle_if_fired(b), case.refs()[b]["iq"]), (case, b)
    if getattr(case, "sc16", None):                       # some components clip in A and in B: the counts have something to add
        for b in range(case.nb):
            assert rs.to_sc16(case.oracle(A[b], b)["iq"], case.sc16)[1] > 0 and rs.to_sc16(case.refs()[b]["iq"], case.sc16)[1] > 0


@pytest.mark.parametrize("case", rs.CHAN_CASES, ids=_ids(rs.CHAN_CASES))
def test_wideband_dirt_matters(case):
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    assert len(cuts_a) % 2 == 1 and sum(cuts_a) == A.shape[-1] and sum(cuts_b) == B.shape[-1]
    if case.chunk_inst:               # A laps the channel ring
        assert len(cuts_a) > 3 and case.inst_a > case.ring + 1024 and max(cuts_a + cuts_b) == case.chunk_inst * case.D
    else:
        assert len(cuts_a) == 3
    if case.form in (1, 2):
        assert A.shape[-1] % case.D
    for b in range(A.shape[0]):
        for port, (carried, alone) in case.carried(b).items():
            assert alone.size > 0 and not rs._bits_equal(carried, alone), (case, port, b)


@pytest.mark.parametrize("case", rs.BITS_CASES, ids=_ids(rs.BITS_CASES))
def test_bit_level_dirt_ends_inside_a_frame_and_matters(case):
    A, B = case.streams()
    cuts_a, cuts_b = case.cuts()
    assert len(cuts_a) == 3 and sum(cuts_a) == A.shape[1] and sum(cuts_b) == B.shape[1] and min(cuts_b) > 0
    for b in range(case.nb):
        found, index = case.in_frame(b)
        assert found == 1 and index >= 19, (case, b, found, index)          # behind a sync word, 19 bits or more into its frame
    _dirt_matters(case)
    assert all(r["records"].size > 0 for r in case.refs())


def test_rssi_dirt_ends_inside_a_block_and_matters():
    A, B = rs.rssi_streams()
    assert A.shape == (rs.RSSI_STREAMS, rs.RSSI_DIRT) and rs.RSSI_DIRT % 2000 == 500
    for b in (0, 1, 37, 69):
        carried = rs.orc.rssi_block(np.concatenate([A[b], B[b]]), level=rs.RSSI_LEVEL)[rs.RSSI_DIRT:]
        assert not rs._bits_equal(carried, rs.orc.rssi_block(B[b], level=rs.RSSI_LEVEL)), b


def test_fft_dirt_would_show_in_the_frame_after_set_fft_size():
    """had set_fft_size kept the half-filled buffer, the next frame of 512 would be A: another tone"""
    A, B = rs.fft_streams()
    n = rs.FFT_SIZE // 2
    w = np.hamming(n).astype(np.float32)
    for b in range(rs.NB):
        stale, fresh = rs.orc.power_spectrum(A[b, :n], w), rs.orc.power_spectrum(B[b, :n], w)
        assert np.argmax(stale) != np.argmax(fresh)
