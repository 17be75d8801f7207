"""GPU: the analogue voice receivers (k_an_gate and the kernels behind it) under a WORKING squelch threshold and AGC rates, bit-exact
against the oracle through the C ABI: a gate that chatters on a fading carrier (ramps cut short, openings shorter than the ramp and
than the audio resampler's look-back, calls that pass nothing), the threshold and the rates moved while receiving, the AGC recursion
in both of its clamps.  Signals, cuttings and the conditions every case asserts on the ORACLE's result before it compares anything
are in tests/analog_controls.py; tests/test_analog_controls_restatement.py checks the oracle's side of all this on the CPU."""
import ctypes as C

import numpy as np
import pytest

import analog_controls as ac

pytestmark = pytest.mark.gpu


def _receive(qrl_ctx, rx, iq, sizes, setup=None, between=None):
    import qradiolink_amd as q
    dem = q.Demod(qrl_ctx, ac.RECEIVERS[rx]["modem"], batch=iq.shape[0], max_chunk=max(sizes))
    try:
        if setup:
            setup(dem)
        hook = (lambda k, delivered: between(dem, k, delivered)) if between else None
        return ac.run_calls(dem, iq, sizes, hook)
    finally:
        dem.close()


def _compare(rx, refs, got, sizes, gates=None):
    """port 0, port 1 and both counts equal the oracle's, stream by stream; with the gates, the counts of every single call too"""
    filt, aud, counts = got
    bounds = ac.call_items(rx, sizes)
    for b, ref in enumerate(refs):
        ac.assert_bit_equal(filt[b], ref["filtered"], "filtered, stream %d" % b)
        ac.assert_bit_equal(aud[b], ref["audio"], "audio, stream %d" % b)
        assert [c[b][0] for c in counts] == [b1 - b0 for b0, b1 in zip(bounds[:-1], bounds[1:])], "port 0 counts, stream %d" % b
        if gates is not None:
            g = [int(gates[b].cum[i]) for i in bounds]
            want = [ac.audio_count(rx, g1) - ac.audio_count(rx, g0) for g0, g1 in zip(g[:-1], g[1:])]
            assert [c[b][1] for c in counts] == want, "port 1 counts, stream %d" % b


@pytest.mark.parametrize("cut", ac.CUTTINGS)
@pytest.mark.parametrize("rx", list(ac.RECEIVERS))
def test_squelch_chatter(qrl_ctx, rx, cut):
    iq, refs, gates = ac.chatter_case(rx)
    sizes = ac.cutting(cut, rx, gates[0])
    ac.check_conditions(rx, refs, gates, ac.call_items(rx, sizes))
    got = _receive(qrl_ctx, rx, iq, sizes, setup=lambda dem: dem.set_squelch(ac.THRESHOLD))
    _compare(rx, refs, got, sizes, gates)


def test_nbfm_chatter_with_ctcss(qrl_ctx):
    """set_ctcss(88.5) behind the chattering power squelch: the tone gate's input count differs from call to call, some calls bring it nothing"""
    iq, refs, gates, sizes = ac.ctcss_case()
    bounds = ac.call_items("nbfm5000", sizes)
    per_call = [ac.audio_count("nbfm5000", int(gates[0].cum[b1])) - ac.audio_count("nbfm5000", int(gates[0].cum[b0])) for b0, b1 in zip(bounds[:-1], bounds[1:])]
    assert gates[0].transitions.size >= 6 and len(set(per_call)) > len(per_call) // 2 and 0 in per_call
    assert refs[0]["audio"].size > 2000 and refs[1]["audio"].size == 0 and refs[1]["filtered"].size == bounds[-1]

    def setup(dem):
        dem.set_ctcss(88.5)
        dem.set_squelch(ac.THRESHOLD)
    _compare("nbfm5000", refs, _receive(qrl_ctx, "nbfm5000", iq, sizes, setup=setup), sizes)


def test_wave_filling_batch(qrl_ctx):
    """66 distinct streams: one full wave of k_an_gate and a second block; neighbouring lanes are in different states at the same item"""
    iq, refs, gates = ac.chatter_case("nbfm5000", 66)
    sizes = ac.cutting("ragged", "nbfm5000", gates[0])
    ac.check_conditions("nbfm5000", refs, gates, ac.call_items("nbfm5000", sizes))
    st = np.stack([g.state for g in gates[:64]])
    assert np.count_nonzero([len(set(st[:, i])) == 4 for i in range(0, st.shape[1], 8)]) > 20
    got = _receive(qrl_ctx, "nbfm5000", iq, sizes, setup=lambda dem: dem.set_squelch(ac.THRESHOLD))
    _compare("nbfm5000", refs, got, sizes, gates)


@pytest.mark.parametrize("direction", list(ac.MOVES))
@pytest.mark.parametrize("rx", ["nbfm5000", "am"])
def test_threshold_moved_while_receiving(qrl_ctx, rx, direction):
    """set_squelch(db2) between two calls, no reset: the estimate and the state machine carry on (pwr_squelch_cc::set_threshold)"""
    case = ac.moved_threshold_case(rx, direction)
    iq, sizes, k, at, refs, gates = case
    ac.check_moved_threshold(rx, direction, case)
    db1, db2 = ac.MOVES[direction]

    def between(dem, call, delivered):
        if call == k:
            assert delivered == at
            dem.set_squelch(db2)
    got = _receive(qrl_ctx, rx, iq, sizes, setup=lambda dem: dem.set_squelch(db1), between=between)
    _compare(rx, refs, got, sizes, gates)


def _agc_gates(rx, refs):
    return [ac.Gate(rx, r["filtered"], ac.AGC_THRESHOLD) for r in refs]


@pytest.mark.parametrize("cut", ["one", "ragged"])
@pytest.mark.parametrize("knob", ac.AGC_KNOBS)
@pytest.mark.parametrize("rx", ["am", "usb", "lsb"])
def test_agc_rates(qrl_ctx, rx, knob, cut):
    """set_agc with what gr_demod_base::set_agc_attack(int) / set_agc_decay(int) make of the GUI's knobs; (1, 100) takes both clamps of the
    recursion on these signals (tests/test_analog_controls_restatement.py::test_agc_inputs_take_both_clamps)"""
    iq, ragged, _, _, refs = ac.agc_case(rx, knob)
    sizes = ragged if cut == "ragged" else [iq.shape[1]]
    gates = _agc_gates(rx, refs)
    assert all(r["audio"].size >= 2048 and np.isfinite(r["audio"]).all() for r in refs)
    if knob != (-10, -10):   # the rates matter: not the audio of the constructor's (0.1, 0.1)
        assert refs[0]["audio"].tobytes() != ac.agc_case(rx, (-10, -10))[4][0]["audio"].tobytes()
    a, d = ac.knob_rates(knob)

    def setup(dem):
        dem.set_squelch(ac.AGC_THRESHOLD)
        dem.set_agc(a, d)
    _compare(rx, refs, _receive(qrl_ctx, rx, iq, sizes, setup=setup), sizes, gates)


@pytest.mark.parametrize("rx", ["am", "usb"])
def test_agc_rates_moved_while_receiving(qrl_ctx, rx):
    """set_agc between two calls: the gain is kept (agc2::set_attack_rate / set_decay_rate)"""
    knob, knob2 = (-10, -10), (3, 2)
    iq, sizes, k, at, refs = ac.agc_case(rx, knob, knob2)
    for other in (knob, knob2):
        assert refs[0]["audio"].tobytes() != ac.agc_case(rx, other)[4][0]["audio"].tobytes()

    def setup(dem):
        dem.set_squelch(ac.AGC_THRESHOLD)
        dem.set_agc(*ac.knob_rates(knob))

    def between(dem, call, delivered):
        if call == k:
            assert delivered == at
            dem.set_agc(*ac.knob_rates(knob2))
    _compare(rx, refs, _receive(qrl_ctx, rx, iq, sizes, setup=setup, between=between), sizes, _agc_gates(rx, refs))


def test_refusals_leave_the_handle_usable(qrl_ctx):
    """set_agc is AM's and SSB's, set_squelch the analogue receivers': QRL_ERR_ARG elsewhere, and nothing has changed"""
    import torch
    import qradiolink_amd as q
    import sig
    QRL_ERR_ARG = -1
    lib = qrl_ctx.lib
    for rx in ("nbfm5000", "wbfm"):
        iq, refs, gates = ac.chatter_case(rx)
        sizes = ac.cutting("ragged", rx, gates[0])

        def setup(dem):
            dem.set_squelch(ac.THRESHOLD)
            assert lib.qrl_demod_set_agc(dem.h, C.c_float(60.0), C.c_float(2.0)) == QRL_ERR_ARG
            with pytest.raises(q.QrlError):
                dem.set_agc(60.0, 2.0)
        _compare(rx, refs, _receive(qrl_ctx, rx, iq, sizes, setup=setup), sizes, gates)
    x = torch.from_numpy(sig.make_batch("gmsk10k", 2, nframes=2, seed=3)).cuda()
    outs = []
    for refuse in (False, True):
        dem = q.Demod(qrl_ctx, q.MODEM_GMSK10K, batch=2, max_chunk=x.shape[1], carrier_offset_hz=25000.0)
        if refuse:
            assert lib.qrl_demod_set_agc(dem.h, C.c_float(60.0), C.c_float(2.0)) == QRL_ERR_ARG
            assert lib.qrl_demod_set_squelch(dem.h, C.c_double(-34.0)) == QRL_ERR_ARG
        outs.append(q.collect(dem, x, x.shape[1]))
        if refuse:   # ... also between two calls
            assert lib.qrl_demod_set_squelch(dem.h, C.c_double(-34.0)) == QRL_ERR_ARG
            dem.reset()
            outs.append(q.collect(dem, x, x.shape[1]))
        dem.close()
    for b in range(2):
        assert outs[0]["bits_a"][b].size > 500
        for port in ("bits_a", "bits_b", "filtered", "constellation"):
            assert outs[0][port][b].tobytes() == outs[1][port][b].tobytes() == outs[2][port][b].tobytes(), (port, b)
