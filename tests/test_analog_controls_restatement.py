"""CPU: the oracle's squelch threshold and AGC rate parameters (oracle/orc_analog.c: orc_set_rx_squelch, orc_set_rx_agc, changeable in
mid-stream) against a second, separately written restatement -- the power recursion and the four-state machine in Python doubles,
agc2_ff / agc2_cc in numpy float32 scalars.  Counts must be EQUAL and samples BIT-EXACT: both sides are the same arithmetic.
The same tests establish that the inputs of tests/test_gpu_analog_controls.py do what that file requires of them (transitions,
short runs, empty calls, both clamps of the AGC recursion); the GPU tests assert the same conditions again before they compare."""
import functools

import numpy as np
import pytest

import analog_controls as ac
import orc
import sig


def squelch_restated(filtered, db, ramp, switch=None, alpha=0.01):
    """pwr_squelch_cc(db, alpha, ramp, gate = true) written from gr-analog's squelch_base_cc_impl.cc / pwr_squelch_cc_impl.cc: per item the power
    estimate is updated and the flag taken, then the state machine steps, then the item passes unless the state is MUTED.
    -> (passed, state) per input item"""
    re, im = filtered.real.astype(np.float32), filtered.imag.astype(np.float32)
    p = (re * re + im * im).astype(np.float64)            # two float32 products, one float32 sum (numpy does not contract), then widened
    MUTED, ATTACK, UNMUTED, DECAY = 0, 1, 2, 3
    threshold = 10.0 ** (db / 10)
    pwr, state, ramped = 0.0, MUTED, 0
    passed, states = np.zeros(p.size, bool), np.zeros(p.size, np.uint8)
    for i, pi in enumerate(p.tolist()):
        if switch is not None and i == switch[0]:
            threshold = 10.0 ** (switch[1] / 10)
        pwr = alpha * pi + (1.0 - alpha) * pwr
        mute = pwr < threshold
        if state == MUTED:
            if not mute:
                state = ATTACK if ramp else UNMUTED
        elif state == UNMUTED:
            if mute:
                state = DECAY if ramp else MUTED
        elif state == ATTACK:
            ramped += 1
            if ramped >= ramp:
                state = UNMUTED
        else:
            ramped -= 1
            if ramped == 0:
                state = MUTED
        passed[i], states[i] = state != MUTED, state
    return passed, states


def test_default_controls_reproduce_the_constructors_graph():
    """no argument = -140 dB and (0.1, 0.1), spelled out or not (the goldens of tests/golden pin the values themselves)"""
    x = sig.make_analog("am", n=100000, seed=4, gap=(30000, 60000))[0]
    a, b = orc.demod_analog(x, "am"), orc.demod_analog(x, "am", squelch=-140.0, agc=(0.1, 0.1), squelch_switch=(700, -140.0), agc_switch=(900, 0.1, 0.1))
    assert a["audio"].size > 500 and a["audio"].tobytes() == b["audio"].tobytes()
    y = sig.make_ssb(n=400000, seed=4)
    a, b = orc.demod_ssb(y), orc.demod_ssb(y, squelch=-140.0, agc=(0.1, 0.1), agc_switch=(1000, 0.1, 0.1))
    assert a["audio"].size >= 2048 and a["audio"].tobytes() == b["audio"].tobytes()
    assert orc.demod_ssb(y)["audio"].tobytes() == a["audio"].tobytes()     # and the settings do not outlive a call


@pytest.mark.parametrize("rx", list(ac.RECEIVERS))
def test_squelch_restatement_and_chatter_inputs(rx):
    R = ac.RECEIVERS[rx]
    iq, refs, gates = ac.chatter_case(rx)
    for b, (ref, g) in enumerate(zip(refs, gates)):
        passed, states = squelch_restated(ref["filtered"], ac.THRESHOLD, R["ramp"])
        assert int(passed.sum()) == int(g.cum[-1]) and np.array_equal(passed, g.passed) and np.array_equal(states, g.state), b
        assert ref["audio"].size == ac.audio_count(rx, int(passed.sum())), b
        # at the constructor's threshold none of this happens: the gate opens once
        assert np.count_nonzero(np.diff(squelch_restated(ref["filtered"], -140.0, R["ramp"])[0].astype(np.int8))) == 1, b
    for name in ac.CUTTINGS:
        sizes = ac.cutting(name, rx, gates[0])
        assert sum(sizes) == R["n"] and min(sizes) > 0
        ac.check_conditions(rx, refs, gates, ac.call_items(rx, sizes))
    fine = ac.cutting("fine", rx, gates[0])
    per_call = gates[0].per_call(ac.call_items(rx, fine))
    assert any(s & 1 for s in fine) and min(fine) < 20 * R["decim"] and per_call.count(0) >= 5 and any(0 < c < 16 for c in per_call)


@pytest.mark.parametrize("direction", list(ac.MOVES))
@pytest.mark.parametrize("rx", ["nbfm5000", "am"])
def test_squelch_restatement_threshold_moved(rx, direction):
    case = ac.moved_threshold_case(rx, direction)
    _, _, _, at, refs, gates = case
    db1, db2 = ac.MOVES[direction]
    for b, (ref, g) in enumerate(zip(refs, gates)):
        passed, states = squelch_restated(ref["filtered"], db1, ac.RECEIVERS[rx]["ramp"], (at, db2))
        assert np.array_equal(passed, g.passed) and np.array_equal(states, g.state), b
        assert ref["audio"].size == ac.audio_count(rx, int(passed.sum())), b
    ac.check_moved_threshold(rx, direction, case)


def test_wave_filling_batch_inputs():
    iq, refs, gates = ac.chatter_case("nbfm5000", 66)
    assert len({x.tobytes() for x in iq}) == 66
    sizes = ac.cutting("ragged", "nbfm5000", gates[0])
    ac.check_conditions("nbfm5000", refs, gates, ac.call_items("nbfm5000", sizes))
    # neighbouring lanes of k_an_gate sit in different states at the same item: every state occurs, at many items, in one wave
    st = np.stack([g.state for g in gates[:64]])
    assert np.count_nonzero([len(set(st[:, i])) == 4 for i in range(0, st.shape[1], 8)]) > 20
    assert sum(g.transitions.size >= 6 for g in gates) >= 60


def test_ctcss_chatter_inputs():
    iq, refs, gates, sizes = ac.ctcss_case()
    assert gates[0].transitions.size >= 6 and refs[0]["audio"].size > 2000 and refs[1]["audio"].size == 0
    per_call = [ac.audio_count("nbfm5000", int(gates[0].cum[b1])) - ac.audio_count("nbfm5000", int(gates[0].cum[b0])) for b0, b1 in zip(ac.call_items("nbfm5000", sizes)[:-1], ac.call_items("nbfm5000", sizes)[1:])]
    assert len(set(per_call)) > len(per_call) // 2 and 0 in per_call           # the tone gate's input count varies from call to call


REF = {"am": 1.0, "usb": 0.25}


@functools.lru_cache(maxsize=None)
def _agc(rx, knob):
    """restated AGC of stream 0 of the AGC case, compared with the oracle's block: -> (clamp-at-zero hits, clamp-at-max hits)"""
    _, _, _, _, refs = ac.agc_case(rx, knob)
    x = ac.agc_input(rx, refs[0]["filtered"])
    a, d = ac.knob_rates(knob)
    out, low, high, _ = ac.agc_restated(x, a, d, REF[rx])
    want = orc.agc2(x, a, d, REF[rx], 1.0) if rx == "usb" else orc.agc2_ff(x, a, d, REF[rx], 1.0)
    assert out.size > 7000 and out.tobytes() == want.tobytes()
    return low, high


@pytest.mark.parametrize("knob", ac.AGC_KNOBS)
@pytest.mark.parametrize("rx", ["am", "usb"])
def test_agc_restatement(rx, knob):
    _agc(rx, knob)


@pytest.mark.parametrize("rx", ["am", "usb"])
def test_agc_inputs_take_both_clamps(rx):
    hits = {knob: _agc(rx, knob) for knob in ac.AGC_KNOBS}
    assert any(low > 0 for low, _ in hits.values()) and any(high > 0 for _, high in hits.values()), hits
    assert hits[(-10, -10)] == (0, 0), hits      # the constructor's rates reach neither, even on this signal


def test_knob_mapping():
    """gr_demod_base::set_agc_attack(int) / set_agc_decay(int), reference src/gr/gr_demod_base.cpp:1420-1461"""
    assert [ac.knob_rates(k) for k in ac.AGC_KNOBS[:4]] == [(float(np.float32(0.1)), float(np.float32(0.1))), (1.0, 1.0), (60.0, 2.0), (float(np.float32(0.01)), 5.0)]


@pytest.mark.parametrize("rx", ["am", "usb"])
def test_agc_restatement_rates_moved(rx):
    """set_attack_rate / set_decay_rate in mid-stream keep the gain; the oracle's chains take the switch point as a squelch-input index"""
    knob, knob2 = (-10, -10), (3, 2)
    iq, sizes, k, at, refs = ac.agc_case(rx, knob, knob2)
    (a, d), (a2, d2) = ac.knob_rates(knob), ac.knob_rates(knob2)
    f = refs[0]["filtered"]
    x = ac.agc_input(rx, f)
    before = int(ac.Gate(rx, f, ac.AGC_THRESHOLD).cum[at])          # the AGC's own index of the switch: items that passed the gate before `at`
    assert 0 < before < x.size and before < at
    out, _, _, gain_at = ac.agc_restated(x, a, d, REF[rx], (before, a2, d2))
    block = orc.agc2 if rx == "usb" else orc.agc2_ff
    want = np.concatenate([block(x[:before], a, d, REF[rx], 1.0), block(x[before:], a2, d2, REF[rx], float(gain_at))])
    assert out.tobytes() == want.tobytes()
    # the chain: the audio that depends on items before the switch only is that of the unswitched chain, the rest is not; a switch at
    # item 0 is the second pair throughout, one behind the last item changes nothing
    plain = ac.oracle(rx, iq[0], squelch=ac.AGC_THRESHOLD, agc=(a, d))["audio"]
    sw = refs[0]["audio"]
    head = ac.audio_count(rx, before)                               # (resampler and filters are causal; the stretcher's two items of look-ahead are inside its count)
    assert sw.size == plain.size and head > 500 and sw[:head].tobytes() == plain[:head].tobytes() and sw.tobytes() != plain.tobytes()
    whole = ac.oracle(rx, iq[0], squelch=ac.AGC_THRESHOLD, agc=(a2, d2))["audio"]
    assert ac.oracle(rx, iq[0], squelch=ac.AGC_THRESHOLD, agc=(a, d), agc_switch=(0, a2, d2))["audio"].tobytes() == whole.tobytes()
    assert ac.oracle(rx, iq[0], squelch=ac.AGC_THRESHOLD, agc=(a, d), agc_switch=(f.size, a2, d2))["audio"].tobytes() == plain.tobytes()
