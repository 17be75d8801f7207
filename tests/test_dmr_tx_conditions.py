"""What the radio loopback of tests/test_gpu_dmr_tx.py rests on, stated with the oracle alone (no device): the bytes of a call of 2 LC
headers + 12 voice bursts + 2 terminators + 2 empty frames, as the reference lays them out (72-byte slots, from the recorded frames of
tests/golden/ref/dmr_tx.npz), through the oracle's gr_mod_dmr, gr_demod_dmr and DMO slicer.  The condition, not a measurement
(dmr_tx.check_radio_records): from some burst on the oracle's receiver delivers every voice burst of the call with no gap, including at
least one complete superframe -- and what it delivers decodes to what was encoded."""
import numpy as np
import pytest

import dmr_l2
import dmr_tx
import orc

G = dmr_tx.load_golden()


@pytest.mark.parametrize("zero_runs", [False, True])
@pytest.mark.parametrize("m", dmr_tx.RADIO_CALLS)
def test_the_oracle_s_receiver_delivers_every_voice_burst(m, zero_runs):
    assert G["call_repeater"][m] == 0
    data, _, runs = dmr_tx.radio_call(G, m)
    sliced = orc.DmoSink().process(orc.demod_dmr_port3(orc.mod_dmr(data, zero_runs=runs if zero_runs else None) * np.float32(0.05)))
    rec = np.array([list(dmr_l2.record(bytes([t, fn, cc, 0]) + burst + bytes(3), 0)) for t, fn, cc, burst in sliced], np.uint8)
    dmr_tx.check_radio_records(G, rec, m, zero_runs)
