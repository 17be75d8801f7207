#!/usr/bin/env python3
"""Writes tests/golden/ref/dmr_l2.npz: the scenario set of tests/dmr_l2.py (mailbox records of every DMR data type, rate 3/4 bursts from
clean to garbage, voice bursts A..F) and the 80-byte record the REFERENCE's own classes give for each of them (tests/host/dmr_l2_ref.cpp,
linked against oracle/_ref/libqrl_ref.so).  Needs the reference's sources; the file holds recorded inputs and results only."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmr_l2  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = dmr_l2.load_ref(tmp)
        if ref is None:
            sys.exit("the reference (sources and oracle/_ref/libqrl_ref.so) is not here")
        inputs, audio_fec, group = dmr_l2.build_scenarios(ref)
        records = ref.records(inputs, audio_fec)
        consts = np.array([ref.const(i) for i in range(8)], np.int32)
    np.savez_compressed(dmr_l2.GOLDEN, inputs=inputs, audio_fec=audio_fec, group=group, records=records, consts=consts)
    print("%s: %d records, %d bytes" % (dmr_l2.GOLDEN, inputs.shape[0], os.path.getsize(dmr_l2.GOLDEN)))


if __name__ == "__main__":
    main()
