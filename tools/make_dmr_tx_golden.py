#!/usr/bin/env python3
"""Writes tests/golden/ref/dmr_tx.npz: the scenario set of tests/dmr_tx.py (TX records of every kind; whole calls of 31 voice bursts) and
the 33-byte bursts the REFERENCE's own classes make of them: DMRFrame and the MMDVM encoders per record, DMRControl (its dmrcontrol.cpp
compiled unmodified against tests/host/dmr_ctl_stub) per call (tests/host/dmr_tx_ref.cpp, linked against oracle/_ref/libqrl_ref.so).
Needs the reference's sources; the file holds recorded inputs and results only."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmr_tx  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = dmr_tx.load_ref(tmp)
        if ref is None:
            sys.exit("the reference (sources and oracle/_ref/libqrl_ref.so) is not here")
        g = dmr_tx.record_golden(ref)
    np.savez_compressed(dmr_tx.GOLDEN, **g)
    print("%s: %d records, %d calls, %d bytes" % (dmr_tx.GOLDEN, g["records"].shape[0], g["calls"].shape[0], os.path.getsize(dmr_tx.GOLDEN)))


if __name__ == "__main__":
    main()
