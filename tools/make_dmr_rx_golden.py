#!/usr/bin/env python3
"""Writes tests/golden/ref/dmr_rx.npz: the scenario set of tests/dmr_rx.py as streams of 40-byte slicer records, and the 128-byte call
records the REFERENCE's own DMRControl makes of them, one addFrames call per burst (its dmrcontrol.cpp compiled unmodified against
tests/host/dmr_rx_stub and tests/host/dmr_ctl_stub, tests/host/dmr_rx_ref.cpp, linked against oracle/_ref/libqrl_ref.so).  The bursts are
built by the reference's encoders (tests/host/dmr_tx_ref.cpp).  Needs the reference's sources; the file holds recorded inputs and results only."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmr_rx  # noqa: E402
import dmr_tx  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref, tx_ref = dmr_rx.load_ref(tmp), dmr_tx.load_ref(tmp)
        if ref is None or tx_ref is None:
            sys.exit("the reference (sources and oracle/_ref/libqrl_ref.so) is not here")
        g = dmr_rx.record_golden(ref, tx_ref)
    np.savez_compressed(dmr_rx.GOLDEN, **g)
    print("%s: %d scenarios, %d bursts, %d bytes" % (dmr_rx.GOLDEN, g["inputs"].shape[0], int(g["counts"].sum()), os.path.getsize(dmr_rx.GOLDEN)))


if __name__ == "__main__":
    main()
