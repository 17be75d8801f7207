#!/usr/bin/env python3
"""Writes tests/golden/ref/dmr_sink.npz: the scenario set of tests/dmr_sink.py as bit streams with their call cuts, flushes, resets and
rx_time tags, and what the REFERENCE's own gr_dmr_sink makes of them under the same cuts: the frame and slot records of every burst,
the bursts found per call, the sink's private state after every call and every slot time DMRTiming stored (its gr_dmr_sink.cpp, dmrframe.cpp
and dmrtiming.cpp compiled unmodified against oracle/gr_stub and the stand-ins of tests/host, tests/host/dmr_sink_ref.cpp, linked against
oracle/_ref/libqrl_ref.so).  The bursts are built by the reference's encoders (tests/host/dmr_tx_ref.cpp).  Needs the reference's sources;
the file holds recorded inputs and results only."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmr_sink  # noqa: E402
import dmr_tx  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref, tx_ref = dmr_sink.load_ref(tmp), dmr_tx.load_ref(tmp)
        if ref is None or tx_ref is None:
            sys.exit("the reference (sources and oracle/_ref/libqrl_ref.so) is not here")
        g = dmr_sink.record_golden(ref, tx_ref)
    np.savez_compressed(dmr_sink.GOLDEN, **g)
    print("%s: %d scenarios, %d bursts, %d bytes" % (dmr_sink.GOLDEN, len(g["names"]), int((g["call_of"] >= 0).sum()), os.path.getsize(dmr_sink.GOLDEN)))


if __name__ == "__main__":
    main()
