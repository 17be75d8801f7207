#!/usr/bin/env python3
"""Writes tests/golden/ref/m17_link.npz: the scenario set of tests/m17_link.py as streams of 56-byte frame-synchroniser records with the
64-byte link records and the decoder state (lsf, lsfFromLich, segment map, lock) the REFERENCE's own gr_modem::processReceivedData makes of
every frame, and the transmit calls (descriptors and payloads in, the bytes its startTransmission / transmitM17Audio / endTransmission hand to
the modulator out).  The reference's gr_modem.cpp, M17Transmitter.cpp, M17FrameDecoder.cpp, M17LinkSetupFrame.cpp, M17Callsign.cpp and
M17Golay.cpp are compiled unmodified behind tests/host/m17_link_ref.cpp.  Needs the reference's sources; the file holds recorded inputs and
results only."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import m17_link  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        ref = m17_link.load_ref(tmp)
        if ref is None:
            sys.exit("the reference's sources are not here")
        g = m17_link.record_golden(ref)
    np.savez_compressed(m17_link.GOLDEN, **g)
    print("%s: %d scenarios, %d frames, %d calls, %d bytes" % (m17_link.GOLDEN, g["inputs"].shape[0], int(g["counts"].sum()), g["tx_desc"].shape[0],
                                                              os.path.getsize(m17_link.GOLDEN)))


if __name__ == "__main__":
    main()
