"""The M17 link layer through the C++ facade (tests/host/test_m17_link_facade.cpp), both directions in one run of the host test program.
Transmit: setM17Call / txM17Audio / endM17Call of gr_modem_hip put into the modulator's byte path the bytes the reference's startTransmission,
transmitM17Audio and endTransmission emit (the recorded calls of tests/golden/ref/m17_link.npz, and what the scalar core, which
tests/test_m17_link.py holds to the reference, gives for the others).  Receive: those bytes through the M17 modulator and the M17 receiver
with the device frame synchroniser; with set_m17_link on, gr_modem_hip::demodulate hands every frame of the m17Frame callback to
m17LinkEvents as well, as the 64-byte record the scalar core gives for the same frames with the state carried across the work() calls;
host/m17_link_hip.h reads that record; off (the default) no event fires and m17Frame is what it was."""
import os
import subprocess

import numpy as np
import pytest

import m17_link as M

pytestmark = pytest.mark.gpu

EXE = os.path.join(M.ROOT, "tests", "host", "test_m17_link_facade")
G = M.load_golden()
# (source, destination, CAN, destination_type, frames): three recorded calls and two more
CALLS = [("YO8RZZ", "AB1CDE", 0, 0, 7), ("YO8RZZ", "", 2, 2, 2), ("N0CALL", "", 15, 0, 3), ("DL1ABC-9", "W1AW/P", 5, 0, 14), ("", "", 3, 4, 6)]
GOLDEN_NAMES = {0: "type_0", 1: "type_2", 2: "empty_destination"}


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(M.ROOT, "qradiolink_amd", "csrc"), "m17_link_facade"])
    return EXE


def _payloads(s, n):
    return np.array([[(31 * (s + 1) + 7 * k + 3 * j + 1) & 255 for j in range(16)] for k in range(n)], np.uint8).reshape(n, 16)


def _run(tmp, link, can_rx, all_can):
    path = os.path.join(str(tmp), "calls.txt")
    with open(path, "w") as f:
        for src, dst, can, dtype, n in CALLS:
            f.write("%s %s %d %d %d\n" % (src or "-", dst or "-", can, dtype, n))
    pre = os.path.join(str(tmp), "out")
    r = subprocess.run([_exe(), path, pre, str(int(link)), str(can_rx), str(int(all_can))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d streams" % len(CALLS)), r.stdout
    frames = [int(x) for x in r.stdout.split("frames")[1].split()]
    tx = [np.fromfile(pre + ".tx.%d.bin" % s, np.uint8) for s in range(len(CALLS))]
    ev = [np.fromfile(pre + ".ev.%d.bin" % s, np.uint8).reshape(-1, M.REC) for s in range(len(CALLS))]
    get = [[l.split() for l in open(pre + ".get.%d.txt" % s).read().splitlines()] for s in range(len(CALLS))]
    return frames, tx, ev, get


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return M.load_core(tmp_path_factory.mktemp("m17_link_facade_core"))


@pytest.fixture(scope="module")
def on(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("m17_link_facade_on"), True, 5, False)


def test_transmit_bytes_are_the_reference_s(on, core):
    _, tx, _, _ = on
    for s, (src, dst, can, dtype, n) in enumerate(CALLS):
        desc = M.descriptor(src, dst, can, dtype)
        pay = _payloads(s, n)
        want = np.concatenate([core.call_start(desc), M.encode_frames(core.call_records(desc, pay)).reshape(-1), core.call_end(desc, n)])
        assert np.array_equal(tx[s], want), s
        if s in GOLDEN_NAMES:      # the recorded calls: the start, the LICH round robin and the end are the reference's own bytes (its payloads differ)
            _, gdesc, _, start, frames, end = M.tx_call(G, GOLDEN_NAMES[s])
            assert np.array_equal(gdesc, desc) and frames.shape[0] == n
            assert np.array_equal(tx[s][:96], start)
            got = M.decode_records(np.stack([M.fs_record(f) for f in tx[s][96:96 + 48 * n].reshape(n, 48)]))
            ref = M.decode_records(np.stack([M.fs_record(f) for f in frames]))
            assert np.array_equal(got[:, 2:4], ref[:, 2:4]) and np.array_equal(got[:, 32:38], ref[:, 32:38]) and np.array_equal(got[:, 4:20], pay)
            assert np.array_equal(tx[s][96 + 48 * n:], end)


def test_link_events_over_the_air_equal_the_core_and_give_the_call_back(on, core):
    frames, tx, ev, get = on
    for s, (src, dst, can, dtype, n) in enumerate(CALLS):
        assert frames[s] == ev[s].shape[0] == n + 3, (s, [int(t) for t in ev[s][:, 2]])      # the LSF, n frames, the last frame, the EOT
        # what went over the air, cut into the synchroniser's records, through the scalar core: CAN 5 only, decode_all_can off
        recs = [M.fs_record(tx[s][48:96])] + [M.fs_record(f) for f in tx[s][96:96 + 48 * (n + 1)].reshape(n + 1, 48)] + [M.fs_record(ftype=M.FT_EOT)]
        want, _ = core.run(np.stack(recs), 5, 0)
        assert np.array_equal(ev[s], want), s
        fl = M.flags(ev[s])
        assert list(np.nonzero(fl & M.INFO)[0]) == [0, n + 2] and [int(t) for t in ev[s][:, 2]] == [1] + [2] * (n + 1) + [0xFF]
        heard = can == 5
        assert bool((fl[1:n + 2] & M.AUDIO).all()) == heard and bool((fl & M.AUDIO).any()) == heard and bool(fl[n + 2] & M.END) == heard
        if heard:
            assert np.array_equal(ev[s][1:n + 1, 48:64], _payloads(s, n)) and not ev[s][n + 1, 48:64].any()
        name = dst or {0: "BROADCAST", 2: "ECHO", 4: "UNLINK"}[dtype]
        assert M.texts(ev[s][0]) == (src, name) and ev[s][0, 3] == can
        # the reader of host/m17_link_hip.h
        for i, g in enumerate(get[s]):
            r = ev[s][i]
            bits = [int(x) for x in g[:8]]
            assert bits == [(int(fl[i]) >> b) & 1 for b in range(8)]
            assert [int(x) for x in g[8:14]] == [int(r[2]), int(r[3]), (int(r[4]) | int(r[5]) << 8) & 0x7FFF, int(r[5]) >> 7, int(r[6]), int(r[7])]
            assert g[14] == bytes(r[8:14]).hex() and g[15] == bytes(r[14:20]).hex()
            assert (g[16], g[17]) == tuple(t or "-" for t in M.texts(r)) and g[18] == bytes(r[48:64]).hex()


def test_off_by_default_no_event_fires(tmp_path):
    frames, tx, ev, _ = _run(tmp_path, False, 0, True)
    assert frames == [n + 3 for *_, n in CALLS] and all(e.shape[0] == 0 for e in ev)
