"""The DMR receive call layer through the C++ facade (tests/host/test_dmr_rx_facade.cpp): with set_dmr_call on, gr_modem_hip::demodulate hands
every burst of the dmrFrames callback to dmrCallEvents as well, as the 128-byte record the scalar core (which tests/test_dmr_rx.py holds to
the reference) gives for the same bursts with the state carried across the work() calls; host/dmr_frame_hip.h reads that record and turns the
alias into the text of the reference's talkerAlias signal; off (the default) dmrFrames and dmrFramesDecoded are what they were."""
import os
import subprocess

import numpy as np
import pytest

import dmr_l2
import dmr_rx

pytestmark = pytest.mark.gpu

ROOT = dmr_rx.ROOT
EXE = os.path.join(ROOT, "tests", "host", "test_dmr_rx_facade")
G = dmr_rx.load_golden()


def _exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "qradiolink_amd", "csrc"), "dmr_rx_facade"])
    return EXE


@pytest.fixture(scope="module")
def air(tmp_path_factory, qrl_ctx):
    """the bursts of the golden whole call, and of the late entry, in 72-byte slots through the DMR modulator at 1 Msps"""
    import torch
    import qradiolink_amd as q
    d = tmp_path_factory.mktemp("dmr_rx_facade")
    names = ["whole_call", "late_entry_promiscuous"]
    n_slots = 2 + max(int(G["counts"][list(G["names"]).index(n)]) for n in names) + 2
    rows = np.zeros((2, n_slots, 72), np.uint8)
    for s, name in enumerate(names):
        _, inp, _, _, _, _ = dmr_rx.scenario(G, name)
        rows[s, 2:2 + inp.shape[0], :33] = inp[:, 4:37]
    mod = q.Mod(qrl_ctx, q.MODEM_DMR, batch=2, max_bytes=n_slots * 72)
    iq = (mod.process(torch.from_numpy(rows.reshape(2, -1)).cuda()) * 0.05).cpu().numpy().astype(np.complex64)
    mod.close()
    n = iq.shape[1] & ~1
    np.ascontiguousarray(iq[:, :n]).tofile(str(d / "iq.bin"))
    return d, n


def _run(air, call, cc=1, prom=1):
    d, n = air
    pre = str(d / ("out%d" % call))
    r = subprocess.run([_exe(), "2", str(n), str(d / "iq.bin"), pre, str(call), str(cc), str(prom)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [(np.fromfile("%s.raw.%d.bin" % (pre, s), np.uint8).reshape(-1, 40), np.fromfile("%s.l2.%d.bin" % (pre, s), np.uint8).reshape(-1, 80),
             np.fromfile("%s.call.%d.bin" % (pre, s), np.uint8).reshape(-1, 128), [line.split() for line in open("%s.get.%d.txt" % (pre, s))]) for s in range(2)]


def test_call_events_arrive_beside_the_frames(air, tmp_path):
    core = dmr_rx.load_core(tmp_path)
    off, on = _run(air, 0), _run(air, 1)
    for s in range(2):
        raw, l2, rec, getters = on[s]
        assert np.array_equal(raw, off[s][0]) and np.array_equal(l2, off[s][1]) and off[s][2].size == 0      # default off: the two callbacks are what they were
        assert raw.shape[0] == l2.shape[0] == rec.shape[0] >= 12 and np.array_equal(l2, dmr_l2.records(raw, 1))
        want, _, _, _ = core.run(raw, 1, 1)
        assert np.array_equal(rec, want), "stream %d: records %s differ from the core's" % (s, np.nonzero((rec != want).any(axis=1))[0][:8])
        f = dmr_rx.flags(rec)
        for r, fl, g in zip(rec, f, getters):
            assert [int(v) for v in g[:17]] == [(int(fl) >> i) & 1 for i in range(11)] + [r[2], r[3], r[4], dmr_rx.ids(r)[0], dmr_rx.ids(r)[1], r[16]]
            assert g[17] == bytes(r[17:26]).hex() and [int(g[18]), int(g[19])] == [r[26], r[27]]
            assert g[20] == (bytes(r[32:32 + r[28]]).hex() or "-")
    # stream 0, the whole call: header, the call's LC, the alias as text, audio on every voice burst the receiver delivered
    raw, l2, rec, getters = on[0]
    f = dmr_rx.flags(rec)
    assert f[0] & dmr_rx.HEADER_VOICE and dmr_rx.ids(rec[0]) == (dmr_rx.A, dmr_rx.B_)
    voice = l2[:, 0] != 0
    assert voice.sum() >= 30 and ((f[voice] & dmr_rx.AUDIO) != 0).all()
    alias = [g for g in getters if int(g[8])]
    assert len(alias) == 1 and bytes.fromhex(alias[0][21]) == dmr_rx.TEXT and bytes.fromhex(alias[0][20]) == dmr_rx.TEXT
    assert (f & dmr_rx.TERMINATOR).any() and rec[-1, 2] == dmr_rx.IDLE
    # stream 1, late entry, promiscuous: no header, both embedded LCs
    raw, l2, rec, getters = on[1]
    f = dmr_rx.flags(rec)
    assert not (f & dmr_rx.HEADER_VOICE).any() and rec[0, 2] == dmr_rx.LATE_ENTRY
    assert [dmr_rx.ids(r) for r in rec[(f & dmr_rx.EMBEDDED) != 0]] == [(1234567, 7654321), (dmr_rx.A, dmr_rx.B_)]


def test_a_fixed_colour_code_refuses_the_late_entry(air):
    """the same air with colour code 1 fixed: the whole call is as before, the late entry is refused burst by burst"""
    on = _run(air, 1, cc=1, prom=0)
    f0, f1 = dmr_rx.flags(on[0][2]), dmr_rx.flags(on[1][2])
    assert f0[0] & dmr_rx.HEADER_VOICE and (f0 & dmr_rx.TALKER_ALIAS).any()
    voice = on[1][1][:, 0] != 0
    assert voice.any() and (f1[voice] == dmr_rx.VALID).all() and (on[1][2][:, 2] == dmr_rx.IDLE).all()
