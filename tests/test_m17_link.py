"""M17 link layer on the CPU: qradiolink_amd/csrc/m17_link_core.hpp, the code k_m17_rx and k_m17_call call, against the recorded records of
tests/golden/ref/m17_link.npz byte for byte, and against the live reference where it is present (its gr_modem, M17FrameDecoder and
M17Transmitter, compiled unmodified: tests/host/m17_link_ref.cpp).  The per-frame FEC in front of the core (receive) and behind it
(transmit) is the oracle's, which tests/test_framefec.py pins against the reference's own decoder and encoder.  And the same core under the
address and undefined-behaviour sanitizers, as a program of its own (tests/host/test_m17_link_core.cpp)."""
import numpy as np
import pytest

import m17_link as M

G = M.load_golden()
NAMES = list(G["names"])
TX_NAMES = list(G["tx_names"])


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return M.load_core(tmp_path_factory.mktemp("m17_link_core"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    r = M.load_ref(tmp_path_factory.mktemp("m17_link_ref"))
    if r is None:
        pytest.skip("the reference's sources are not here")
    return r


def _run_core(core, name, step=None):
    """a scenario through the core in calls of `step` frames (None: one call per configuration) -> (records, the state after every call's last
    frame as {frame index: state})"""
    _, inp, _, _, can_rx, all_can, reconfig = M.scenario(G, name)
    cuts = sorted({0, inp.shape[0]} | {slot for slot, _, _ in reconfig} | (set(range(0, inp.shape[0], step)) if step else set()))
    cfg_at = {0: (can_rx, all_can)}
    cfg_at.update({slot: (c, a) for slot, c, a in reconfig})
    out, state, cfg, states = [], None, None, {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        cfg = cfg_at.get(a, cfg)
        o, state = core.run(inp[a:b], cfg[0], cfg[1], state)
        out.append(o)
        states[b - 1] = bytes(state)
    return np.concatenate(out), states


def _state64(state62):
    """the reference's recorded state in the layout of m17_rx_state"""
    s = bytes(state62)
    return s[0:30] + s[60:62] + s[30:60] + b"\0\0"


@pytest.mark.parametrize("name", NAMES)
def test_core_equals_the_golden(core, name):
    _, _, want, states, _, _, _ = M.scenario(G, name)
    got, last = _run_core(core, name)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), "frames %s differ; first: core %s, reference %s" % (bad[:8], got[bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex())
    end = want.shape[0] - 1
    assert last[end] == _state64(states[end])
    assert np.array_equal(core.public(last[end]), M.public_state(states[end]))


@pytest.mark.parametrize("step", [1, 2, 5])
def test_core_cut_into_calls_equals_the_uncut_run_and_the_reference_state(core, step):
    """the state carried through its 64 bytes from call to call; after every call it is the reference's lsf, lsfFromLich, map and lock"""
    for name in NAMES:
        _, _, want, states, _, _, _ = M.scenario(G, name)
        got, seen = _run_core(core, name, step)
        assert np.array_equal(got, want), name
        for i, st in seen.items():
            assert st == _state64(states[i]), (name, i)
            assert np.array_equal(core.public(st), M.public_state(states[i])), (name, i)


def test_fresh_state_is_the_decoder_after_reset(core):
    st = bytes(core.fresh())
    assert st[0:6] == b"\xff" * 6 and st[6:32] == bytes(26) and st[32:38] == b"\xff" * 6 and st[38:64] == bytes(26)
    assert bytes(core.public(st)) == b"\0\0\0\0" + bytes(6) + b"\xff" * 6


def test_golden_is_fresh(ref):
    g = M.record_golden(ref)
    assert sorted(g) == sorted(G)
    for k in g:
        assert np.array_equal(g[k], G[k]), k


def test_core_equals_the_live_reference_on_shuffled_streams(core, ref):
    """frames of the golden scenarios in an order no scenario has: every fifth frame dropped, pairs swapped, reversed, both CAN rules"""
    for name in ("lsf_then_stream", "late_entry_phase_3", "lich_golay_uncorrectable", "lich_round_bad_crc", "segment_6", "two_calls", "destinations"):
        _, inp, _, _, can_rx, all_can, _ = M.scenario(G, name)
        for mode in (0, 1):
            keep = [i for i in range(inp.shape[0]) if i % 5 != 4]
            x = inp[keep].copy()
            m = (x.shape[0] - 3) // 4 * 4
            x[1:m + 1:4], x[2:m + 2:4] = x[2:m + 2:4].copy(), x[1:m + 1:4].copy()
            if mode:
                x = x[::-1].copy()
            got, state = core.run(x, can_rx, all_can ^ mode)
            want, states = ref.run(x, can_rx, all_can ^ mode)
            assert np.array_equal(got, want), (name, mode)
            assert bytes(state) == _state64(states[-1]), (name, mode)


def test_callsign_text_equals_the_live_reference_on_random_addresses(core, ref):
    """decode_callsign / getDestination over random 48-bit addresses, the largest values and the bytes the special names compare"""
    rng = np.random.RandomState(17)
    special = [bytes([a, b]) + tail for a, b in ((0, 0), (0x9C, 0x01)) for tail in (b"\x7d\xd8\x0e\x00", b"\xb9\xcd\x0e\x00", b"\x45\x77\x4f\x45", b"\xff" * 4)]
    values = [bytes(rng.randint(0, 256, 6).astype(np.uint8)) for _ in range(60)] + [M.call6(value=v) for v in (0, 1, 39, 40, 40 ** 9 - 1, 40 ** 9, 2 ** 48 - 1)]
    frames = [M.fs_record(M.lsf_frame(M.make_lsf(src, dst, can=i & 15))) for i, (src, dst) in enumerate(zip(values, (special + values)[:len(values)]))]
    x = np.stack(frames)
    got, _ = core.run(x, 0, 1)
    want, _ = ref.run(x, 0, 1)
    assert np.array_equal(got, want)
    assert all(M.flags(want) & M.INFO) and {len(M.texts(r)[0]) for r in want} >= {0, 1, 9, 10}


# ------------------------------------------------------------------------------------------------------------------ transmit
@pytest.mark.parametrize("name", TX_NAMES)
def test_transmit_core_equals_the_golden(core, name):
    _, desc, pay, start, frames, end = M.tx_call(G, name)
    assert np.array_equal(core.call_start(desc), start)
    n = pay.shape[0]
    sel = np.arange(n) if n <= 64 else np.concatenate([np.arange(20), np.arange(2040, n)])      # the wrap of the long call
    for i in sel:
        assert np.array_equal(M.encode_frames(core.call_records(desc, pay[i:i + 1], first=int(i)))[0], frames[i]), (name, i)
    assert np.array_equal(core.call_end(desc, n), end)


def test_transmit_call_end_at_several_indices(core):
    """the last frame of a call is stream frame `first` with a zero payload and the EOS bit: the calls of the golden end at 0, 1, 2, 3, 5, 6, 7, 2050"""
    ends = sorted({int(n) for n in G["tx_n"]})
    assert ends[:7] == [0, 1, 2, 3, 5, 6, 7] and ends[-1] == 2050
    _, desc, pay, _, frames, _ = M.tx_call(G, "long_call")
    for k in (0, 5, 6, 2047, 2048):
        last = core.call_end(desc, k)
        rec = M.decode_records(M.fs_record(last[:48])[None])[0]
        same = M.decode_records(M.fs_record(frames[k])[None])[0]
        assert rec[2] == (same[2] | 0x80) and rec[3] == same[3] and not rec[4:20].any() and bytes(rec[32:38]) == bytes(same[32:38])
        assert bytes(last[48:]) == b"\x55\x5d" * 8


def test_transmit_is_a_function_of_the_frame_index(core):
    """the long call cut at first = 0, 1, 5, 6, 7, 2047 and 2048 equals the uncut bytes"""
    _, desc, pay, _, frames, _ = M.tx_call(G, "long_call")
    for first in (0, 1, 5, 6, 7, 2047, 2048):
        n = min(4, pay.shape[0] - first)
        got = M.encode_frames(core.call_records(desc, pay[first:first + n], first=first))
        assert np.array_equal(got, frames[first:first + n]), first


def test_transmit_equals_the_live_reference_on_other_calls(core, ref):
    for t, (src, dst, can, dtype, n) in enumerate((("M17", "ECHO", 1, 0, 13), ("zz9", "", 14, 3, 8), ("LONGCALLSIGN", "A", 3, 0, 1), ("", "Q", 3, 7, 2))):
        pay = M.tx_payloads(40 + t, n)
        start, frames, end = ref.call(src.encode(), dst.encode(), can, dtype, pay)
        desc = M.descriptor(src, dst, can, dtype)
        assert np.array_equal(core.call_start(desc), start)
        assert np.array_equal(M.encode_frames(core.call_records(desc, pay)).reshape(-1), frames)
        assert np.array_equal(core.call_end(desc, n), end)


def test_reference_transmission_received_by_the_core(core):
    """the recorded bytes of a call, cut into frames as the synchroniser would, give back the payloads, the callsigns, one INFO and one END"""
    _, desc, pay, start, frames, end = M.tx_call(G, "type_0")
    recs = [M.fs_record(start[48:])] + [M.fs_record(f) for f in frames] + [M.fs_record(end[:48]), M.fs_record(ftype=M.FT_EOT)]
    out, _ = core.run(np.stack(recs), 0, 0)
    fl = M.flags(out)
    assert int(((fl & M.INFO) != 0).sum()) == 2 and (fl[0] & M.INFO) and (fl[-1] & M.INFO) and int(((fl & M.END) != 0).sum()) == 1
    audio = out[(fl & M.AUDIO) != 0]
    assert np.array_equal(audio[:-1, 48:64], pay) and not audio[-1, 48:64].any()
    assert M.texts(out[0]) == ("YO8RZZ", "AB1CDE") and out[-2, 5] & 0x80


# ------------------------------------------------------------------------------------------------------------------ the core under the sanitizers
def _flat_file(path, core):
    """the golden's one-configuration scenarios with the oracle's decode records, and call records of every transmit call (the oracle's decode of
    the reference's own frames: the record the core has to build)"""
    import struct
    with open(path, "wb") as f:
        plain = M.plain(G)
        f.write(struct.pack("<I", len(plain)))
        for k in plain:
            _, inp, want, _, can_rx, all_can, _ = M.scenario(G, NAMES[k])
            f.write(struct.pack("<Iii", inp.shape[0], can_rx, all_can) + inp.tobytes() + M.decode_records(inp).tobytes() + want.tobytes())
        calls = []
        for name in TX_NAMES:
            _, desc, pay, start, frames, end = M.tx_call(G, name)
            n = pay.shape[0]
            calls.append((desc, 0, bytes(16), 0, M.decode_records(M.fs_record(start[48:])[None])[0]))
            for i in list(range(min(n, 8))) + ([2047, 2048] if n > 2048 else []):
                calls.append((desc, i, pay[i].tobytes(), 1, M.decode_records(M.fs_record(frames[i])[None])[0]))
            calls.append((desc, n, bytes(16), 2, M.decode_records(M.fs_record(end[:48])[None])[0]))
        f.write(struct.pack("<I", len(calls)))
        for desc, k, pay, kind, rec in calls:
            rec = rec.copy()
            if kind == 0:
                rec[1] = 0                      # an LSF record carries no LICH fields
            f.write(desc.tobytes() + struct.pack("<I", k) + pay + struct.pack("<i", kind) + rec.tobytes())
    return len(plain), sum(int(G["counts"][k]) for k in plain), len(calls)


def test_core_header_equals_the_golden_under_the_sanitizers(core, tmp_path):
    import os
    import subprocess
    exe, data = str(tmp_path / "test_m17_link_core"), str(tmp_path / "golden.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(M.ROOT, "tests", "host", "test_m17_link_core.cpp"), "-o", exe])
    s, n, c = _flat_file(data, core)
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d scenarios, %d frames, %d call records" % (s, n, c)), r.stdout
