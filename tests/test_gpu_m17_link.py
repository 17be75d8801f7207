"""M17 link layer on the GPU (k_m17_link_decode + k_m17_rx through qrl_m17_rx_process, k_m17_call through qrl_m17_call_*): the reference's
recorded records, states and transmitted bytes (tests/golden/ref/m17_link.npz) are the expected values, byte for byte; the reference itself
is not read here.  Then the chains: bits -> FrameSync -> link layer with no host copy between the stages, and the loopback of a whole
transmission."""
import ctypes as C

import numpy as np
import pytest

import m17_link as M

pytestmark = pytest.mark.gpu
G = M.load_golden()
NAMES = list(G["names"])
PLAIN = [NAMES[k] for k in M.plain(G)]
# a handle has one configuration; with decode_all_can set the CAN to receive does not matter, so those scenarios share a handle
ALL_CAN = [n for n in PLAIN if G["config"][NAMES.index(n), 1] == 1]
CAP = 12
ERR_ARG = -1


def _rows(inp):
    """[B, n, 56] records -> the [B, 56 n] rows a frame synchroniser writes"""
    return np.ascontiguousarray(inp).reshape(inp.shape[0], -1)


def _process(rx, inp, counts, stream=None):
    """inp [B, n, 56], counts [B] frames -> records [B, n, 64]"""
    import torch
    d_in = torch.from_numpy(_rows(inp)).cuda()
    c = np.zeros((inp.shape[0], 2), np.int32)
    c[:, 0], c[:, 1] = np.asarray(counts) * M.FS_REC, counts
    out = rx.process(d_in, torch.from_numpy(c).cuda(), cap_frames=inp.shape[1], stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_same(got, want, what=""):
    bad = np.nonzero((got != want).any(axis=-1))
    assert not len(bad[0]), "%s: records %s differ; first: device %s, reference %s" % (
        what, list(zip(*bad))[:6], got[tuple(a[0] for a in bad)].tobytes().hex(), want[tuple(a[0] for a in bad)].tobytes().hex())


FRESH_PUBLIC = np.frombuffer(b"\0\0\0\0" + bytes(6) + b"\xff" * 6, np.uint8)


def _streams(batch=66):
    """66 streams (a wave and two): the decode_all_can scenarios in turn, every stream another count, 0 and counts above CAP among them
    -> (names, inputs [B, CAP, 56], counts as given to the device [B], expected [B, CAP, 64], expected public state [B, 16])"""
    names = [ALL_CAN[(5 * b + b // len(ALL_CAN)) % len(ALL_CAN)] for b in range(batch)]
    assert len(set(names)) == len(ALL_CAN) >= 15 and all(a != b for a, b in zip(names[:-1], names[1:]))
    idx = [NAMES.index(n) for n in names]
    full = G["counts"][idx].astype(np.int64)
    b = np.arange(batch)
    counts = np.maximum(full - (2 * (b // len(ALL_CAN)) + b % 2), 0)      # the n-th time a scenario comes round it is cut 2 n or 2 n + 1 frames short
    counts[::11] = 0
    assert (counts == 0).any() and (counts > CAP).any() and len(set(zip(names, counts))) == batch
    inp, want, pub = G["inputs"][idx, :CAP].copy(), G["expected"][idx, :CAP].copy(), np.zeros((batch, M.STATE_PUBLIC), np.uint8)
    for b, c in enumerate(counts):
        used = int(min(c, CAP))
        want[b, used:] = 0
        pub[b] = M.public_state(G["states"][idx[b], used - 1]) if used else FRESH_PUBLIC
    return names, inp, counts.astype(np.int32), want, pub


@pytest.mark.parametrize("name", PLAIN)
def test_every_scenario_at_batch_1(qrl_ctx, name):
    import qradiolink_amd as q
    _, inp, want, states, can_rx, all_can, _ = M.scenario(G, name)
    rx = q.M17Rx(qrl_ctx, 1, can_rx=can_rx, decode_all_can=bool(all_can))
    got = _process(rx, inp[None], [inp.shape[0]])
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got[0], want, name)
    assert np.array_equal(state[0], M.public_state(states[-1]))


def test_distinct_streams_with_ragged_counts(qrl_ctx):
    import qradiolink_amd as q
    names, inp, counts, want, pub = _streams()
    rx = q.M17Rx(qrl_ctx, len(names), can_rx=0, decode_all_can=True)
    assert np.array_equal(rx.state().cpu().numpy(), np.tile(FRESH_PUBLIC, (len(names), 1)))
    got = _process(rx, inp, counts)
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got, want, "66 streams")
    assert np.array_equal(state, pub)


@pytest.mark.parametrize("step", [1, 2, 5])
def test_ragged_calls_equal_the_single_call(qrl_ctx, step):
    """the same streams cut into calls of `step` frames: a LICH round, a lock and an EOT each straddle a call boundary somewhere"""
    import qradiolink_amd as q
    names, inp, counts, want, pub = _streams()
    rx = q.M17Rx(qrl_ctx, len(names), can_rx=0, decode_all_can=True)
    got = np.zeros_like(want)
    for a in range(0, CAP, step):
        b = min(a + step, CAP)
        got[:, a:b] = _process(rx, inp[:, a:b], np.clip(counts - a, 0, b - a))
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got, want, "calls of %d" % step)
    assert np.array_equal(state, pub)


def test_reset_in_mid_round_gives_a_fresh_handle_s_output(qrl_ctx):
    import qradiolink_amd as q
    names, inp, counts, want, pub = _streams()
    rx = q.M17Rx(qrl_ctx, len(names), can_rx=0, decode_all_can=True)
    _process(rx, inp[:, :4], np.minimum(counts, 4))           # LSFs, locks and half a LICH round in the state
    assert not np.array_equal(rx.state().cpu().numpy(), np.tile(FRESH_PUBLIC, (len(names), 1)))
    rx.reset()
    assert np.array_equal(rx.state().cpu().numpy(), np.tile(FRESH_PUBLIC, (len(names), 1)))
    got = _process(rx, inp, counts)
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got, want, "after reset")
    assert np.array_equal(state, pub)


def test_set_config_between_calls_takes_effect(qrl_ctx):
    import qradiolink_amd as q
    _, inp, want, states, can_rx, all_can, reconfig = M.scenario(G, "reconfigured")
    rx = q.M17Rx(qrl_ctx, 3, can_rx=can_rx, decode_all_can=bool(all_can))
    cuts = [0] + [slot for slot, _, _ in reconfig] + [inp.shape[0]]
    got = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k:
            rx.set_config(reconfig[k - 1][1], bool(reconfig[k - 1][2]))
        got.append(_process(rx, np.stack([inp[a:b]] * 3), [b - a, 0, b - a]))
    got = np.concatenate(got, axis=1)
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got[0], want, "reconfigured")
    _assert_same(got[2], want, "reconfigured, stream 2")
    assert not got[1].any() and np.array_equal(state[1], FRESH_PUBLIC) and np.array_equal(state[0], M.public_state(states[-1]))


def _bits_of(inp):
    """the bits that make the frame synchroniser cut these records: sync word (two bytes, four for the EOT), 46 bytes, a few idle bits"""
    out = []
    for rec in inp:
        ftype = int(rec[:4].copy().view("<u4")[0])
        word = ftype.to_bytes(4, "big") if ftype == M.FT_EOT else ftype.to_bytes(2, "big")
        out.append(np.unpackbits(np.concatenate([np.frombuffer(word, np.uint8), rec[8:54]])))
        out.append(np.zeros(24, np.uint8))
    return np.concatenate(out)


def test_chained_behind_the_frame_synchroniser(qrl_ctx):
    """bits in, events out: FrameSync.process with enable_m17_link queues the link layer on the synchroniser's stream; three calls so that
    frames and LICH rounds straddle them"""
    import torch
    import qradiolink_amd as q
    names = [n for n in ALL_CAN if n != "passed_over"][:9]
    scen = [M.scenario(G, n) for n in names]
    bits = [_bits_of(s[1]) for s in scen]
    n = max(len(b) for b in bits)
    x = np.zeros((len(names), n), np.uint8)
    for b, v in enumerate(bits):
        x[b, :len(v)] = v
    fs = q.FrameSync(qrl_ctx, q.MODEM_M17, len(names))
    fs.enable_m17_link(can_rx=0, decode_all_can=True)
    got = [[] for _ in names]
    third = (n // 3 + 7) & ~7
    for a in range(0, n, third):
        chunk = torch.from_numpy(np.ascontiguousarray(x[:, a:a + third])).cuda()
        _, cnt = fs.process(chunk)
        cnt, ev = cnt.cpu().numpy(), fs.m17_events.cpu().numpy()
        for b in range(len(names)):
            got[b].append(ev[b, :cnt[b, 1]])
            assert not ev[b, cnt[b, 1]:].any()
    state = fs.m17_rx.state().cpu().numpy()
    fs.close()
    for b, s in enumerate(scen):
        _assert_same(np.concatenate(got[b]), s[2], names[b])
        assert np.array_equal(state[b], M.public_state(s[3][-1]))


# ------------------------------------------------------------------------------------------------------------------ transmit
def test_transmit_equals_the_reference_s_bytes(qrl_ctx):
    import torch
    import qradiolink_amd as q
    tx = list(G["tx_names"])
    calls = torch.from_numpy(np.ascontiguousarray(G["tx_desc"])).cuda()
    assert np.array_equal(q.m17_call_start(qrl_ctx, calls).cpu().numpy(), G["tx_start"])
    ends = torch.from_numpy(G["tx_n"].astype(np.int32)).cuda()
    assert np.array_equal(q.m17_call_end(qrl_ctx, calls, ends).cpu().numpy(), G["tx_end"])
    # every call's first frames in one batch (first NULL), padded with zero payloads where a call is shorter
    n = 7
    pay = np.zeros((len(tx), n, 16), np.uint8)
    for t, name in enumerate(tx):
        p = M.tx_call(G, name)[2][:n]
        pay[t, :p.shape[0]] = p
    out = q.m17_call_encode(qrl_ctx, calls, torch.from_numpy(pay).cuda(), slot_bytes=51).cpu().numpy()
    for t, name in enumerate(tx):
        frames = M.tx_call(G, name)[4][:n]
        assert np.array_equal(out[t, :frames.shape[0], :48], frames), name
    assert not out[:, :, 48:].any()


def test_transmit_long_call_whole_and_cut(qrl_ctx):
    """2 050 frames, so the frame number wraps; then the same call cut at first = 0, 1, 5, 6, 7, 2047 and 2048 as seven streams of one batch"""
    import torch
    import qradiolink_amd as q
    _, desc, pay, _, frames, _ = M.tx_call(G, "long_call")
    one = torch.from_numpy(desc[None].copy()).cuda()
    out = q.m17_call_encode(qrl_ctx, one, torch.from_numpy(pay[None].copy()).cuda()).cpu().numpy()
    assert np.array_equal(out[0], frames)
    firsts = np.array([0, 1, 5, 6, 7, 2047, 2048], np.int32)
    seven = torch.from_numpy(np.tile(desc, (7, 1))).cuda()
    p = np.stack([pay[f:f + 2] for f in firsts])
    out = q.m17_call_encode(qrl_ctx, seven, torch.from_numpy(p).cuda(), first=torch.from_numpy(firsts).cuda()).cpu().numpy()
    for b, f in enumerate(firsts):
        assert np.array_equal(out[b], frames[f:f + 2]), f
    ends = q.m17_call_end(qrl_ctx, seven, torch.from_numpy(firsts).cuda()).cpu().numpy()
    assert all(bytes(e[48:]) == b"\x55\x5d" * 8 for e in ends) and len({bytes(e[:48]) for e in ends}) == 7


def test_loopback_of_a_whole_transmission(qrl_ctx):
    """m17_call_bytes -> unpacked bits -> FrameSync -> link layer: the payloads and the callsigns come back; per stream m17FrameInfoReceived
    fires once when the LSF locks the decoder and once with the EOT, as the reference's does, and the transmission ends once"""
    import torch
    import qradiolink_amd as q
    calls = [("YO8RZZ", "AB1CDE", 0, 0, 9), ("N0CALL-9", "", 7, 0, 14), ("DL1ABC", "", 15, 2, 6)]
    rng = np.random.RandomState(3)
    pays = [rng.randint(0, 256, (n, 16)).astype(np.uint8) for *_, n in calls]
    rows = [np.unpackbits(q.m17_call_bytes(qrl_ctx, q.m17_call_descriptor(s, d, c, t), p)) for (s, d, c, t, _), p in zip(calls, pays)]
    for r, (*_, n) in zip(rows, calls):
        assert r.size == 8 * (96 + 48 * n + 64)
    width = max(r.size for r in rows) + 512              # the EOT word opens a 46-byte frame: idle bits behind the sixteen EOT bytes
    x = np.zeros((len(calls), width), np.uint8)
    for b, r in enumerate(rows):
        x[b, :r.size] = r
    fs = q.FrameSync(qrl_ctx, q.MODEM_M17, len(calls))
    fs.enable_m17_link(can_rx=0, decode_all_can=True)
    _, cnt = fs.process(torch.from_numpy(x).cuda())
    cnt, ev = cnt.cpu().numpy(), fs.m17_events.cpu().numpy()
    fs.close()
    for b, ((src, dst, can, dtype, n), p) in enumerate(zip(calls, pays)):
        rec = ev[b, :cnt[b, 1]]
        fl = M.flags(rec)
        assert cnt[b, 1] == n + 3                                  # the LSF, n frames, the last frame, the EOT (the preamble is no frame)
        assert [int(t) for t in rec[:, 2]] == [1] + [2] * (n + 1) + [0xFF]
        assert list(np.nonzero(fl & M.INFO)[0]) == [0, n + 2] and list(np.nonzero(fl & M.END)[0]) == [n + 2]
        audio = rec[(fl & M.AUDIO) != 0]
        assert np.array_equal(audio[:n, 48:64], p) and audio.shape[0] == n + 1 and not audio[n, 48:64].any() and rec[n + 1, 5] & 0x80
        assert M.texts(rec[0])[0] == src and M.texts(rec[0])[1] == (dst or ("ECHO" if dtype == 2 else "BROADCAST")) and rec[0, 3] == can
        assert M.texts(rec[n + 2]) == M.texts(rec[0])


def test_refusals_return_before_any_launch(qrl_ctx):
    import torch
    import qradiolink_amd as q
    lib = qrl_ctx.lib
    rx = q.M17Rx(qrl_ctx, 2)
    frames = torch.zeros((2, 4 * M.FS_REC + 8), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    out = torch.full((2, 4, M.REC + 16), 0xA5, dtype=torch.uint8, device="cuda")
    f, c, o, stride = frames.data_ptr(), counts.data_ptr(), out.data_ptr(), frames.stride(0)
    assert lib.qrl_m17_rx_process(rx.h, None, f, stride, c, 4, o) == 0
    torch.cuda.synchronize()
    out.fill_(0xA5)
    for args in ((None, stride, c, 4, o), (f, stride, None, 4, o), (f, stride, c, 4, None), (f, stride, c, 0, o), (f, stride, c, 5, o),
                 (f, 4 * M.FS_REC - 4, c, 4, o), (f + 1, stride, c, 4, o), (f, stride, c, 4, o + 8)):
        assert lib.qrl_m17_rx_process(rx.h, None, *args) == ERR_ARG, args
    assert lib.qrl_m17_rx_get_state(rx.h, None, None) == ERR_ARG and lib.qrl_m17_rx_get_state(rx.h, None, o + 4) == ERR_ARG
    for cfg in ((16, 0), (-1, 1), (0, 2)):
        assert lib.qrl_m17_rx_set_config(rx.h, C.byref(q._M17RxConfig(*cfg))) == ERR_ARG
        h = C.c_void_p()
        assert lib.qrl_m17_rx_create(qrl_ctx.h, 2, C.byref(q._M17RxConfig(*cfg)), C.byref(h)) == ERR_ARG and not h.value
    calls = torch.zeros((2, M.CALL_BYTES), dtype=torch.uint8, device="cuda")
    pay = torch.zeros((2, 3, 16), dtype=torch.uint8, device="cuda")
    first = torch.zeros((2,), dtype=torch.int32, device="cuda")
    k, p, fi = calls.data_ptr(), pay.data_ptr(), first.data_ptr()
    assert lib.qrl_m17_call_start(qrl_ctx.h, None, k, 2, o, 95) == ERR_ARG and lib.qrl_m17_call_start(qrl_ctx.h, None, k, 0, o, 96) == ERR_ARG
    assert lib.qrl_m17_call_start(qrl_ctx.h, None, None, 2, o, 96) == ERR_ARG
    for args in ((None, p, fi, 2, 3, o, 144, 48), (k, None, fi, 2, 3, o, 144, 48), (k, p, fi, 2, 3, None, 144, 48), (k, p, fi, 0, 3, o, 144, 48),
                 (k, p, fi, 2, 0, o, 144, 48), (k, p, fi, 2, 3, o, 144, 47), (k, p, fi, 2, 3, o, 143, 48)):
        assert lib.qrl_m17_call_encode(qrl_ctx.h, None, *args) == ERR_ARG, args
    assert lib.qrl_m17_call_end(qrl_ctx.h, None, k, None, 2, o, 64) == ERR_ARG and lib.qrl_m17_call_end(qrl_ctx.h, None, k, fi, 2, o, 63) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                # nothing was launched on the refused calls
    rx.close()
