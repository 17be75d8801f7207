"""DMR receive call layer on the GPU (k_dmr_rx through qrl_dmr_rx_process, behind qrl_dmr_l2_decode): the reference's recorded call
records (tests/golden/ref/dmr_rx.npz) are the expected values, byte for byte; the reference itself is not read here.  Then the whole device
chain: qrl_dmr_voice_call_encode -> DMR modulator -> DMR receiver -> DMO slicer -> layer 2 -> tracker through Demod.enable_dmo_call."""
import ctypes as C

import numpy as np
import pytest

import dmr_rx
import dmr_tx

pytestmark = pytest.mark.gpu
G = dmr_rx.load_golden()
NAMES = list(G["names"])
PLAIN = [NAMES[k] for k in dmr_rx.plain(G)]
# a handle has one configuration: the scenarios recorded with colour code 1 fixed, and those recorded promiscuous (any colour code then)
GROUPS = {"fixed": [n for n in PLAIN if tuple(G["config"][NAMES.index(n)]) == (1, 0)], "promiscuous": [n for n in PLAIN if G["config"][NAMES.index(n), 1] == 1]}
GUARD, FILL = 256, 0xA5


def _batch(names, counts=None):
    """streams = the named scenarios -> (inputs [B, cap, 40], counts [B], expected [B, cap, 128]); counts cut a stream short: the records
    of a prefix are the prefix of the records"""
    idx = [NAMES.index(n) for n in names]
    full = G["counts"][idx].astype(np.int64)
    counts = full if counts is None else np.minimum(np.asarray(counts, np.int64), full)
    cap = max(int(counts.max()), 1)
    inp, want = G["inputs"][idx, :cap].copy(), G["expected"][idx, :cap].copy()
    for b, c in enumerate(counts):
        want[b, int(c):] = 0
    return inp, counts.astype(np.int32), want


def _process(ctx, rx, inp, counts, stream=None):
    import torch
    import qradiolink_amd as q
    d_in = torch.from_numpy(np.ascontiguousarray(inp)).cuda()
    d_cnt = torch.from_numpy(np.asarray(counts, np.int32)).cuda() if counts is not None else None
    l2 = q.dmr_l2_decode(ctx, d_in, d_cnt, audio_fec=bool(dmr_rx.AUDIO_FEC))
    out = rx.process(l2, d_cnt, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_same(got, want, what=""):
    bad = np.nonzero((got != want).any(axis=-1))
    assert not len(bad[0]), "%s: records %s differ; first: device %s, reference %s" % (
        what, list(zip(*bad))[:6], got[tuple(a[0] for a in bad)][:36], want[tuple(a[0] for a in bad)][:36])


def _public(rec):
    """the 12 public state bytes that follow from a call record"""
    return bytes(rec[2:5]) + b"\0" + bytes(rec[8:16])


@pytest.mark.parametrize("name", PLAIN)
def test_every_scenario_at_batch_1(qrl_ctx, name):
    import qradiolink_amd as q
    k, inp, want, cc, prom, _ = dmr_rx.scenario(G, name)
    rx = q.DmrRx(qrl_ctx, 1, colour_code=cc, promiscuous=bool(prom))
    got = _process(qrl_ctx, rx, inp[None], None)
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got[0], want, name)
    assert bytes(state[0]) == _public(want[-1])


@pytest.mark.parametrize("batch", [65, 72])
@pytest.mark.parametrize("group", ["fixed", "promiscuous"])
def test_scenarios_as_neighbouring_streams_with_ragged_counts(qrl_ctx, batch, group):
    """a wave and a bit: a different scenario in neighbouring lanes, every stream cut short by another amount"""
    import qradiolink_amd as q
    names = [GROUPS[group][(3 * b + b // 7) % len(GROUPS[group])] for b in range(batch)]
    assert len(set(names)) == len(GROUPS[group]) >= 5 and all(a != b for a, b in zip(names[:-1], names[1:]))
    full = np.array([G["counts"][NAMES.index(n)] for n in names])
    counts = np.maximum(full - (np.arange(batch) * 5) % 23, 0)
    counts[::9] = full[::9]
    inp, counts, want = _batch(names, counts)
    rx = q.DmrRx(qrl_ctx, batch, colour_code=7 if group == "promiscuous" else 1, promiscuous=group == "promiscuous")
    got = _process(qrl_ctx, rx, inp, counts)
    state = rx.state().cpu().numpy()
    rx.close()
    _assert_same(got, want, group)
    for b in range(batch):
        assert bytes(state[b]) == (_public(want[b, counts[b] - 1]) if counts[b] else bytes(12)), b


def test_counts_around_cap_and_nothing_written_outside(qrl_ctx):
    import torch
    import qradiolink_amd as q
    cap, counts = 10, [0, 7, 10, 25, 9]
    names = ["whole_call", "alias_corners", "terminators", "whole_call", "gps_and_unknown_flco"]
    idx = [NAMES.index(n) for n in names]
    inp, want = G["inputs"][idx, :cap].copy(), G["expected"][idx, :cap].copy()
    for b, c in enumerate(counts):
        want[b, min(c, cap):] = 0
    batch = len(names)
    d_in, d_cnt = torch.from_numpy(inp).cuda(), torch.from_numpy(np.array(counts, np.int32)).cuda()
    l2 = q.dmr_l2_decode(qrl_ctx, d_in, d_cnt)
    buf = torch.full((GUARD + batch * cap * 128 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rx = q.DmrRx(qrl_ctx, batch, colour_code=1)
    assert qrl_ctx.lib.qrl_dmr_rx_process(rx.h, None, l2.data_ptr(), d_cnt.data_ptr(), cap, buf.data_ptr() + GUARD) == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[-GUARD:] == FILL).all(), "wrote outside the output"
    _assert_same(host[GUARD:-GUARD].reshape(batch, cap, 128), want)
    # refused before any device work: null pointers, cap_frames 0, an output off the 16-byte grid
    lib = qrl_ctx.lib
    assert lib.qrl_dmr_rx_process(rx.h, None, None, d_cnt.data_ptr(), cap, buf.data_ptr() + GUARD) == -1
    assert lib.qrl_dmr_rx_process(rx.h, None, l2.data_ptr(), d_cnt.data_ptr(), cap, None) == -1
    assert lib.qrl_dmr_rx_process(rx.h, None, l2.data_ptr(), d_cnt.data_ptr(), 0, buf.data_ptr() + GUARD) == -1
    assert lib.qrl_dmr_rx_process(rx.h, None, l2.data_ptr(), d_cnt.data_ptr(), cap, buf.data_ptr() + GUARD + 4) == -1
    assert lib.qrl_dmr_rx_set_config(rx.h, C.byref(q._DmrRxConfig(16, 0))) == -1
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == host).all()
    # counts == NULL: every slot
    got = rx.process(l2)          # the state is carried: not a fresh run, so only the shape of the answer is looked at
    assert got.shape == (batch, cap, 128)
    rx.close()


@pytest.mark.parametrize("cut", [1, 3, 5])
@pytest.mark.parametrize("group", ["fixed", "promiscuous"])
def test_calls_of_a_few_slots_equal_the_uncut_run(qrl_ctx, cut, group):
    """the four fragments of an embedded LC and the blocks of an alias straddle calls; the public state after every call is the last record's"""
    import qradiolink_amd as q
    names = GROUPS[group]
    inp, counts, want = _batch(names)
    batch, n = inp.shape[0], inp.shape[1]
    rx = q.DmrRx(qrl_ctx, batch, colour_code=1, promiscuous=group == "promiscuous")
    got = np.zeros_like(want)
    last = [bytes(12)] * batch
    for a in range(0, n, cut):
        part = np.clip(counts - a, 0, cut).astype(np.int32)
        pad = np.zeros((batch, cut, 40), np.uint8)
        pad[:, :min(cut, n - a)] = inp[:, a:a + cut]
        out = _process(qrl_ctx, rx, pad, part)
        state = rx.state().cpu().numpy()
        for b in range(batch):
            assert not out[b, part[b]:].any()
            got[b, a:a + part[b]] = out[b, :part[b]]
            if part[b]:
                last[b] = _public(out[b, part[b] - 1])
            assert bytes(state[b]) == last[b], (a, b)
    rx.close()
    _assert_same(got, want, "cut %d" % cut)


def test_reset_in_mid_assembly_equals_a_fresh_handle(qrl_ctx):
    import qradiolink_amd as q
    names = ["alias_format_3", "damaged_fragments", "alias_corners"]
    dirty = np.stack([G["inputs"][NAMES.index(n), :21] for n in names])      # header, three superframes, two fragments: an LC and an alias half built
    clean = ["whole_call", "alias_corners", "terminators"]
    inp, counts, want = _batch(clean)
    rx = q.DmrRx(qrl_ctx, 3, colour_code=1, promiscuous=True)
    _process(qrl_ctx, rx, dirty, None)
    assert rx.state().cpu().numpy().any()
    rx.set_config(1, False)
    again = _process(qrl_ctx, rx, inp, counts)
    assert (again != want).any(), "the carried state made no difference: the test shows nothing"
    rx.reset()
    assert not rx.state().cpu().numpy().any()
    got = _process(qrl_ctx, rx, inp, counts)
    rx.close()
    _assert_same(got, want)


def test_set_config_between_calls(qrl_ctx):
    import qradiolink_amd as q
    k, inp, want, cc, prom, reconfig = dmr_rx.scenario(G, "reconfigured")
    assert len(reconfig) == 2
    rx = q.DmrRx(qrl_ctx, 1, colour_code=cc, promiscuous=bool(prom))
    cuts = [0] + [slot for slot, _, _ in reconfig] + [inp.shape[0]]
    got = []
    for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if j:
            rx.set_config(reconfig[j - 1][1], bool(reconfig[j - 1][2]))
        got.append(_process(qrl_ctx, rx, inp[None, a:b], None)[0])
    _assert_same(np.concatenate(got), want)
    # and without the changes the second call's header is refused
    rx.reset()
    rx.set_config(cc, bool(prom))
    same = _process(qrl_ctx, rx, inp[None], None)[0]
    rx.close()
    assert dmr_rx.flags(same[8]) == dmr_rx.VALID and dmr_rx.flags(want[8]) & dmr_rx.HEADER_VOICE


def test_two_handles_on_two_streams_back_to_back(qrl_ctx):
    """layer 2 and the tracker of two handles queued on two HIP streams, three calls each, with no host synchronisation until the end"""
    import torch
    import qradiolink_amd as q
    lib = qrl_ctx.lib
    groups = [GROUPS["fixed"], GROUPS["promiscuous"]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    data, keep = [], []
    for names in groups:
        inp, counts, want = _batch(names)
        n = inp.shape[1]
        cuts = [0, n // 3, n // 3 + 5, n]
        data.append((inp, counts, want, cuts))
    rxs = [q.DmrRx(qrl_ctx, data[0][0].shape[0], colour_code=1), q.DmrRx(qrl_ctx, data[1][0].shape[0], colour_code=3, promiscuous=True)]
    torch.cuda.synchronize()
    outs = [[], []]
    for j in range(3):
        for h in range(2):
            inp, counts, want, cuts = data[h]
            a, b = cuts[j], cuts[j + 1]
            s = streams[h].cuda_stream
            with torch.cuda.stream(streams[h]):
                d_in = torch.from_numpy(np.ascontiguousarray(inp[:, a:b])).cuda()
                d_cnt = torch.from_numpy(np.clip(counts - a, 0, b - a).astype(np.int32)).cuda()
                l2 = torch.empty((inp.shape[0], b - a, 80), dtype=torch.uint8, device="cuda")
                out = torch.empty((inp.shape[0], b - a, 128), dtype=torch.uint8, device="cuda")
            assert lib.qrl_dmr_l2_decode(qrl_ctx.h, C.c_void_p(s), d_in.data_ptr(), d_cnt.data_ptr(), inp.shape[0], b - a, dmr_rx.AUDIO_FEC, l2.data_ptr()) == 0
            rxs[h].process(l2, d_cnt, out=out, stream=s)
            keep.append((d_in, d_cnt, l2))
            outs[h].append(out)
    torch.cuda.synchronize()
    for h in range(2):
        _assert_same(np.concatenate([o.cpu().numpy() for o in outs[h]], axis=1), data[h][2], "handle %d" % h)
        rxs[h].close()


def test_device_chain_through_enable_dmo_call(qrl_ctx):
    """qrl_dmr_voice_call_encode -> DMR modulator (1 Msps) -> DMR receiver -> DMO slicer -> layer 2 -> tracker, two streams, one call of 2 LC
    headers + 12 voice bursts + 2 terminators + 2 empty frames each (the batch and length of test_gpu_dmr_tx.py's loopback), received in three
    ragged calls.  Against the call descriptor: the header opens the call with its ids and colour code, every voice burst is audio, the
    first superframe delivers the call's LC and the second the alias header with the first six alias bytes (twelve voice bursts end there,
    so no alias completes), the terminator closes the call."""
    import torch
    import qradiolink_amd as q
    T = dmr_tx.load_golden()
    calls, voice, nv = T["calls"], T["call_voice"], dmr_tx.RADIO_VOICE
    ms = dmr_tx.RADIO_CALLS
    slots = [q.dmr_call_slots(calls[m], voice[m, :nv], stream=s) for s, m in enumerate(ms)]
    records = np.stack([r for r, _ in slots])
    n_slots = records.shape[1]
    rows = q.dmr_l2_encode(qrl_ctx, torch.from_numpy(records).cuda(), slot_bytes=q.DMR_SLOT_BYTES)
    built = q.dmr_voice_call_encode(qrl_ctx, torch.from_numpy(np.ascontiguousarray(calls[list(ms)])).cuda(),
                                    torch.from_numpy(np.ascontiguousarray(voice[list(ms), :nv])).cuda(), slot_bytes=q.DMR_SLOT_BYTES)
    assert torch.equal(rows[:, 2:2 + nv], built)
    rows[:, 2:2 + nv] = built
    rows = rows.reshape(2, n_slots * 72).contiguous()
    mod = q.Mod(qrl_ctx, q.MODEM_DMR, batch=2, max_bytes=rows.shape[1])
    iq = (mod.process(rows) * 0.05).contiguous()
    mod.close()
    n = iq.shape[1]
    dem = q.Demod(qrl_ctx, q.MODEM_DMR, batch=2, max_chunk=n)
    with pytest.raises(RuntimeError):
        dem.enable_dmo_call()
    dem.enable_dmo_sink(cap_frames=32)
    with pytest.raises(RuntimeError):
        dem.enable_dmo_call()
    dem.enable_dmo_l2(audio_fec=False)
    dem.enable_dmo_call(colour_code=0, promiscuous=True)
    assert dem.dmo_call.shape == (2, 32, 128)
    l2, rec = [[], []], [[], []]
    for a, b in zip([0, (n // 5) & ~1, (3 * n // 5 + 1234) & ~1], [(n // 5) & ~1, (3 * n // 5 + 1234) & ~1, n]):
        dem.process(iq[:, a:b].contiguous())
        cnt, x, y = dem.dmo_counts.cpu().numpy(), dem.dmo_l2.cpu().numpy(), dem.dmo_call.cpu().numpy()
        for s in range(2):
            c = min(int(cnt[s]), 32)
            assert not y[s, c:].any()
            l2[s].extend(x[s, :c])
            rec[s].extend(y[s, :c])
    state = dem.dmo_call_rx.state().cpu().numpy()
    for s, m in enumerate(ms):
        call = calls[m]
        x, y = np.stack(l2[s]), np.stack(rec[s])
        f = dmr_rx.flags(y)
        src, dst = int.from_bytes(bytes(call[0:3]), "big"), int.from_bytes(bytes(call[3:6]), "big")
        assert list(x[:, 3]) == [1, 1] + [0xF0 if k % 6 == 0 else 0xF1 for k in range(nv)] + [2], "stream %d: what the receiver delivered" % s
        assert (f & (dmr_rx.VALID | dmr_rx.PROCESSED) == dmr_rx.VALID | dmr_rx.PROCESSED).all()
        assert f[0] & dmr_rx.HEADER_VOICE and f[0] & dmr_rx.END_BEEP and f[1] & dmr_rx.HEADER_VOICE and not f[1] & dmr_rx.END_BEEP
        assert (y[:2 + nv, 2] == dmr_rx.AUDIO_STATE).all() and (y[:2 + nv, 3] == call[8] & 15).all() and (y[:2 + nv, 4] == call[6]).all()
        assert all(dmr_rx.ids(r) == (src, dst) for r in y[:2 + nv])
        assert ((f[2:2 + nv] & dmr_rx.AUDIO) != 0).all() and not (f[:2] & dmr_rx.AUDIO).any()
        emb = np.nonzero(f & dmr_rx.EMBEDDED)[0]
        assert list(emb) == [2 + 4, 2 + 10]
        own = bytes([call[6], call[7], 0]) + bytes(call[3:6]) + bytes(call[0:3])
        assert y[emb[0], 16] == call[6] and bytes(y[emb[0], 17:26]) == own
        assert y[emb[1], 16] == 4 and bytes(y[emb[1], 17:26]) == bytes([4, 0, 0x76]) + bytes(call[9:15])
        assert not (f & (dmr_rx.TALKER_ALIAS | dmr_rx.GPS | dmr_rx.UNKNOWN_FLCO)).any()
        assert f[-1] == dmr_rx.VALID | dmr_rx.PROCESSED | dmr_rx.TERMINATOR | dmr_rx.END_BEEP and y[-1, 2] == dmr_rx.IDLE
        assert bytes(state[s]) == bytes(12)
    # reset() resets the tracker too: a call cut off in the middle leaves nothing behind
    dem.process(iq[:, :(n // 2) & ~1].contiguous())
    assert dem.dmo_call_rx.state().cpu().numpy().any()
    dem.reset()
    dem.sync()
    assert not dem.dmo_call_rx.state().cpu().numpy().any()
    dem.close()
